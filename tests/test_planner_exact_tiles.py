"""The planner's five-pixel-tile wave shapes (blocks of 80 / 160 / 320 pixels), host-only: they are offered where -- and only
where -- the default wave tile cannot cover the map without computing pixels that do not exist (20x20, 40x40), and every other
shape keeps the candidate list it had before they existed."""
import pytest

from cvsd_amd import ops


@pytest.mark.parametrize("kw", [
    dict(n=512, h=20, w=20, cin=128, cout=128, k=3, stride=1),
    dict(n=512, h=40, w=40, cin=128, cout=256, k=3, stride=2),      # 40x40 -> 20x20
    dict(n=512, h=40, w=40, cin=80, cout=80, k=3, stride=1),
    dict(n=512, h=20, w=20, cin=256, cout=144, k=3, stride=1),      # the head's merged cv2.2.0 + cv3.2.0
])
def test_maps_of_20x20_and_40x40_get_a_tiling_without_padded_pixels(kw):
    wo, ho = kw["w"] // kw["stride"], kw["h"] // kw["stride"]
    plans = ops.plan_tiles(**kw)
    assert [p["version"] for p in plans] == ops.plan_versions(**kw)
    exact = [p for p in plans if p["version"] == 1 and p["tiles_x"] * p["tiles_y"] * p["P"] == wo * ho]
    assert exact and any(p["P"] % 80 == 0 for p in exact), [(p["PT"], p["WP"], p["TW"], p["TH"]) for p in plans]
    for p in plans:
        if p["PT"] == 5:                                            # offered under the narrow rule only: exact, CT <= 3
            assert p["version"] == 1 and p["CT"] <= 3 and p["P"] == p["WP"] * 80 and p["TW"] * p["TH"] == p["P"]
            assert p["tiles_x"] * p["tiles_y"] * p["P"] == wo * ho, p
            assert p["grid_x"] == kw["n"] * p["tiles_x"] * p["tiles_y"]


# what mi355_plan_query returned for these shapes before the five-pixel-tile shapes existed
UNCHANGED = [
    (dict(n=512, h=80, w=80, cin=64, cout=64, k=3), [1] * 23),
    (dict(n=512, h=160, w=160, cin=16, cout=16, k=3), [1] * 7),
    (dict(n=1, h=20, w=20, cin=128, cout=128, k=3), [6, 1] * 8 + [1] * 67),
    (dict(n=8, h=80, w=80, cin=64, cout=64, k=3, f2_cout=64), [101] * 41),
]


@pytest.mark.parametrize("kw,versions", UNCHANGED)
def test_maps_that_tile_exactly_and_latency_bound_launches_keep_their_candidates(kw, versions):
    plans = ops.plan_tiles(**kw)
    assert all(p["PT"] != 5 for p in plans)
    assert ops.plan_versions(**kw) == versions
    assert [p["version"] for p in plans] == versions


def test_a_ragged_map_is_offered_no_five_pixel_tile_shape():
    """22x20 is tiled exactly by neither block size: the rule offers PT = 5 only for an exact cover"""
    assert all(p["PT"] != 5 for p in ops.plan_tiles(256, 20, 22, 16, 32, 3))
