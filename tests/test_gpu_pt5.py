"""The five-pixel-tile wave shapes of conv_igemm_f32 (blocks of 80 / 160 / 320 pixels for 20x20 and 40x40 maps) and the halo
staging's remainder batches: every candidate launch plan against the canonical-order oracle, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _data(n, h, w, cin, cout, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, cin), dtype=np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    return rng, x, wt, b


def _every_plan(x, wt, b, stride, silu, res):
    """-> the planner's view of the candidates that were run, after checking each against the oracle"""
    from cvsd_amd import ops
    from oracle import det
    n, h, w, cin = x.shape
    ref = det.conv2d(x, wt, b, stride=stride, act=silu, residual=res)
    y, n_plans = ops.conv2d(x, wt, b, stride=stride, silu=silu, residual=res, plan=0, return_n_plans=True)
    np.testing.assert_array_equal(y, ref)
    for plan in range(1, n_plans):
        np.testing.assert_array_equal(ops.conv2d(x, wt, b, stride=stride, silu=silu, residual=res, plan=plan), ref,
                                      err_msg=f"plan {plan} of {n_plans}")
    cout = wt.shape[0]
    tiles = ops.plan_tiles(n, h, w, cin, cout, 3, stride, res_cs=(cout + 3) // 4 * 4 if res is not None else 0)
    assert len(tiles) == n_plans
    return tiles


@pytest.mark.parametrize("n,h,w,cin,cout,stride,silu,residual,blocks", [
    (256, 20, 20, 16, 32, 1, True, True, {80}),             # 20x4 tiles
    (256, 20, 20, 48, 51, 1, True, False, {80}),            # ragged Cout: the dword store path
    (256, 40, 40, 16, 32, 2, True, False, {80}),            # stride 2 onto 20x20
    (64, 40, 40, 16, 80, 1, True, False, {160, 320}),       # 40x4 / 40x8 tiles, five cout tiles
])
def test_five_pixel_tile_plans_give_the_oracles_bits(n, h, w, cin, cout, stride, silu, residual, blocks):
    rng, x, wt, b = _data(n, h, w, cin, cout, cin * 100 + cout + stride)
    res = rng.standard_normal((n, h // stride, w // stride, cout), dtype=np.float32) if residual else None
    tiles = _every_plan(x, wt, b, stride, silu, res)
    pt5 = [p for p in tiles if p["PT"] == 5 and p["version"] == 1]
    assert pt5 and blocks <= {p["P"] for p in pt5}, sorted({(p["PT"], p["P"]) for p in tiles})
    for p in pt5:
        assert p["tiles_x"] * p["tiles_y"] * p["P"] == (h // stride) * (w // stride)


def test_a_map_no_block_of_80_pixels_tiles_exactly_is_offered_none():
    """the planner's rule: PT = 5 only for an exact cover; 22x20 has none, and its candidates give the oracle's bits as before"""
    rng, x, wt, b = _data(256, 20, 22, 16, 32, 5)
    res = rng.standard_normal((256, 20, 22, 32), dtype=np.float32)
    tiles = _every_plan(x, wt, b, 1, True, res)
    assert all(p["PT"] != 5 for p in tiles)


@pytest.mark.parametrize("n,h,w,cin,c1,stride,c2,silu2", [
    (256, 40, 40, 16, 32, 2, 32, False), (256, 40, 40, 16, 32, 2, 32, True),
    (64, 40, 40, 32, 32, 1, 48, False), (64, 40, 40, 32, 32, 1, 48, True),
])
def test_fused_pointwise_stage_behind_five_pixel_tiles(n, h, w, cin, c1, stride, c2, silu2):
    """the first conv's LDS image [P pixels][channels] at P = 80 / 160 / 320 and the second stage's per-tile offsets"""
    from cvsd_amd import ops
    from oracle import det
    rng, x, w1, b1 = _data(n, h, w, cin, c1, cin + c1 + c2 + stride)
    w2 = (rng.standard_normal((c2, c1, 1, 1)) / np.sqrt(c1)).astype(np.float32)
    b2 = rng.standard_normal(c2).astype(np.float32)
    ref = det.conv2d(det.conv2d(x, w1, b1, stride=stride, act=True), w2, b2, stride=1, act=silu2)
    y, n_plans = ops.conv2d_fused(x, w1, b1, w2, b2, stride=stride, silu2=silu2, plan=0, return_n_plans=True)
    np.testing.assert_array_equal(y, ref)
    for plan in range(1, n_plans):
        np.testing.assert_array_equal(ops.conv2d_fused(x, w1, b1, w2, b2, stride=stride, silu2=silu2, plan=plan), ref,
                                      err_msg=f"fused plan {plan} of {n_plans}")
    tiles = ops.plan_tiles(n, h, w, cin, c1, 3, stride, f2_cout=c2)
    assert len(tiles) == n_plans and all(p["version"] == 101 for p in tiles)
    assert any(p["PT"] == 5 for p in tiles), sorted({(p["PT"], p["P"]) for p in tiles})


@pytest.mark.parametrize("n,h,w,cin,cout", [
    (1, 7, 9, 16, 16),          # small halos: the staging loop's remainder pieces (1 .. 7 slots per thread), every candidate tile
    (2, 33, 31, 80, 16),        # ... and a second channel chunk of 16 behind one of 64
])
def test_halo_staging_remainders(n, h, w, cin, cout):
    rng, x, wt, b = _data(n, h, w, cin, cout, h * w + cin)
    _every_plan(x, wt, b, 1, True, None)
