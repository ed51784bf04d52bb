"""The five-cout-tile small wave shapes of conv_igemm_f32 (PT 2 / PT 1 x CT 5, all four waves along the pixels: blocks of 128 / 64
pixels that take 80 couts in one block along grid.y), plain, fused and as the class sub-range launch of a merged head conv: every
candidate launch plan against the canonical-order oracle, bit for bit.  All maps are 16x16 (128 = 16x8 and 64 = 8x8 tile it exactly)
and all cases run 256 images of 16+ channels, which keeps the launch in the planner's throughput regime, where the rule applies."""
import numpy as np
import pytest

gpu = pytest.mark.gpu


def _data(n, h, w, cin, cout, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, cin), dtype=np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    return rng, x, wt, b


def _is_ct5(p, pt=None):
    return p["CT"] == 5 and (p["PT"] in (1, 2) if pt is None else p["PT"] == pt)


@gpu
@pytest.mark.parametrize("cin,cout,silu,residual", [
    (16, 80, True, True),           # a: full cout tiles, SiLU, residual
    (16, 75, True, False),          # b: ragged last tile, the dword store path
    (80, 80, True, False),          # c: five k-blocks, a second staged chunk of 16 behind one of 64
])
def test_five_cout_tile_plans_give_the_oracles_bits(cin, cout, silu, residual):
    from cvsd_amd import ops
    from oracle import det
    n, h, w = 256, 16, 16
    rng, x, wt, b = _data(n, h, w, cin, cout, cin * 100 + cout)
    res = rng.standard_normal((n, h, w, cout), dtype=np.float32) if residual else None
    ref = det.conv2d(x, wt, b, stride=1, act=silu, residual=res)
    y, n_plans = ops.conv2d(x, wt, b, stride=1, silu=silu, residual=res, plan=0, return_n_plans=True)
    np.testing.assert_array_equal(y, ref)
    for plan in range(1, n_plans):
        np.testing.assert_array_equal(ops.conv2d(x, wt, b, stride=1, silu=silu, residual=res, plan=plan), ref,
                                      err_msg=f"plan {plan} of {n_plans}")
    tiles = ops.plan_tiles(n, h, w, cin, cout, 3, 1, res_cs=(cout + 3) // 4 * 4 if residual else 0)
    assert len(tiles) == n_plans
    for pt, block in ((2, 128), (1, 64)):
        ct5 = [p for p in tiles if _is_ct5(p, pt)]
        assert ct5, sorted({(p["PT"], p["CT"], p["WP"]) for p in tiles})
        for p in ct5:
            assert p["version"] == 1 and p["WP"] == 4 and p["P"] == block and p["grid_y"] == 1
            assert p["tiles_x"] * p["tiles_y"] * p["P"] == h * w and p["grid_x"] == n * p["tiles_x"] * p["tiles_y"]


@gpu
def test_class_subrange_of_a_merged_head_conv():
    """d: 16 -> 144 plain (64 box couts + 80 class couts), launched over cout tiles 4 .. 8 alone as a sparse pass launches it: the class
    couts get the oracle's bits from every plan, the box couts keep what the buffer held, and five-cout-tile plans run with grid.y 1"""
    from cvsd_amd import ops
    from oracle import det
    n, h, w, cin, cout, t0 = 256, 16, 16, 16, 144, 4
    rng, x, wt, b = _data(n, h, w, cin, cout, 144)
    ref = det.conv2d(x, wt, b, stride=1, act=False)
    held = rng.standard_normal((n, h, w, cout), dtype=np.float32)
    want = np.concatenate([held[..., :16 * t0], ref[..., 16 * t0:]], axis=-1)
    y, n_plans, tile = ops.conv2d_subrange(x, wt, b, t0, held, silu=False, plan=0)
    np.testing.assert_array_equal(y, want)
    tiles = [tile]
    for plan in range(1, n_plans):
        y, _, tile = ops.conv2d_subrange(x, wt, b, t0, held, silu=False, plan=plan)
        np.testing.assert_array_equal(y, want, err_msg=f"plan {plan} of {n_plans}")
        tiles.append(tile)
    for pt, block in ((2, 128), (1, 64)):
        ct5 = [p for p in tiles if _is_ct5(p, pt)]
        assert ct5, sorted({(p["PT"], p["CT"], p["WP"]) for p in tiles})
        for p in ct5:
            assert p["P"] == block and p["grid_y"] == 1 and p["tiles_x"] * p["tiles_y"] * p["P"] == h * w
    # the whole nine-tile conv is offered no such plan: five tiles do not cover nine
    assert not any(_is_ct5(p) for p in ops.plan_tiles(n, h, w, cin, cout, 3))


@gpu
@pytest.mark.parametrize("c2,silu2", [(80, False), (80, True), (51, False)])
def test_fused_pointwise_stage_behind_five_cout_tiles(c2, silu2):
    """all 80 first-conv channels of a block in its LDS image with no idle wave; c2 = 51: the second stage's ragged last tile"""
    from cvsd_amd import ops
    from oracle import det
    n, h, w, cin, c1 = 256, 16, 16, 16, 80
    rng, x, w1, b1 = _data(n, h, w, cin, c1, c1 + c2 + int(silu2))
    w2 = (rng.standard_normal((c2, c1, 1, 1)) / np.sqrt(c1)).astype(np.float32)
    b2 = rng.standard_normal(c2).astype(np.float32)
    ref = det.conv2d(det.conv2d(x, w1, b1, stride=1, act=True), w2, b2, stride=1, act=silu2)
    y, n_plans = ops.conv2d_fused(x, w1, b1, w2, b2, stride=1, silu2=silu2, plan=0, return_n_plans=True)
    np.testing.assert_array_equal(y, ref)
    for plan in range(1, n_plans):
        np.testing.assert_array_equal(ops.conv2d_fused(x, w1, b1, w2, b2, stride=1, silu2=silu2, plan=plan), ref,
                                      err_msg=f"fused plan {plan} of {n_plans}")
    tiles = ops.plan_tiles(n, h, w, cin, c1, 3, 1, f2_cout=c2)
    assert len(tiles) == n_plans and all(p["version"] == 101 for p in tiles)
    assert any(_is_ct5(p, 2) for p in tiles) and any(_is_ct5(p, 1) for p in tiles), sorted({(p["PT"], p["CT"]) for p in tiles})


@pytest.mark.parametrize("kw", [
    dict(n=512, h=160, w=160, cin=16, cout=16, k=3),        # one cout tile
    dict(n=512, h=80, w=80, cin=64, cout=64, k=3),          # four cout tiles
    dict(n=256, h=20, w=22, cin=80, cout=80, k=3),          # five cout tiles, but neither 128 nor 64 pixels tile 22x20 exactly
    dict(n=512, h=40, w=40, cin=128, cout=80, k=3, stride=2),   # the rule names stride 1
    dict(n=1, h=80, w=80, cin=80, cout=80, k=3),            # latency-bound
])
def test_shapes_the_rule_does_not_name_are_offered_no_five_cout_small_tile(kw):
    """host-only: CT 5 over PT 2 / PT 1 needs five-fold cout tiles, an exact cover, stride 1 and the throughput regime"""
    from cvsd_amd import ops
    assert not any(_is_ct5(p) for p in ops.plan_tiles(**kw))


def test_the_80x80_and_40x40_class_convs_are_offered_exact_five_cout_tile_blocks():
    """host-only: 80 -> 80 at 80x80 gets blocks of 128 (16x8) and 64 (8x8) pixels, at 40x40 the 8x8 block alone (128 pixels have no exact
    cover of 1,600); plain and with the 1x1 fused behind"""
    from cvsd_amd import ops
    for f2 in (0, 80):
        big = [p for p in ops.plan_tiles(512, 80, 80, 80, 80, 3, f2_cout=f2) if _is_ct5(p)]
        assert {(p["PT"], p["TW"], p["TH"]) for p in big} == {(2, 16, 8), (1, 8, 8)} and all(p["grid_y"] == 1 for p in big)
        mid = [p for p in ops.plan_tiles(512, 40, 40, 80, 80, 3, f2_cout=f2) if _is_ct5(p)]
        assert {(p["PT"], p["TW"], p["TH"]) for p in mid} == {(1, 8, 8)} and all(p["grid_y"] == 1 for p in mid)
