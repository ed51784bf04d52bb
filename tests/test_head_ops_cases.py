"""CPU side of tests/test_gpu_head_ops.py: the wrappers' argument checks (they must refuse before any library call), the
references, and a census of the crafted decode inputs -- a later edit of the generator must not be able to drop an edge silently."""
import numpy as np
import pytest

import _head_ops_cases as H


def _sigmoid(v):
    from oracle import det
    v = np.asarray(v, dtype=np.float32)
    return (np.float32(1.0) / (np.float32(1.0) + det.expf(-v))).astype(np.float32)


@pytest.fixture
def no_library(monkeypatch):
    """any library call from a wrapper is a failure: validation comes first"""
    from cvsd_amd import _lib

    def boom():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(_lib, "lib", boom)


# ------------------------------------------------------------------------------------------------------------- ValueErrors
def test_decode_wrapper_refuses_bad_arguments(no_library):
    from cvsd_amd import ops
    buf = np.zeros((2, 3, 3, 72), np.float32)
    lv = (buf, 0, 64, 0, 8)
    bad = [
        dict(levels=[lv], nc=4, mode="dense"),                                   # unknown mode
        dict(levels=[lv], nc=4, mode="split"),                                   # split without a gate
        dict(levels=[lv], nc=4, mode="nms", gate=1),                             # a gate without split
        dict(levels=[], nc=4),                                                   # no level
        dict(levels=[lv] * 5, nc=4),                                             # more than 4
        dict(levels=[lv], nc=0),
        dict(levels=[lv], nc=4, nkpt=2, kdim=4),
        dict(levels=[lv], nc=4, nkpt=0, kdim=3),
        dict(levels=[lv], nc=4, nkpt=2, kdim=0),
        dict(levels=[(buf[0], 0, 64, 0, 8)], nc=4),                              # not [n, h, w, cs]
        dict(levels=[lv, (np.zeros((1, 2, 2, 72), np.float32), 0, 64, 0, 16)], nc=4),      # frames differ between levels
        dict(levels=[(buf, 12, 64, 0, 8)], nc=4),                                # 64 box logits from 12 do not fit 72
        dict(levels=[(buf, -4, 64, 0, 8)], nc=4),
        dict(levels=[(buf, 0, 64, 0, 8)], nc=9),                                 # classes run past cs
        dict(levels=[(buf, 0, 64, 68, 8)], nc=2, nkpt=2, kdim=3),                # keypoints run past cs
        dict(levels=[(buf, 0, 64, 0, 0)], nc=4),                                 # stride
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.decode(**kw)


def test_sppf_wrapper_refuses_bad_arguments(no_library):
    from cvsd_amd import ops
    x = np.zeros((1, 4, 4, 24), np.float32)
    bad = [
        dict(x_nhwc=x, c=6),                                                     # c % 4
        dict(x_nhwc=x, c=0),
        dict(x_nhwc=x, c=8, x_off=2),                                            # view not 16-byte aligned
        dict(x_nhwc=x, c=8, x_off=20),                                           # view past the tensor
        dict(x_nhwc=x, c=8, x_off=-4),
        dict(x_nhwc=x[..., :22], c=8),                                           # pixel stride not 16-byte aligned
        dict(x_nhwc=x[0], c=8),
        dict(x_nhwc=x, c=8, y=np.zeros((1, 4, 4, 24), np.float32), y_off=4),     # 3c from 4 does not fit 24
        dict(x_nhwc=x, c=8, y=np.zeros((1, 4, 4, 26), np.float32)),
        dict(x_nhwc=x, c=8, y=np.zeros((1, 4, 4, 32), np.float32), y_off=6),
        dict(x_nhwc=x, c=8, y=np.zeros((1, 4, 5, 32), np.float32)),              # another map
        dict(x_nhwc=x, c=12, half=True),                                         # fp16: 8 halfs per 16 bytes
        dict(x_nhwc=x, c=8, x_off=4, half=True),
        dict(x_nhwc=x[..., :20], c=8, half=True),
        dict(x_nhwc=x, c=8, y=np.zeros((1, 4, 4, 32), np.float32), y_off=4, half=True),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.sppf_pools(**kw)


def test_upsample_wrapper_refuses_bad_arguments(no_library):
    from cvsd_amd import ops
    x = np.zeros((1, 2, 2, 12), np.uint32)
    bad = [
        dict(x_nhwc=x, c=0),
        dict(x_nhwc=x, c=6, x_off=2),
        dict(x_nhwc=x, c=6, x_off=8),                                            # 8 + 6 > 12
        dict(x_nhwc=x[..., :10], c=6),
        dict(x_nhwc=x[0], c=6),
        dict(x_nhwc=x.astype(np.float64), c=6),                                  # not 32-bit words
        dict(x_nhwc=x.astype(np.uint16), c=6),
        dict(x_nhwc=x, c=6, y=np.zeros((1, 4, 4, 6), np.uint32)),                # y's stride
        dict(x_nhwc=x, c=6, y=np.zeros((1, 4, 4, 8), np.uint32), y_off=4),
        dict(x_nhwc=x, c=6, y=np.zeros((1, 2, 2, 8), np.uint32)),                # not the doubled map
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.upsample2x(**kw)


def test_sentinel_is_a_quiet_nan_that_keeps_its_payload():
    from cvsd_amd import ops
    a = ops._sentinel((3, 5))
    assert a.dtype == np.float32 and np.isnan(a).all() and (a.view(np.uint32) == ops.SENTINEL_BITS).all()
    assert np.isnan(a.astype(np.float16)).all()                                  # the fp16 pool path keeps it a NaN


# -------------------------------------------------------------------------------------------------------------- references
def test_sppf_reference_is_the_5_9_13_window_maximum():
    """three chained 5-windows == the 5-, 9- and 13-window of the input, borders included: on maps wider and thinner than the windows"""
    for (n, h, w, c), half in (((2, 15, 17, 4), False), ((1, 2, 3, 8), True), ((1, 4, 9, 4), False), ((1, 1, 1, 8), True)):
        x = H.sppf_input(n, h, w, c, half, seed=h * w)
        ref = H.sppf_reference(x)
        assert not np.isnan(ref).any()
        for i, r in enumerate((2, 4, 6)):
            np.testing.assert_array_equal(ref[..., i * c:(i + 1) * c], H.window_max(x, r))
    # and it tells a zero-padded pool from the real one: the corner of a map of negatives
    x = H.sppf_input(1, 6, 6, 4, False, seed=1)
    assert (H.sppf_reference(x)[0, 0, 0] < 0).any()


def test_sppf_inputs_hold_their_edge_values():
    for half, big, sub in ((False, 3.0e38, 2.0 ** -126), (True, 65504.0, 2.0 ** -14)):
        x = H.sppf_input(2, 20, 20, 40, half, seed=3)
        assert not np.isnan(x).any()
        assert (x == -np.inf).any() and (x == big).any() and (x == -big).any()
        assert ((x > 0) & (x < sub)).any() and ((x < 0) & (x > -sub)).any()
        assert np.median(x) < -2 and (x < 0).mean() > 0.9
        if half:
            np.testing.assert_array_equal(x, x.astype(np.float16).astype(np.float32))


@pytest.mark.parametrize("n,h,w,c,half,branch", H.SPPF_CASES)
def test_sppf_cases_reach_the_branch_they_name(n, h, w, c, half, branch):
    assert H.sppf_branch(n, h, w, c, half) == branch
    cx, x_off, cy, y_off = H.sppf_view(c, half)
    al = 8 if half else 4
    assert cx > x_off + c - 1 and x_off > 0 and cy == 4 * c and y_off == c and not (cx % al or x_off % al or c % al)


def test_sppf_cases_cover_every_launcher_branch():
    seen = {(half, b[:2] if b[0] == "lds" else b) for *_, half, b in H.SPPF_CASES}
    assert {(False, ("lds", p)) for p in (16, 8, 4)} | {(True, ("lds", p)) for p in (32, 16, 8)} <= seen
    assert {(hf, ("global", cap)) for hf in (False, True) for cap in (False, True)} <= seen
    assert any(b == ("lds", 16, True) for *_, hf, b in H.SPPF_CASES if not hf) and any(b == ("lds", 32, True) for *_, hf, b in H.SPPF_CASES if hf)
    assert any(h < 5 and w < 5 for _, h, w, *_ in H.SPPF_CASES)


def test_upsample_cases_and_reference():
    assert {c % 4 for *_, c in H.UPSAMPLE_CASES} >= {0, 2, 3}                    # whole vectors, and tails of 2 and 3 words
    assert [H.upsample_blocks(*s) > 4096 for s in H.UPSAMPLE_CASES].count(True) == 1
    x = np.arange(2 * 2 * 3 * 8, dtype=np.uint32).reshape(2, 2, 3, 8)
    y = np.full((2, 4, 6, 12), 7, np.uint32)
    out = H.upsample_reference(x, 3, 4, y, 8)
    assert (out[..., :8] == 7).all() and (out[..., 11] == 7).all()
    for oy in range(4):
        for ox in range(6):
            np.testing.assert_array_equal(out[:, oy, ox, 8:11], x[:, oy // 2, ox // 2, 4:7])
    pat = H.upsample_input((3, 5, 7, 12), seed=0)
    assert np.isnan(pat.view(np.float32)).any() and (pat == 0xFFFFFFFF).any() and (pat == 0x7F800001).any()


def test_best_of_returns_the_first_argmax():
    pred = np.zeros((1, 2, 4 + 5), np.float32)
    pred[0, 0, 4:] = [0.1, 0.7, 0.7, 0.2, 0.7]
    pred[0, 1, 4:] = [0.0, 0.0, 0.0, 0.0, 0.0]
    np.testing.assert_array_equal(H.best_of(pred, 5), np.array([[[0.7, 1.0], [0.0, 0.0]]], np.float32))


# ------------------------------------------------------------------------------------------------- census of the decode inputs
def test_decode_cases_cover_both_row_store_forms():
    nos = {(4 + nc + nkpt * kdim) % 4 == 0 for nc, _, (nkpt, kdim) in H.DECODE_CASES}
    assert nos == {True, False}
    assert {H.uses_float4_class_loads(nc, off) for nc, off, _ in H.DECODE_CASES} == {True, False}
    assert len(H.DECODE_CASES) == 7 * 2 * 4


def test_tie_placements_exist_where_the_class_count_has_room():
    assert set(H.tie_pairs(80, True)) == {"same_lane", "low_class_in_high_lane", "same_float4"}
    assert set(H.tie_pairs(4, True)) == {"same_float4"}
    for nc in (5, 80, 81):
        assert set(H.tie_pairs(nc, False)) == {"same_lane", "low_class_in_high_lane", "ascending_lanes"}
    assert set(H.tie_pairs(2, False)) == {"ascending_lanes"} and H.tie_pairs(1, False) == {}
    for nc, vec in ((80, True), (81, False)):          # with room to choose, class 0 is not part of a tie
        for a, b in H.tie_pairs(nc, vec).values():
            assert 0 < a < b < nc


@pytest.mark.parametrize("nc,cls_off", [(nc, off) for nc in H.NCS for off in H.CLS_OFFS])
def test_crafted_class_rows_contain_what_they_claim(nc, cls_off):
    """read back from the data of the case the GPU tests decode (the generator's tags are only checked for the N(0, 1) flavours)"""
    case = H.decode_case(nc, cls_off, 0, 0)
    L, vec = case.cls, case.vec
    assert L.shape == (153, nc) and np.isfinite(L).all()
    tags = set(case.cls_tags)
    assert {f"normal:{s}:{sh}" for s, sh in H.NORMAL_FLAVOURS} <= tags
    seen = H.class_census(L, vec, _sigmoid)
    for placement in H.tie_pairs(nc, vec):
        assert seen[f"tie:{placement}"] >= 2, (placement, seen)
    if nc >= 3:
        assert seen["tie:first_class_is_not_0"] >= 1
    for v in H.SEAMS:
        assert seen[f"seam:{v!r}"] >= 1, (v, seen)
    assert seen["underflow"] >= 2 and seen["all_equal"] >= 2
    assert seen["underflow:all_scores_zero"] >= 1 and seen["underflow:subnormal_score"] >= 1
    if nc >= 2:
        assert seen["saturated"] >= 2
    if nc >= 3:                                        # a maximum and a logit on either side of max - 0.01
        assert seen["seam:logits_on_both_sides_of_the_window_edge"] >= 3
    if nc >= 4:
        assert seen["saturated:equal_scores_from_unequal_logits_and_first_is_not_the_largest"] >= 1
    # the regimes of the window's threshold are all visited by the row maxima
    m = L.max(1)
    assert (m > 11).any() and (m < -80).any() and ((m <= 11) & (m >= -80)).any()


def test_crafted_box_rows_and_keypoints_contain_what_they_claim():
    case = H.decode_case(80, 64, 17, 3)
    seen = H.box_census(case.box)
    for kind in ("all_equal", "one_hot_0", "one_hot_15", "peaked"):
        assert seen[kind] >= 20, seen
    # all-equal sides decode to distance 7.5 on every side: a box of 15 strides centred on the anchor
    rows = [i for i, t in enumerate(case.box_tags) if t == "all_equal"]
    ref = case.ref_pred.reshape(-1, case.no)
    strides = np.concatenate([np.full(h * w, s, np.float32) for h, w, s in H.DECODE_LEVELS] * H.DECODE_N)
    np.testing.assert_allclose(ref[rows, 2], 15 * strides[rows], rtol=1e-5)
    np.testing.assert_allclose(ref[rows, 3], 15 * strides[rows], rtol=1e-5)
    # the tiny case carries a tie
    tiny = H.decode_case(80, 64, 17, 3, True)
    assert tiny.cls.shape == (1, 80) and tiny.cls_tags[0].startswith("tie:") and (tiny.cls[0] == tiny.cls[0].max()).sum() == 2
    # frame() is the frame's slice of every level
    one = case.frame(1)
    assert all(a[0].shape[0] == 1 and np.array_equal(a[0][0], b[0][1]) and a[1:] == b[1:] for a, b in zip(one, case.levels))


def test_decode_reference_is_anchor_major_and_its_best_is_the_first_argmax():
    case = H.decode_case(5, 66, 5, 3)
    assert case.ref_pred.shape == (3, 51, 4 + 5 + 15) and case.ref_best.shape == (3, 51, 2)
    sc = _sigmoid(case.cls).reshape(3, 51, 5)
    np.testing.assert_array_equal(case.ref_pred[:, :, 4:9], sc)
    np.testing.assert_array_equal(case.ref_best[:, :, 0], sc.max(2))
    np.testing.assert_array_equal(case.ref_best[:, :, 1], sc.argmax(2))
    ties = [i for i, t in enumerate(case.cls_tags) if t.startswith("tie:")]
    pairs = H.tie_pairs(5, False)
    checked = 0
    for i in ties:
        if -70 < case.cls[i].max() < 5:            # where fp32 scores of logits 0.005 apart cannot collide
            assert case.ref_best.reshape(-1, 2)[i, 1] == pairs[case.cls_tags[i][4:]][0]
            checked += 1
    assert checked >= 3


def test_entry_points_refuse_bad_arguments_before_touching_a_device():
    """the C side repeats the checks for callers that do not come through ops.py: MI355_EINVAL (-1), no GPU needed"""
    import ctypes as C
    from cvsd_amd import _lib
    L = _lib.lib()
    x = np.zeros((1, 2, 2, 80), np.float32)
    y = np.zeros((1, 4, 4, 80), np.float32)
    p, q = x.ctypes.data, y.ctypes.data
    assert L.mi355_op_sppf_pools(0, p, 1, 2, 2, 80, 0, 6, q, 80, 0, 0) == -1          # c % 4
    assert L.mi355_op_sppf_pools(0, p, 1, 2, 2, 80, 4, 8, q, 80, 0, 1) == -1          # fp16 view not 16-byte aligned
    assert L.mi355_op_sppf_pools(0, p, 1, 2, 2, 80, 0, 32, q, 80, 0, 0) == -1         # 3c > y_cs
    assert L.mi355_op_sppf_pools(0, None, 1, 2, 2, 80, 0, 8, q, 80, 0, 0) == -1
    assert L.mi355_op_upsample2x(0, p, 1, 2, 2, 80, 2, 8, q, 80, 0) == -1
    assert L.mi355_op_upsample2x(0, p, 1, 2, 2, 80, 76, 8, q, 80, 0) == -1
    assert L.mi355_op_upsample2x(0, p, 1, 2, 2, 80, 0, 0, q, 80, 0) == -1
    bufs = (C.c_void_p * 5)(*[p] * 5)
    geom = (C.c_int * 35)(*[80, 0, 64, 0, 2, 2, 8] * 5)
    cnt = C.c_int(0)
    pred, best = q, q
    assert L.mi355_op_decode(0, bufs, geom, 5, 1, 4, 0, 0, 0, 0, pred, best, C.byref(cnt)) == -1     # 5 levels
    assert L.mi355_op_decode(0, bufs, geom, 0, 1, 4, 0, 0, 0, 0, pred, best, C.byref(cnt)) == -1
    assert L.mi355_op_decode(0, bufs, geom, 1, 1, 4, 0, 0, 3, 0, pred, best, C.byref(cnt)) == -1     # mode
    assert L.mi355_op_decode(0, bufs, geom, 1, 1, 4, 2, 4, 0, 0, pred, best, C.byref(cnt)) == -1     # kdim
    assert L.mi355_op_decode(0, bufs, geom, 1, 1, 17, 0, 0, 0, 0, pred, best, C.byref(cnt)) == -1    # 64 + 17 > 80
    assert L.mi355_op_decode(0, bufs, geom, 1, 1, 4, 27, 3, 0, 0, pred, best, C.byref(cnt)) == -1    # 81 keypoint values past cs
    assert b"levels" in L.mi355_last_error() or b"slice" in L.mi355_last_error()
