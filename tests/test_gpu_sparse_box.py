"""The three kernels of the sparse box branch (csrc/conv_f32_sparse.hip: the lists kernel and the two gathered convs) alone,
through the C ABI (cvsd_amd.ops.sparse_box), against a numpy statement of the lists and the canonical-order oracle's dense box
chain (oracle.det) restricted to the listed positions.  Every comparison is equality of bits; the order inside a list depends on
atomics and is not pinned, so lists are compared sorted.

Inputs, cases and references: tests/_sparse_box_cases.py (checked on the CPU by tests/test_sparse_box_cases.py)."""
import functools

import numpy as np
import pytest

import _sparse_box_cases as S

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _sentinel_mask(a):
    from cvsd_amd import ops
    return _bits(a) == ops.SENTINEL_BITS


@functools.lru_cache(maxsize=None)
def _run(name):
    """one launch per case, shared by the tests that look at its parts"""
    from cvsd_amd import ops
    c = S.case(name)
    return ops.sparse_box(c.inputs, c.best, c.conf, c.nc, no=c.no, classes=c.classes)


def _first_difference(got, want, what):
    """index and both words of the first mismatch: which position, which channel"""
    bad = np.argwhere(_bits(got) != _bits(want))
    if len(bad):
        i = tuple(bad[0])
        pytest.fail(f"{what}: {len(bad)} words differ, first at {i}: got {got[i]!r} ({_bits(got)[i]:#010x}), want {want[i]!r} ({_bits(want)[i]:#010x})")


def _expected_mid(c, l):
    from cvsd_amd import ops
    h, w, _ = c.shapes[l]
    cs, off = c.mid
    want = ops._sentinel((c.n * h * w, cs))
    want[c.ref_dil[l], off:off + 64] = c.ref_mid[l].reshape(-1, 64)[c.ref_dil[l]]
    return want.reshape(c.n, h, w, cs)


def _expected_pred(c):
    from cvsd_amd import ops
    want = ops._sentinel((c.n, c.A, c.no))
    want[..., :4][c.cand] = c.ref_box[c.cand]
    return want


def _check_lists(c, r):
    assert r.overflow == 0
    assert r.n_dil == [len(e) for e in c.ref_dil] and r.n_cand == [len(e) for e in c.ref_cand]
    for l in range(len(c.shapes)):
        for kind, got, want in (("dilated", r.dil[l], c.ref_dil[l]), ("candidate", r.cand[l], c.ref_cand[l])):
            assert got.dtype == np.int32 and len(np.unique(got)) == len(got), f"level {l}: duplicates in the {kind} list"
            np.testing.assert_array_equal(np.sort(got), want, err_msg=f"level {l}, {kind} list")


@pytest.mark.parametrize("name", S.PLAIN_CASES)
def test_lists_hold_the_reference_positions(name):
    """sorted entries, no duplicates, all six counts, no overflow"""
    _check_lists(S.case(name), _run(name))


@pytest.mark.parametrize("name", S.PLAIN_CASES)
def test_mid_has_the_oracle_bits_at_the_dilated_pixels_and_nothing_else(name):
    """cv2.i.0 at the dilated pixels: the 64 channels of the slice bit for bit; every other word of mid keeps the sentinel"""
    c, r = S.case(name), _run(name)
    for l in range(len(c.shapes)):
        assert r.mid[l].shape == (c.n,) + c.shapes[l][:2] + (c.mid[0],)
        _first_difference(r.mid[l], _expected_mid(c, l), f"{name}: mid of level {l} [frame, y, x, channel]")


@pytest.mark.parametrize("name", S.PLAIN_CASES)
def test_pred_has_the_oracle_boxes_at_the_candidates_and_nothing_else(name):
    """cv2.i.1 -> cv2.i.2 -> DFL -> dist2bbox at the candidate anchors: columns 0 .. 3 bit for bit; every other word of pred (the
    other columns of the row, the neighbouring rows) keeps the sentinel -- for no = 5, 6, 7 through the element-wise store"""
    c, r = S.case(name), _run(name)
    assert r.pred.shape == (c.n, c.A, c.no)
    _first_difference(r.pred, _expected_pred(c), f"{name}: pred [frame, anchor, column]")


@pytest.mark.parametrize("name", S.OVERFLOW_CASES)
def test_a_list_one_entry_short_raises_the_flag_and_writes_nothing(name):
    """the overflow word is 1, pred and every mid stay sentinel, and the counts are still the true totals (the engine's
    call-to-call feedback reads them)"""
    c, r = S.case(name), _run(name)
    assert c.overflows and r.overflow == 1
    assert r.n_dil == [len(e) for e in c.ref_dil] and r.n_cand == [len(e) for e in c.ref_cand]
    assert _sentinel_mask(r.pred).all()
    for m in r.mid:
        assert _sentinel_mask(m).all()
    # what the lists do hold below their capacity are reference positions, each once
    for l in range(len(c.shapes)):
        for got, want, cap in ((r.dil[l], c.ref_dil[l], c.inputs[l]["cap_dil"]), (r.cand[l], c.ref_cand[l], c.inputs[l]["cap_cand"])):
            assert len(got) == min(len(want), cap) and len(np.unique(got)) == len(got) and set(got.tolist()) <= set(want.tolist())


def test_the_same_call_twice_gives_the_same_bits():
    from cvsd_amd import ops
    for name in ("lengths", "masked"):
        c, a = S.case(name), _run(name)
        b = ops.sparse_box(c.inputs, c.best, c.conf, c.nc, no=c.no, classes=c.classes)
        np.testing.assert_array_equal(_bits(a.pred), _bits(b.pred))
        for l in range(len(c.shapes)):
            np.testing.assert_array_equal(_bits(a.mid[l]), _bits(b.mid[l]))
            np.testing.assert_array_equal(np.sort(a.dil[l]), np.sort(b.dil[l]))
            np.testing.assert_array_equal(np.sort(a.cand[l]), np.sort(b.cand[l]))
        assert (a.n_dil, a.n_cand, a.overflow) == (b.n_dil, b.n_cand, b.overflow)


@pytest.mark.parametrize("name", ["lengths", "masked"])
def test_one_frame_does_not_depend_on_the_batch(name):
    """frame 1 alone (other blocks, other list positions, other waves) has the bits it has inside the batch of 3"""
    from cvsd_amd import ops
    c, r = S.case(name), _run(name)
    levels, best = c.frame(1)
    one = ops.sparse_box(levels, best, c.conf, c.nc, no=c.no, classes=c.classes)
    assert one.overflow == 0 and sum(one.n_cand) == int(c.cand[1].sum()) > 0 and sum(one.n_dil) == int(c.dil[1].sum())
    np.testing.assert_array_equal(_bits(one.pred[0]), _bits(r.pred[1]))
    for l, (h, w, _) in enumerate(c.shapes):
        np.testing.assert_array_equal(_bits(one.mid[l][0]), _bits(r.mid[l][1]))
        in_frame = lambda e: np.sort(e[(e >= h * w) & (e < 2 * h * w)] - h * w)
        np.testing.assert_array_equal(np.sort(one.dil[l]), in_frame(r.dil[l]))
        np.testing.assert_array_equal(np.sort(one.cand[l]), in_frame(r.cand[l]))


def test_bad_shapes_come_back_as_errors_without_a_launch():
    """a cin that is no multiple of 16 and a fourth level are refused by the wrapper and, for callers that come another way, by the
    entry itself: MI355_EINVAL, every output left as it was handed in; the neighbouring good call runs"""
    import ctypes as C
    from cvsd_amd import _lib, ops
    c = S.case("tiny")
    lv = c.inputs[0]
    rng = np.random.default_rng(0)
    lv24 = dict(lv, src=rng.standard_normal((1, 1, 1, 24), dtype=np.float32), cin=24,
                wA=rng.standard_normal((64, 24, 3, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.sparse_box([lv24], c.best, c.conf, c.nc)
    with pytest.raises(ValueError, match="1 to 3 levels"):
        ops.sparse_box([lv] * 4, np.repeat(c.best, 4, axis=1), c.conf, c.nc)
    # the entry, past the wrapper
    arrs = [lv24["src"], lv24["wA"], lv["bA"], lv["wB"], lv["bB"], lv["wC"], lv["bC"]]
    mid, dil, cand, pred = ops._sentinel((1, 1, 1, 64)), np.full(1, -1, np.int32), np.full(1, -1, np.int32), ops._sentinel((1, 4, 5))
    state = (C.c_int * 12)(*[-7] * 12)
    ptrs = (C.c_void_p * 40)(*([a.ctypes.data for a in arrs + [mid, dil, cand]] * 4))
    best4 = np.ascontiguousarray(np.repeat(c.best, 4, axis=1))
    for n_levels, geom in ((1, [1, 1, 24, 0, 24, 64, 8, 64, 0, 1, 1]), (4, [1, 1, 24, 0, 16, 64, 8, 64, 0, 1, 1])):
        g = (C.c_int * 44)(*(geom * 4))
        rc = _lib.lib().mi355_op_sparse_box(0, ptrs, g, n_levels, 1, best4.ctypes.data, 0.25, None, 0, 1, 5, 1, pred.ctypes.data, state)
        assert rc == -1
        assert _sentinel_mask(pred).all() and _sentinel_mask(mid).all() and dil[0] == -1 and cand[0] == -1 and list(state) == [-7] * 12
    r = _run("tiny")
    assert r.overflow == 0 and r.n_cand == [1] and not _sentinel_mask(r.pred[0, 0, :4]).any()
