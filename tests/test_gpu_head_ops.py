"""The head decode kernel, the four SPPF pool kernels and the 2x upsample kernel, each alone through the C ABI
(cvsd_amd.ops.decode / sppf_pools / upsample2x) against an independent reference -- at the branches that the whole-network tests
on random-weight checkpoints never visit.  Every comparison is equality: decode against the canonical-order oracle
(oracle/det_oracle.c:det_decode_level) bit for bit, max-pools against torch by value, the upsample word for word.

Inputs, case lists and references: tests/_head_ops_cases.py (checked on the CPU by tests/test_head_ops_cases.py).  All inputs
are free of NaN: NaN semantics of decode and pooling are out of scope."""
import numpy as np
import pytest

import _head_ops_cases as H

pytestmark = pytest.mark.gpu

DECODE_IDS = [f"nc{nc}-off{off}-k{nkpt}x{kdim}" for nc, off, (nkpt, kdim) in H.DECODE_CASES]
DECODE_PARAMS = [(nc, off, nkpt, kdim, tiny) for nc, off, (nkpt, kdim) in H.DECODE_CASES for tiny in (False, True)]
DECODE_PARAM_IDS = [f"{i}{'-1x1' if tiny else ''}" for i in DECODE_IDS for tiny in (False, True)]
decode_cases = pytest.mark.parametrize("nc,cls_off,nkpt,kdim,tiny", DECODE_PARAMS, ids=DECODE_PARAM_IDS)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same_bits(got, want):
    """equal as values first (readable report), then as bit patterns (-0 / +0, NaN payloads)"""
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_bits(got), _bits(want))


def _is_sentinel(a):
    from cvsd_amd import ops
    return _bits(a) == ops.SENTINEL_BITS


def _check_nms_form(case, pred, best, box_written=True):
    """what predict()'s decode leaves: box, keypoints and best as the reference has them; a class column is untouched or right"""
    nc = case.nc
    if box_written:
        _assert_same_bits(pred[:, :, :4], case.ref_pred[:, :, :4])
    else:
        assert _is_sentinel(pred[:, :, :4]).all()
    _assert_same_bits(pred[:, :, 4 + nc:], case.ref_pred[:, :, 4 + nc:])
    _assert_same_bits(best, case.ref_best)
    sc = pred[:, :, 4:4 + nc]
    assert (_is_sentinel(sc) | (_bits(sc) == _bits(case.ref_pred[:, :, 4:4 + nc]))).all()


@decode_cases
def test_decode_full_is_the_oracle_bit_for_bit(nc, cls_off, nkpt, kdim, tiny):
    """FULL = true (the raw-head form): every word of pred and best.  Finite logits only."""
    from cvsd_amd import ops
    case = H.decode_case(nc, cls_off, nkpt, kdim, tiny)
    pred, best = ops.decode(case.levels, nc, nkpt, kdim, mode="full")
    assert pred.shape == case.ref_pred.shape and best.shape == case.ref_best.shape
    _assert_same_bits(pred, case.ref_pred)
    _assert_same_bits(best, case.ref_best)


@decode_cases
def test_decode_nms_form_keeps_max_score_and_first_argmax(nc, cls_off, nkpt, kdim, tiny):
    """FULL = false, the launch predict() makes: the sigmoid is evaluated inside the logit window only, and (max score, FIRST
    argmax) must still be the reference's -- on exact ties in every quad placement, saturated, underflowed and seam rows."""
    from cvsd_amd import ops
    case = H.decode_case(nc, cls_off, nkpt, kdim, tiny)
    pred, best = ops.decode(case.levels, nc, nkpt, kdim, mode="nms")
    _check_nms_form(case, pred, best)


@decode_cases
def test_decode_split_form_with_open_and_closed_gate(nc, cls_off, nkpt, kdim, tiny):
    """PART 1 then gated PART 2 (the sparse box branch's dense fall-back): gate 1 = the nms form and one counted launch;
    gate 0 = the box stage returns at once: box columns untouched, nothing counted."""
    from cvsd_amd import ops
    case = H.decode_case(nc, cls_off, nkpt, kdim, tiny)
    pred, best, count = ops.decode(case.levels, nc, nkpt, kdim, mode="split", gate=1)
    _check_nms_form(case, pred, best)
    assert count == 1
    pred0, best0, count0 = ops.decode(case.levels, nc, nkpt, kdim, mode="split", gate=0)
    _check_nms_form(case, pred0, best0, box_written=False)
    assert count0 == 0


@pytest.mark.parametrize("mode", ["full", "nms"])
@pytest.mark.parametrize("nc,cls_off,nkpt,kdim", [(nc, off, nkpt, kdim) for nc, off, (nkpt, kdim) in H.DECODE_CASES], ids=DECODE_IDS)
def test_decode_of_one_frame_does_not_depend_on_the_batch(nc, cls_off, nkpt, kdim, mode):
    """frame 1 decoded alone (51 anchors: other blocks, other dead quads) has the bits it has inside the batch of 3"""
    from cvsd_amd import ops
    case = H.decode_case(nc, cls_off, nkpt, kdim)
    pred, best = ops.decode(case.levels, nc, nkpt, kdim, mode=mode)
    pred1, best1 = ops.decode(case.frame(1), nc, nkpt, kdim, mode=mode)
    np.testing.assert_array_equal(_bits(pred1[0]), _bits(pred[1]))
    np.testing.assert_array_equal(_bits(best1[0]), _bits(best[1]))
    _assert_same_bits(best1[0], case.ref_best[1])


def test_decode_alignment_errors_come_back_as_library_errors():
    """the launcher's own rules (cs and box_off multiples of 4) surface as the library's error with the launcher's message"""
    from cvsd_amd import _lib, ops
    buf = np.zeros((1, 2, 2, 76), np.float32)
    with pytest.raises(_lib.Mi355Error, match="16-byte aligned"):
        ops.decode([(buf, 2, 68, 0, 8)], nc=4)
    with pytest.raises(_lib.Mi355Error, match="16-byte aligned"):
        ops.decode([(buf[..., :74], 0, 64, 0, 8)], nc=4, mode="nms")
    pred, best = ops.decode([(buf, 4, 68, 0, 8)], nc=4)            # and the aligned neighbour runs
    assert not _is_sentinel(pred).any() and not _is_sentinel(best).any()


# -------------------------------------------------------------------------------------------------------------- SPPF pools
@pytest.mark.parametrize("n,h,w,c,half,branch", H.SPPF_CASES,
                         ids=[f"{'f16' if hf else 'f32'}-{n}x{h}x{w}x{c}-{'-'.join(map(str, b))}" for n, h, w, c, hf, b in H.SPPF_CASES])
def test_sppf_pools_equal_three_chained_torch_max_pools(n, h, w, c, half, branch):
    """x1 | x2 | x3 by value (max is exact) on a channel view; inputs are N(-3, 1) with -inf, huge and subnormal entries, so a pool
    padded with 0, a window one too wide or narrow, or a flushed subnormal shows.  The channels of y outside the view keep their bits."""
    from cvsd_amd import ops
    cx, x_off, cy, y_off = H.sppf_view(c, half)
    x = H.sppf_input(n, h, w, cx, half, seed=n * 1000 + h * w + c)
    rng = np.random.default_rng(c)
    y = np.resize(rng.standard_normal(4099, dtype=np.float32).astype(np.float16 if half else np.float32).astype(np.float32), (n, h, w, cy))
    y[..., y_off:y_off + 3 * c] = ops.SENTINEL
    got = ops.sppf_pools(x, c, x_off=x_off, y=y, y_off=y_off, half=half)
    assert got.shape == y.shape and got.dtype == np.float32
    ref = H.sppf_reference(x[..., x_off:x_off + c])
    np.testing.assert_array_equal(got[..., y_off:y_off + 3 * c], ref)
    _assert_same_bits(got[..., :y_off], y[..., :y_off])
    _assert_same_bits(got[..., y_off + 3 * c:], y[..., y_off + 3 * c:])


def test_sppf_pools_default_output_and_zero_offsets():
    """y = None: a [n, h, w, 3c] tensor, every word written; x_off = 0 on a tensor that is exactly the view"""
    from cvsd_amd import ops
    for half in (False, True):
        x = H.sppf_input(2, 7, 6, 16, half, seed=9)
        got = ops.sppf_pools(x, 16, half=half)
        np.testing.assert_array_equal(got, H.sppf_reference(x))


# ---------------------------------------------------------------------------------------------------------------- upsample
@pytest.mark.parametrize("n,h,w,c", H.UPSAMPLE_CASES)
def test_upsample2x_moves_raw_words(n, h, w, c):
    """np.repeat on both axes, as uint32: random bit patterns (NaN payloads, fp16 pairs) survive; whole vectors and scalar tails
    (c = 6, 51); the words of y around the view keep their bits"""
    from cvsd_amd import ops
    cx, x_off, cy, y_off = H.upsample_view(c)
    x = H.upsample_input((n, h, w, cx), seed=c + h)
    y = H.upsample_input((n, 2 * h, 2 * w, cy), seed=c + h + 1)
    got = ops.upsample2x(x, c, x_off=x_off, y=y, y_off=y_off)
    assert got.dtype == np.uint32
    np.testing.assert_array_equal(got, H.upsample_reference(x, c, x_off, y, y_off))
    # the same words handed over as fp32 (the engine's own view of them) come back with the same bits
    got_f = ops.upsample2x(x.view(np.float32), c, x_off=x_off, y=y.view(np.float32), y_off=y_off)
    np.testing.assert_array_equal(got_f, got)


def test_upsample2x_default_output():
    from cvsd_amd import ops
    x = H.upsample_input((2, 3, 2, 8), seed=4)
    got = ops.upsample2x(x, 8)
    assert got.shape == (2, 6, 4, 8) and not (got == ops.SENTINEL_BITS).any()
    np.testing.assert_array_equal(got, np.repeat(np.repeat(x, 2, axis=1), 2, axis=2))
