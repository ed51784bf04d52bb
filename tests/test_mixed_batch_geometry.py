"""Host-only checks of the mixed-batch geometry (no GPU): the engine's letterbox geometry for both LetterBox modes -- auto=True (rect,
padding modulo 32: every call whose frames share one shape) and auto=False (the square imgsz x imgsz canvas of a call whose frames
differ in shape) -- against the oracle's letterbox_geometry and the constants of its scale_boxes / scale_coords."""
import ctypes as C
import random

import numpy as np
import pytest


def _oracle(h0, w0, s, auto):
    from oracle import yolo_oracle as O
    (wr, hr), top, bottom, left, right = O.letterbox_geometry(h0, w0, (s, s), auto=auto)
    hl, wl = hr + top + bottom, wr + left + right
    # utils/ops.py:scale_boxes / scale_coords against img1_shape = the letterboxed (hl, wl), as oracle/yolo_oracle.py computes them
    gain = min(hl / h0, wl / w0)
    pad_x = round((wl - w0 * gain) / 2 - 0.1)
    pad_y = round((hl - h0 * gain) / 2 - 0.1)
    kpad = ((wl - w0 * gain) / 2, (hl - h0 * gain) / 2)
    return (hl, wl, hr, wr, top, left), (gain, float(pad_x), float(pad_y), kpad[0], kpad[1]), (bottom, right)


def _engine(h0, w0, s, auto):
    from cvsd_amd import _lib
    i6 = (C.c_int * 6)()
    d5 = (C.c_double * 5)()
    _lib.check(_lib.lib().mi355_letterbox_geometry(h0, w0, s, int(auto), i6, d5))
    return tuple(i6), tuple(d5)


def _triples():
    fixed = [(240, 320, 640), (720, 1280, 640), (1080, 1920, 640), (640, 640, 640), (100, 331, 640), (7, 5, 640),
             (480, 640, 640), (1, 1, 32), (1, 4000, 640), (4000, 1, 640), (33, 17, 96), (360, 480, 320), (1280, 1280, 640),
             (159, 160, 160), (161, 160, 160), (2160, 3840, 1280)]
    rnd = random.Random(7)
    out = list(fixed)
    while len(out) < 320:
        s = 32 * rnd.randint(1, 40)
        out.append((rnd.randint(1, 2200), rnd.randint(1, 2200), s))
    return out


@pytest.mark.parametrize("auto", [True, False])
def test_geometry_matches_oracle(auto):
    odd_pads = up = down = 0
    for h0, w0, s in _triples():
        (ints, dbls, (bottom, right)) = _oracle(h0, w0, s, auto)
        gi, gd = _engine(h0, w0, s, auto)
        assert gi == ints, (h0, w0, s, auto, gi, ints)
        assert gd == dbls, (h0, w0, s, auto, gd, dbls)          # exact: the same double arithmetic
        if not auto:
            assert gi[0] == gi[1] == s                           # the square canvas
        odd_pads += bottom != gi[4] or right != gi[5]
        up += gd[0] > 1
        down += gd[0] < 1
    assert odd_pads and up and down                              # the triples cover top != bottom, upscaling and downscaling


def test_named_cases():
    """the frames of the GPU suite: 100 x 331 pads 223 / 224 rows, 7 x 5 pads 91 / 92 columns; 640 x 640 at 640 is the identity"""
    i, _ = _engine(100, 331, 640, False)
    assert i[:6] == (640, 640, 193, 640, 223, 0)
    i, _ = _engine(7, 5, 640, False)
    assert i[:6] == (640, 640, 640, 457, 0, 91)
    i, d = _engine(640, 640, 640, False)
    assert i == (640, 640, 640, 640, 0, 0) and d == (1.0, 0.0, 0.0, 0.0, 0.0)
    assert _engine(640, 640, 640, True) == (i, d)
    # the rect mode keeps its padding modulo 32: 240 x 320 -> 480 x 640, no padding
    assert _engine(240, 320, 640, True)[0] == (480, 640, 480, 640, 0, 0)
    assert _engine(240, 320, 640, False)[0] == (640, 640, 480, 640, 80, 0)


def test_bad_arguments_are_refused():
    from cvsd_amd import _lib
    i6 = (C.c_int * 6)()
    d5 = (C.c_double * 5)()
    assert _lib.lib().mi355_letterbox_geometry(0, 5, 640, 0, i6, d5) != 0
    assert _lib.lib().mi355_letterbox_geometry(5, 5, 640, 0, None, d5) != 0


def test_mixed_batch_symbols_exported():
    from cvsd_amd import _lib
    handle = _lib.lib()
    for name in ("mi355_yolo_infer_multi", "mi355_yolo_raw_head_multi", "mi355_op_letterbox_multi", "mi355_letterbox_geometry"):
        assert name in _lib.SIGNATURES
        assert getattr(handle, name) is not None


def test_mixed_list_is_a_ragged_batch_not_an_error():
    """the façade no longer refuses a list of frames of different shapes; a list of one shape keeps the stacked path"""
    from cvsd_amd import YOLO
    a = np.zeros((240, 320, 3), np.uint8)
    wide = np.zeros((720, 1400, 3), np.uint8)
    b = wide[:, 10:1290]                                         # a column slice: rows 1400*3 bytes apart
    batch, orig = YOLO._as_batch([a, b])
    assert isinstance(batch, YOLO._Ragged) and len(orig) == 2
    assert batch.shapes == [(240, 320), (720, 1280)]
    assert batch.row_strides.tolist() == [960, 4200]
    assert batch.ptrs[1] == b.ctypes.data
    same, orig = YOLO._as_batch([a, a.copy()])
    assert isinstance(same, np.ndarray) and same.shape == (2, 240, 320, 3)
