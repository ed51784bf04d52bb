"""NV12 / I420 -> BGR through the conversion's host twin, ``ops.yuv_to_bgr(..., device=-1)``: the same per-block routine the
kernel compiles, run in a host loop -- no GPU.  Expectations come from the numpy restatement in tests/_yuv_numpy.py, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import _yuv_numpy as Y

FMTS = ["nv12", "i420"]


_convert = Y.convert_guarded


@pytest.mark.parametrize("fmt", FMTS)
def test_known_answers(fmt):
    # one 2x2 block per triple, side by side: the four pixels of a block carry the triple's colour
    n = len(Y.KNOWN)
    y = np.repeat(np.array([[k[0][0] for k in Y.KNOWN]], np.uint8), 2, axis=1).repeat(2, axis=0)
    u = np.array([[k[0][1] for k in Y.KNOWN]], np.uint8)
    v = np.array([[k[0][2] for k in Y.KNOWN]], np.uint8)
    got = _convert([Y.make_frame(y, u, v, fmt)])[0]
    assert got.shape == (2, 2 * n, 3)
    for i, (_, bgr) in enumerate(Y.KNOWN):
        assert (got[:, 2 * i:2 * i + 2] == np.array(bgr, np.uint8)).all(), (Y.KNOWN[i], got[0, 2 * i])
    np.testing.assert_array_equal(got, Y.yuv_to_bgr(y, u, v))      # the restatement gives the table too


@pytest.fixture(scope="module")
def triples():
    y, u, v = Y.all_triples()
    return y, u, v, Y.yuv_to_bgr(y, u, v)


def test_all_triples_image_holds_every_triple_once():
    y, u, v = Y.all_triples()
    code = (np.repeat(np.repeat(u.astype(np.int64), 2, 0), 2, 1) << 16) | (np.repeat(np.repeat(v.astype(np.int64), 2, 0), 2, 1) << 8) | y
    assert np.array_equal(np.sort(code.ravel()), np.arange(1 << 24))


@pytest.mark.parametrize("fmt", FMTS)
def test_every_triple_equals_the_restatement(triples, fmt):
    y, u, v, want = triples
    got = _convert([Y.make_frame(y, u, v, fmt)])[0]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(Y.LAYOUT_CASES))
def test_layout_cases(name, fmt):
    frame, want = Y.layout_frame(name, fmt)
    got = _convert([frame])[0]
    np.testing.assert_array_equal(got, want)
    # constant Y: a block is one colour, and it is the colour of its own chroma sample
    h, w = frame.shape
    blocks = got.reshape(h // 2, 2, w // 2, 2, 3)
    assert (blocks == blocks[:, :1, :, :1]).all()
    if w >= 4:
        assert not np.array_equal(got[:, 0:2], got[:, 2:4])


def test_layout_cases_take_the_intended_pitches():
    f, _ = Y.layout_frame("6x48 pitched vector", "nv12")
    assert f.y.strides[0] == 64 and f.uv.strides[0] == 64 and f.y.ctypes.data % 16 == 0 and f.uv.ctypes.data % 16 == 0
    f, _ = Y.layout_frame("6x48 pitched vector", "i420")
    assert f.y.strides[0] == 64 and f.u.strides[0] == 32 and f.v.strides[0] == 32 and f.u.ctypes.data % 8 == 0
    f, _ = Y.layout_frame("4x16 Y base offset by 1", "nv12")
    assert f.y.ctypes.data % 16 == 1 and f.uv.ctypes.data % 16 == 0


@pytest.mark.parametrize("name", list(Y.LAYOUT_CASES))
def test_nv12_and_i420_of_the_same_samples_agree(name):
    a, _ = Y.layout_frame(name, "nv12")
    b, _ = Y.layout_frame(name, "i420")
    got = _convert([a, b])
    np.testing.assert_array_equal(got[0], got[1])


def test_from_packed():
    from cvsd_amd import YUVFrame
    rng = np.random.default_rng(3)
    y, u, v = rng.integers(0, 256, (8, 12), np.uint8), rng.integers(0, 256, (4, 6), np.uint8), rng.integers(0, 256, (4, 6), np.uint8)
    want = Y.yuv_to_bgr(y, u, v)
    nv12 = np.concatenate([y, np.stack([u, v], -1).reshape(4, 12)])
    i420 = np.concatenate([y, u.reshape(2, 12), v.reshape(2, 12)])
    for arr, fmt in ((nv12, "nv12"), (i420, "i420")):
        f = YUVFrame.from_packed(arr, fmt)
        assert f.shape == (8, 12)
        np.testing.assert_array_equal(f.to_bgr(-1), want)


# ---------------------------------------------------------------------------------------------------- refusals
def _raw(y, u, v, h, w, ys, uvs, fmt):
    """the C entry point on a hand-made mi355_yuv_frame; -> the error message (the call must fail before it writes anything)"""
    from cvsd_amd import _lib
    out, buf, _ = Y.guarded((max(h, 1), max(w, 1), 3))
    addr = lambda a: None if a is None else a.ctypes.data
    fr = (_lib.YuvFrame * 1)(_lib.YuvFrame(y=addr(y), u=addr(u), v=addr(v), height=h, width=w, y_stride=ys, uv_stride=uvs, format=fmt))
    ptrs = (C.c_void_p * 1)(out.ctypes.data)
    rc = _lib.lib().mi355_op_yuv_to_bgr(-1, fr, 1, ptrs)
    assert rc == -1                                                   # MI355_EINVAL
    assert (buf == 0x5C).all()
    return _lib.lib().mi355_last_error().decode()


def test_refusals_of_the_entry_point():
    p = np.zeros((8, 8), np.uint8)
    assert "width" in _raw(p, p, None, 4, 5, 8, 8, 1)
    assert "height" in _raw(p, p, None, 3, 4, 8, 8, 1)
    assert "height" in _raw(p, p, None, 0, 4, 8, 8, 1)
    assert "width" in _raw(p, p, None, 4, 0, 8, 8, 1)
    assert "width" in _raw(p, p, None, 4, -2, 8, 8, 1)
    assert "y_stride" in _raw(p, p, None, 4, 8, 6, 8, 1)
    assert "uv_stride" in _raw(p, p, None, 4, 8, 8, 6, 1)            # NV12 chroma rows are `width` bytes
    assert "uv_stride" in _raw(p, p, p, 4, 8, 8, 3, 2)               # I420: width / 2
    assert "y is null" in _raw(None, p, None, 4, 8, 8, 8, 1)
    assert "u is null" in _raw(p, None, None, 4, 8, 8, 8, 1)
    assert "v is null" in _raw(p, p, None, 4, 8, 8, 4, 2)
    assert "format" in _raw(p, p, p, 4, 8, 8, 8, 0)
    assert "format" in _raw(p, p, p, 4, 8, 8, 8, 3)


def test_refusals_of_the_python_surface():
    from cvsd_amd import YOLO, YUVFrame, ops
    y, c = np.zeros((4, 8), np.uint8), np.zeros((2, 8), np.uint8)
    with pytest.raises(ValueError, match="uv"):
        YUVFrame(y, fmt="nv12")
    with pytest.raises(ValueError, match="u:"):
        YUVFrame(y, v=c[:, :4], fmt="i420")
    with pytest.raises(ValueError, match="v:"):
        YUVFrame(y, u=c[:, :4], fmt="i420")
    with pytest.raises(ValueError, match="fmt"):
        YUVFrame(y, uv=c, fmt="yuy2")
    with pytest.raises(ValueError, match="uv"):
        YUVFrame(y, uv=c[:, :6], fmt="nv12")                          # chroma plane of the wrong shape
    with pytest.raises(ValueError, match="width"):
        ops.yuv_to_bgr([YUVFrame(np.zeros((4, 5), np.uint8), uv=np.zeros((2, 5), np.uint8))], device=-1)
    with pytest.raises(ValueError, match="height"):
        ops.yuv_to_bgr([YUVFrame(np.zeros((3, 4), np.uint8), uv=np.zeros((1, 4), np.uint8))], device=-1)
    with pytest.raises(ValueError, match="height"):
        ops.yuv_to_bgr([YUVFrame(np.zeros((0, 4), np.uint8), uv=np.zeros((0, 4), np.uint8))], device=-1)
    with pytest.raises(ValueError, match="H % 4"):
        YUVFrame.from_packed(np.zeros((9, 8), np.uint8), "i420")      # H = 6
    good = YUVFrame(y, uv=c)
    with pytest.raises(ValueError, match="source"):
        YOLO._as_batch([good, np.zeros((4, 8, 3), np.uint8)])
    with pytest.raises(ValueError, match="source"):
        YOLO._as_batch([np.zeros((4, 8, 3), np.uint8), good])
