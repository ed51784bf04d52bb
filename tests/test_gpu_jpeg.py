"""JPEG evidence frames on the GPU (csrc/jpeg_kernels.hip): the case table of tests/_jpeg_cases.py through
``ops.jpeg_encode`` against the host twin, byte for byte (the host twin is checked against the sequential checker, Pillow and a float64
DCT in tests/test_jpeg_cases.py), and ``encode=`` of predict / track / track_cameras against ``ops.jpeg_encode(ops.render(...))``.  The
feature is integer arithmetic: nothing here has a tolerance."""
import ctypes as C
import io

import numpy as np
import pytest
import torch
from PIL import Image

import _jpeg_cases as K
from cvsd_amd import JpegSpec, RenderSpec, YUVFrame, _lib, ops
from cvsd_amd.render import primitives
from tools import synth

pytestmark = pytest.mark.gpu

INPUTS = K.inputs()
COMBOS = [(ss, q) for ss in K.SUBSAMPLINGS for q in K.QUALITIES]


@pytest.fixture(scope="module")
def table():
    """every input of the table in ONE call per quality and subsampling: fifteen frames of twelve sizes, three launches; the outputs lie
    between guard bytes"""
    lib = _lib.lib()
    out = {}
    for ss, q in COMBOS:
        ssv = int(ss)
        fr = (_lib.RenderFrame * len(INPUTS))()
        od = (_lib.JpegOut * len(INPUTS))()
        keep, bufs = [], []
        for i, (_, f, _) in enumerate(INPUTS):
            g = f if f.strides[2] == 1 and f.strides[1] == 3 else np.ascontiguousarray(f)
            keep.append(g)
            fr[i] = _lib.RenderFrame(g.ctypes.data, g.shape[0], g.shape[1], g.strides[0], 0)
            cap = int(lib.mi355_jpeg_bound(g.shape[0], g.shape[1], ssv))
            b = np.full(cap + 64, 0x5A, np.uint8)
            bufs.append(b)
            od[i] = _lib.JpegOut(b.ctypes.data + 32, cap, -1)
        _lib.check(lib.mi355_jpeg_encode(0, fr, len(INPUTS), q, ssv, od, None, None))
        for i, (name, _, _) in enumerate(INPUTS):
            n = int(od[i].length)
            out[(name, ss, q)] = (bytes(bufs[i][32:32 + n]), bool((bufs[i][:32] == 0x5A).all() and (bufs[i][32 + n:] == 0x5A).all()))
    return out


@pytest.mark.parametrize("ss,q", COMBOS)
def test_kernels_match_host_twin(table, ss, q):
    want = ops.jpeg_encode([f for _, f, _ in INPUTS], quality=q, subsampling=ss, device=-1)
    for (name, _, _), w in zip(INPUTS, want):
        got, guards = table[(name, ss, q)]
        assert guards, f"{name}: bytes outside the reported length were written"
        assert len(got) == len(w), (name, len(got), len(w))
        bad = [i for i in range(len(w)) if got[i] != w[i]]
        assert not bad, f"{name}: {len(bad)} bytes differ, first at {bad[0]} of {len(w)}"


@pytest.mark.parametrize("ss", K.SUBSAMPLINGS)
def test_coefficients_match_host(ss):
    frames = [f for _, f, _ in INPUTS]
    for q in (1, 85, 100):
        got = ops.jpeg_coefficients(frames, quality=q, subsampling=ss, device=0)
        want = ops.jpeg_coefficients(frames, quality=q, subsampling=ss, device=-1)
        for (name, _, _), g, w in zip(INPUTS, got, want):
            assert g.shape == w.shape and g.dtype == np.int16 and np.array_equal(g, w), (name, q)


def test_more_blocks_than_one_chunk_and_single_calls():
    """a 40 x 1500 frame has 282 blocks (4:2:0) / 564 (4:4:4) per MCU row: more than the 256 a segment's block takes at a time, so the
    bit offset, the DC predictors and the shared word cross a chunk boundary; alone, a case takes the bytes it takes in the batch"""
    rng = np.random.default_rng(12)
    wide = rng.integers(0, 256, (40, 1500, 3), dtype=np.uint8)
    wide[:, 300:900] = wide[:, 300:900] // 32 + 100                     # a calm stretch: short blocks beside long ones
    for ss in K.SUBSAMPLINGS:
        for q in (30, 100):
            assert ops.jpeg_encode(wide, quality=q, subsampling=ss, device=0) == ops.jpeg_encode(wide, quality=q, subsampling=ss, device=-1), (ss, q)
    for name, f, _ in INPUTS[:4]:
        assert ops.jpeg_encode(f, device=0) == ops.jpeg_encode(f, device=-1), name
    im = Image.open(io.BytesIO(ops.jpeg_encode(wide, device=0)))
    im.load()
    assert im.size == (1500, 40)


def test_pitched_cuda_view_yuv_and_mixed_sizes():
    big = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (40, 100, 3), dtype=np.uint8)).cuda()
    keep = big.cpu().numpy().copy()
    view = big[3:36, 7:77]                                        # 33 x 70, rows 300 bytes apart, first byte at offset 921
    rng = np.random.default_rng(5)
    yuv = YUVFrame(rng.integers(0, 256, (48, 64), dtype=np.uint8), uv=rng.integers(0, 256, (24, 64), dtype=np.uint8), fmt="nv12")
    small = INPUTS[0][1]
    got = ops.jpeg_encode([view, yuv, small, keep], quality=60, subsampling="444", device=0)
    assert np.array_equal(big.cpu().numpy(), keep), "the source tensor was written"
    want = ops.jpeg_encode([np.ascontiguousarray(keep[3:36, 7:77]), yuv.to_bgr(0), small, keep], quality=60, subsampling="444", device=-1)
    assert got == want
    assert ops.jpeg_encode(view, quality=60, subsampling="444", device=0) == want[0] and ops.jpeg_encode(yuv, device=0) == ops.jpeg_encode(yuv.to_bgr(0), device=-1)


def test_bad_arguments_on_the_gpu_path():
    f = INPUTS[4][1]
    for kw in (dict(quality=0), dict(quality=101), dict(subsampling="422")):
        with pytest.raises(ValueError):
            ops.jpeg_encode(f, device=0, **kw)
    with pytest.raises(ValueError):
        ops.jpeg_encode(torch.zeros((4, 4, 3), dtype=torch.uint8).cuda(), device=-1)


# ---- encode= of the detector's entry points -------------------------------------------------------------------------------------------
def _model(name="yolov8n-pose", **kw):
    from cvsd_amd import YOLO
    _, sd = synth.synthetic_checkpoint(name, seed=0)
    return YOLO.from_state_dict(name, sd, device=0, **kw)


@pytest.fixture(scope="module")
def pose():
    return _model()


KW = dict(conf=0.05, max_det=12)


def _same_rows(a, b):
    assert np.array_equal(a.boxes.data.numpy(), b.boxes.data.numpy()) and np.array_equal(a.anchor_idx, b.anchor_idx)
    assert np.array_equal(a.keypoints.data.numpy(), b.keypoints.data.numpy())


def test_predict_render_encode(pose, tmp_path):
    frames = synth.synthetic_frames(2, 240, 320, seed=3)
    keep = frames.copy()
    plain = pose.predict(frames, imgsz=320, **KW)
    drawn = pose.predict(frames, imgsz=320, render=True, **KW)
    both = pose.predict(frames, imgsz=320, render=True, encode="jpeg", **KW)
    kept = pose.predict(frames, imgsz=320, render=True, encode=JpegSpec(quality=60, subsampling="444", keep_pixels=True), **KW)
    assert np.array_equal(frames, keep) and sum(len(r) for r in both) > 0
    for f, a, d, b, k in zip(frames, plain, drawn, both, kept):
        _same_rows(a, b)
        _same_rows(a, k)
        assert a.jpeg is None and d.jpeg is None and b.rendered is None
        pic = ops.render(f, primitives(b, RenderSpec()), device=0)
        assert np.array_equal(pic, d.rendered) and np.array_equal(k.rendered, d.rendered)
        assert b.jpeg == ops.jpeg_encode(pic, device=0) == ops.jpeg_encode(pic, device=-1)
        assert k.jpeg == ops.jpeg_encode(pic, quality=60, subsampling="444", device=-1)
        im = Image.open(b.save(tmp_path / "evidence.jpg"))
        assert im.size == (320, 240)
    with pytest.raises(ValueError, match="encode="):
        plain[0].save(tmp_path / "none.jpg")
    with pytest.raises(TypeError):
        pose.predict(frames, imgsz=320, encode="png", **KW)


def test_predict_encode_alone_encodes_the_source(pose):
    a, b = synth.synthetic_frames(1, 240, 320, seed=4)[0], synth.synthetic_frames(1, 200, 300, seed=5)[0]
    plain = pose.predict([a, b], imgsz=320, **KW)
    enc = pose.predict([a, b], imgsz=320, encode={"quality": 40}, **KW)
    for f, x, y in zip((a, b), plain, enc):
        _same_rows(x, y)
        assert y.rendered is None and y.jpeg == ops.jpeg_encode(f, quality=40, device=-1)
    t = torch.from_numpy(np.stack([a, a[::-1].copy()])).cuda()                # frames on the GPU: read where they are
    dev = pose.predict(t, imgsz=320, encode="jpeg", **KW)
    for f, r in zip(t.cpu().numpy(), dev):
        assert r.jpeg == ops.jpeg_encode(f, device=-1)
    yuv = YUVFrame(np.ascontiguousarray(a[..., 1]), uv=np.random.default_rng(9).integers(96, 160, (120, 320), dtype=np.uint8), fmt="nv12")
    assert pose.predict(yuv, imgsz=320, encode="jpeg", **KW)[0].jpeg == ops.jpeg_encode(yuv.to_bgr(0), device=-1)


def test_track_and_track_cameras_encode(pose):
    clip = np.ascontiguousarray(synth.synthetic_clip(3, 240, 320, seed=3))
    plain = [pose.track(f, persist=i > 0, imgsz=320, **KW)[0] for i, f in enumerate(clip)]
    both = [pose.track(f, persist=i > 0, imgsz=320, render=True, encode="jpeg", **KW)[0] for i, f in enumerate(clip)]
    alone = [pose.track(f, persist=i > 0, imgsz=320, encode="jpeg", **KW)[0] for i, f in enumerate(clip)]
    assert any(r.boxes.is_track for r in both)
    for f, a, b, c in zip(clip, plain, both, alone):
        assert np.array_equal(a.boxes.data.numpy(), b.boxes.data.numpy()) and np.array_equal(a.boxes.data.numpy(), c.boxes.data.numpy())
        assert a.jpeg is None and b.rendered is None and c.rendered is None
        assert b.jpeg == ops.jpeg_encode(ops.render(f, primitives(b), device=0), device=-1)
        assert c.jpeg == ops.jpeg_encode(f, device=-1)
    x, y = synth.synthetic_clip(2, 240, 320, seed=3), synth.synthetic_clip(2, 200, 300, seed=4)
    for t in range(2):
        fa, fb = np.ascontiguousarray(x[t]), np.ascontiguousarray(y[t])
        ref = pose.track_cameras([fa, None, fb], persist=t > 0, imgsz=320, render=True, **KW)
    for t in range(2):
        fa, fb = np.ascontiguousarray(x[t]), np.ascontiguousarray(y[t])
        out = pose.track_cameras([fa, None, fb], persist=t > 0, imgsz=320, render=True, encode=JpegSpec(keep_pixels=True), **KW)
        assert out[1] is None
        for f, r in ((fa, out[0]), (fb, out[2])):
            pic = ops.render(f, primitives(r), device=0)
            assert np.array_equal(r.rendered, pic) and r.jpeg == ops.jpeg_encode(pic, device=-1)
    src = pose.track_cameras([fa, None, fb], persist=False, imgsz=320, encode="jpeg", **KW)
    assert src[1] is None
    for f, s in ((fa, src[0]), (fb, src[2])):
        assert s.rendered is None and s.jpeg == ops.jpeg_encode(f, device=-1)
    for r, o in ((ref[0], out[0]), (ref[2], out[2])):
        assert np.array_equal(r.boxes.data.numpy(), o.boxes.data.numpy()) and np.array_equal(r.rendered, o.rendered)
    with pytest.raises(TypeError):
        pose.track_cameras([fa, None, fb], encod="jpeg")


def test_two_engines_side_by_side(pose):
    frames = synth.synthetic_frames(2, 240, 320, seed=8)
    other = _model()
    one = pose.predict(frames, imgsz=320, render=True, encode="jpeg", **KW)
    two = other.predict(frames[::-1].copy(), imgsz=320, render=True, encode="jpeg", **KW)
    again = pose.predict(frames, imgsz=320, render=True, encode="jpeg", **KW)
    for x, y, z in zip(one, two[::-1], again):
        assert x.jpeg == y.jpeg == z.jpeg and x.jpeg[:2] == b"\xff\xd8"
    with pytest.raises(LookupError):
        ops.jpeg_encode(None, device=0, handle=_model()._h)
