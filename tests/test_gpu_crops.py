"""Person crops on the GPU (csrc/crop_kernels.hip): every call of tests/_crop_cases.py through ``mi355_crops`` and
``ops.crop_resize`` against the host twin, byte for byte, for host and device outputs and for host frames and pitched CUDA tensors; and
``crops=`` of predict / track / track_cameras against ``ops.crop_resize(frame, crop_rects(boxes))``.  Integer arithmetic: nothing here
has a tolerance."""
import numpy as np
import pytest
import torch

import _crop_cases as K
from cvsd_amd import JPEGFrame, RenderSpec, YUVFrame, _lib, ops
from cvsd_amd.crops import CropSpec, crop_rects
from tools import synth

pytestmark = pytest.mark.gpu

CALLS = K.calls()
CALL_IDS = [c[0] for c in CALLS]
_twin = {}


def twin(call):
    """the host twin's crops of a call (tests/test_crop_cases.py holds them to the checker), made once"""
    cid, names, rects, size, fit, fill = call
    if cid not in _twin:
        _twin[cid] = K.raw_call(-1, K.flat(names), rects, size, fit, fill)
    return _twin[cid]


def _same(got, exp, what):
    assert len(got) == len(exp), what
    for k, (g, e) in enumerate(zip(got, exp)):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.shape == e.shape and np.array_equal(g, e), (what, k)


_cuda_frames = {}


def cuda_frame(name):
    """the table's frame as a pitched view of a larger CUDA tensor: rows further apart than 3 w, first byte at an odd offset"""
    if name not in _cuda_frames:
        f = K.frames()[name]
        big = torch.zeros((f.shape[0] + 2, f.shape[1] + 3, 3), dtype=torch.uint8, device="cuda:0")
        big[1:1 + f.shape[0], 2:2 + f.shape[1]] = torch.from_numpy(np.ascontiguousarray(f)).cuda()
        _cuda_frames[name] = (big, big[1:1 + f.shape[0], 2:2 + f.shape[1]])
    return _cuda_frames[name][1]


def _device_alloc(nbytes):
    t = torch.full((nbytes,), K.GUARD, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr(), lambda: t.cpu().numpy()


def _device_desc(t):
    return _lib.RenderFrame(t.data_ptr(), t.shape[0], t.shape[1], t.stride(0), 1)


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", CALLS, ids=CALL_IDS)
def test_kernel_equals_host_twin(call):
    """host frames into pitched host destinations, and pitched CUDA tensors into pitched device destinations (3 bytes off a dword, rows
    3 w + 5 apart: every row takes another alignment), guard bytes intact"""
    cid, names, rects, size, fit, fill = call
    exp = twin(call)
    _same(K.raw_call(0, K.flat(names), rects, size, fit, fill), exp, (cid, "host"))
    dev = [cuda_frame(n) for n in names]
    torch.cuda.synchronize()
    _same(K.raw_call(0, dev, rects, size, fit, fill, alloc=_device_alloc, frame_desc=_device_desc), exp, (cid, "device"))


@pytest.mark.parametrize("call", [c for c in CALLS if not c[0].startswith("same-")], ids=lambda c: c[0])
def test_ops_crop_resize(call):
    """``ops.crop_resize``: out="numpy" and out="cuda", host frames and CUDA tensors"""
    cid, names, rects, size, fit, fill = call
    exp = twin(call)
    kw = dict(size=size, fit=fit, fill=fill, device=0)
    for frames in (K.flat(names), [cuda_frame(n) for n in names]):
        got = ops.crop_resize(frames, rects, **kw)
        assert [len(g) for g in got] == [len(r) for r in rects]
        _same([c for g in got for c in g], exp, cid)
        got = ops.crop_resize(frames, rects, out="cuda", **kw)
        if size is not None:                                   # one tensor [M, h, w, 3] per frame, views into a single allocation
            assert all(isinstance(g, torch.Tensor) and g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == (len(r), *size, 3)
                       for g, r in zip(got, rects))
            live = [g for g in got if len(g)]
            assert len({g.untyped_storage().data_ptr() for g in live}) <= 1
        _same([c for g in got for c in g], exp, cid)
    for n in names:                                            # the sources were only read
        assert np.array_equal(cuda_frame(n).cpu().numpy(), K.frames()[n])


def test_single_frame_and_yuv_and_device_frame():
    f = K.frames()["37x53"]
    r = K.rects("37x53")
    one = ops.crop_resize(f, r, size=(17, 9), device=0)
    _same(one, K.raw_call(-1, [f], [r], (17, 9)), "single")
    rng = np.random.default_rng(5)
    yuv = YUVFrame(rng.integers(0, 256, (48, 64), dtype=np.uint8), uv=rng.integers(0, 256, (24, 64), dtype=np.uint8), fmt="nv12")
    bgr = yuv.to_bgr(0)
    rr = np.array([[3, 2, 40, 41], [0, 0, 64, 48], [60, 40, 64, 48]], np.int32)
    _same(ops.crop_resize(yuv, rr, size=(32, 16), fit="pad", device=0), K.raw_call(-1, [bgr], [rr], (32, 16), "pad"), "yuv")
    t = cuda_frame("37x53")
    df = ops.DeviceFrame(t.data_ptr(), 37, 53, t.stride(0))
    _same(ops.crop_resize(df, r, device=0), K.raw_call(-1, [f], [r], None), "device frame")


def test_refusals_on_the_gpu_path_leave_destinations_untouched():
    f = K.frames()["16x16"]
    bad = np.array([[1, 1, 9, 9], [0, 0, 17, 4]], np.int32)
    assert "rects[0][1]" in K.raw_call(0, [f], [bad], (4, 4), expect_rc=-1)
    assert "rects[0][1]" in K.raw_call(0, [cuda_frame("16x16")], [bad], None, expect_rc=-1, alloc=_device_alloc, frame_desc=_device_desc)
    assert "spec.height" in K.raw_call(0, [f], [bad[:1]], (0, 4), expect_rc=-1, alloc=_device_alloc)
    assert "spec.fit" in K.raw_call(0, [f], [bad[:1]], (4, 4), expect_rc=-1, fit_code=7)


# ---- crops= of the detector's entry points ------------------------------------------------------------------------------------------------
def _model(name="yolov8n-pose", **kw):
    from cvsd_amd import YOLO
    _, sd = synth.synthetic_checkpoint(name, seed=0)
    return YOLO.from_state_dict(name, sd, device=0, **kw)


@pytest.fixture(scope="module")
def pose():
    return _model()


KW = dict(conf=0.05, max_det=12, imgsz=320)
H, W = 96, 128
SPECS = [CropSpec(), CropSpec(size=(64, 32)), CropSpec(size=(32, 32), fit="pad", fill=0, square=True, gain=1.0, pad=0)]


def _same_rows(a, b):
    assert np.array_equal(a.boxes.data.numpy(), b.boxes.data.numpy()) and np.array_equal(a.keypoints.data.numpy(), b.keypoints.data.numpy())
    if a.anchor_idx is not None and b.anchor_idx is not None:
        assert np.array_equal(a.anchor_idx, b.anchor_idx)


def _expected(frame, res, spec):
    """``ops.crop_resize(frame, crop_rects(boxes))``: the crops the entry point must return for ``res``"""
    rects = crop_rects(res.boxes.xyxy.numpy(), res.orig_shape, spec.gain, spec.pad, spec.square)
    assert len(rects) == len(res)
    return ops.crop_resize(frame, rects, size=spec.size, fit=spec.fit, fill=spec.fill, device=0)


def _check(frame, plain, got, spec):
    if plain is not None:
        _same_rows(plain, got)
        assert plain.crops is None and plain.crop_jpegs is None
    assert got.crops is not None and len(got.crops) == len(got)
    _same(got.crops, _expected(frame, got, spec), "crops")


@pytest.mark.parametrize("spec", SPECS, ids=["native", "64x32", "32x32-pad-square"])
def test_predict_crops(pose, spec):
    frames = synth.synthetic_frames(2, H, W, seed=3)
    keep = frames.copy()
    plain = pose.predict(frames, **KW)
    got = pose.predict(frames, crops=spec, **KW)
    assert np.array_equal(frames, keep), "the caller's frames were written"
    assert sum(len(r) for r in got) > 0, "nothing was detected: the test would compare empty lists"
    for f, a, b in zip(frames, plain, got):
        _check(f, a, b, spec)
        assert b.rendered is None and b.jpeg is None and b.crop_jpegs is None
    again = pose.predict(frames, **KW)                          # opt-in: the call without crops= is what it was
    for a, b in zip(plain, again):
        _same_rows(a, b)
        assert b.crops is None
    as_dict = pose.predict(frames, crops=dict(size=spec.size, fit=spec.fit, fill=spec.fill, square=spec.square, gain=spec.gain, pad=spec.pad), **KW)
    for a, b in zip(got, as_dict):
        _same(b.crops, a.crops, "dict")
    if spec.size is None:
        for a, b in zip(got, pose.predict(frames, crops=True, **KW)):
            _same(b.crops, a.crops, "True")


def test_predict_crops_out_cuda_is_one_tensor_per_frame(pose):
    frames = synth.synthetic_frames(2, H, W, seed=3)
    spec = CropSpec(size=(64, 32), out="cuda")
    got = pose.predict(frames, crops=spec, **KW)
    assert sum(len(r) for r in got) > 0
    for f, r in zip(frames, got):
        assert isinstance(r.crops, torch.Tensor) and r.crops.is_cuda and tuple(r.crops.shape) == (len(r), 64, 32, 3)
        _same(list(r.crops), _expected(f, r, spec), "cuda")
        if len(r) > 1:                                          # subscripting a Results keeps the crops aligned with the boxes
            _same(list(r[1].crops), _expected(f, r, spec)[1:2], "row")
    native = pose.predict(frames, crops=CropSpec(out="cuda"), **KW)
    for f, r in zip(frames, native):
        assert all(isinstance(c, torch.Tensor) and c.is_cuda for c in r.crops)
        _same(r.crops, _expected(f, r, CropSpec()), "cuda native")


PAD = CropSpec(size=(48, 24), fit="pad")


def test_predict_crops_from_cuda_yuv_and_jpeg_frames(pose):
    """a CUDA tensor, a YUVFrame, a JPEGFrame: the crops are those of the BGR frame the call detected on"""
    spec = PAD
    a = synth.synthetic_frames(1, H, W, seed=4)[0]
    t = torch.from_numpy(np.stack([a, a[::-1].copy()])).cuda()
    keep = t.cpu().numpy().copy()
    dev = pose.predict(t, crops=spec, **KW)
    assert sum(len(r) for r in dev) > 0
    for f, p, r in zip(keep, pose.predict(t, **KW), dev):
        assert r.orig_img is None
        _check(f, p, r, spec)
    assert np.array_equal(t.cpu().numpy(), keep), "the caller's tensor was written"
    yuv = YUVFrame(np.ascontiguousarray(a[..., 1]), uv=np.random.default_rng(9).integers(96, 160, (H // 2, W), dtype=np.uint8), fmt="nv12")
    r = pose.predict(yuv, crops=spec, **KW)[0]
    assert len(r) > 0
    _check(yuv.to_bgr(0), pose.predict(yuv, **KW)[0], r, spec)
    data = ops.jpeg_encode(a, quality=95, subsampling="444", device=0)
    bgr = ops.jpeg_decode(data, device=-1)
    r = pose.predict(JPEGFrame(data), crops=spec, **KW)[0]
    assert len(r) > 0
    _check(bgr, pose.predict(bgr, **KW)[0], r, spec)


def test_predict_crops_of_a_mixed_size_list(pose):
    spec = PAD
    a, b = synth.synthetic_frames(1, H, W, seed=4)[0], synth.synthetic_frames(1, 80, 112, seed=5)[0]
    mixed = pose.predict([a, b], crops=spec, **KW)
    assert sum(len(r) for r in mixed) > 0
    for f, p, r in zip((a, b), pose.predict([a, b], **KW), mixed):
        _check(f, p, r, spec)


def test_tiled_predict_crops_in_frame_pixels(pose):
    spec = PAD
    a = synth.synthetic_frames(1, H, W, seed=4)[0]
    tiled = pose.predict(a, tile=64, crops=spec, **dict(KW, imgsz=64))[0]
    assert len(tiled) > 0 and tiled.tile_idx is not None
    _check(a, pose.predict(a, tile=64, **dict(KW, imgsz=64))[0], tiled, spec)          # rectangles in frame pixels, not tile pixels


def test_batch_invariance_and_a_frame_without_detections(pose):
    frames = synth.synthetic_frames(3, H, W, seed=7)
    spec = CropSpec(size=(40, 20))
    batch = pose.predict(frames, crops=spec, **KW)
    assert sum(len(r) for r in batch) > 0
    for f, b in zip(frames, batch):
        alone = pose.predict(f, crops=spec, **KW)[0]
        _same_rows(alone, b)
        _same(alone.crops, b.crops, "batch invariance")
    for sp in (CropSpec(), spec, CropSpec(size=(40, 20), out="cuda")):
        none = pose.predict(frames, crops=sp, **dict(KW, conf=0.9999))
        assert all(len(r) == 0 and r.crops is not None and len(r.crops) == 0 for r in none)
    some = pose.predict([frames[0], frames[1]], crops=spec, classes=[0], **KW)       # a mixed call: rows may be many in one, none in another
    for f, r in zip(frames, some):
        _check(f, None, r, spec)


def test_crops_from_the_rendered_picture(pose):
    frames = synth.synthetic_frames(2, H, W, seed=3)
    rspec = RenderSpec(anonymize="box", mosaic=8)
    spec = CropSpec(size=(64, 32), source="rendered")
    got = pose.predict(frames, render=rspec, crops=spec, **KW)
    assert sum(len(r) for r in got) > 0
    differs = False
    for f, r in zip(frames, got):
        assert r.rendered is not None and not np.array_equal(r.rendered, f)
        _same(r.crops, _expected(r.rendered, r, spec), "rendered")
        differs |= any(not np.array_equal(x, y) for x, y in zip(r.crops, _expected(f, r, spec)))
    assert differs, "the crops were cut from the source frame"
    with pytest.raises(ValueError, match="render="):
        pose.predict(frames, crops=spec, **KW)
    enc = pose.predict(frames, render=rspec, crops=spec, encode="jpeg", **KW)      # render, then crops, then encode
    for a, b in zip(got, enc):
        assert b.rendered is None and b.crops is None and b.jpeg == ops.jpeg_encode(a.rendered, device=0)
        assert b.crop_jpegs == [ops.jpeg_encode(c, device=0) for c in a.crops]


def test_crop_jpegs_and_save_crop(pose, tmp_path):
    frames = synth.synthetic_frames(2, H, W, seed=3)
    spec = CropSpec(size=(64, 32))
    got = pose.predict(frames, crops=spec, encode=dict(keep_pixels=True), **KW)
    assert sum(len(r) for r in got) > 0
    for f, r in zip(frames, got):
        _same(r.crops, _expected(f, r, spec), "keep_pixels")
        assert r.crop_jpegs == [ops.jpeg_encode(c, device=0) for c in r.crops] and r.jpeg == ops.jpeg_encode(f, device=0)
    bare = pose.predict(frames, crops=spec, encode="jpeg", **KW)
    assert all(b.crops is None and b.crop_jpegs == a.crop_jpegs for a, b in zip(got, bare))   # only the bytes came back
    on_gpu = pose.predict(frames, crops=CropSpec(size=(64, 32), out="cuda"), encode="jpeg", **KW)
    assert all(b.crops.is_cuda and b.crop_jpegs == a.crop_jpegs for a, b in zip(got, on_gpu))
    # save_crop=True: crops=True, encode="jpeg" -- native crops, their streams, and the files
    saved = pose.predict(frames, save_crop=True, **KW)
    for k, (f, r) in enumerate(zip(frames, saved)):
        native = _expected(f, r, CropSpec())
        assert r.crop_jpegs == [ops.jpeg_encode(c, device=0) if c.size else None for c in native]
        paths = r.save_crop(tmp_path / f"call{k}")
        want = [b for b in r.crop_jpegs if b is not None]
        assert len(paths) == len(want) and [open(p, "rb").read() for p in paths] == want
        assert all(p.split("/")[-2] == r.names[0] for p in paths)                   # save_dir/<class name>/im.jpg, im2.jpg, ...
        assert [p.split("/")[-1] for p in paths] == ["im.jpg", *[f"im{i}.jpg" for i in range(2, len(want) + 1)]][:len(want)]
        lazy = pose.predict(f, **KW)[0]                              # no streams: made now, from orig_img
        assert lazy.crop_jpegs is None
        lazy_paths = lazy.save_crop(tmp_path / f"lazy{k}", file_name="p")
        assert [open(p, "rb").read() for p in lazy_paths] == want
    with pytest.raises(ValueError, match="save_crop"):
        pose.predict(torch.from_numpy(frames).cuda(), **KW)[0].save_crop(tmp_path / "none")


def test_track_crops_follow_the_trackers_boxes(pose):
    clip = np.ascontiguousarray(synth.synthetic_clip(3, H, W, seed=3))
    spec = CropSpec(size=(64, 32))
    plain = [pose.track(f, persist=i > 0, **KW)[0] for i, f in enumerate(clip)]
    got = [pose.track(f, persist=i > 0, crops=spec, **KW)[0] for i, f in enumerate(clip)]
    assert any(r.boxes.is_track for r in got), "no track came back: the rows would be the detector's"
    for f, a, b in zip(clip, plain, got):
        assert np.array_equal(a.boxes.data.numpy(), b.boxes.data.numpy()) and a.crops is None
        _same(b.crops, _expected(f, b, spec), "track")


def test_track_cameras_crops(pose):
    a, b = synth.synthetic_clip(2, H, W, seed=3), synth.synthetic_clip(2, 80, 112, seed=4)
    spec = CropSpec(size=(64, 32), fit="pad")
    for t in range(2):
        fa, fb = np.ascontiguousarray(a[t]), np.ascontiguousarray(b[t])
        plain = pose.track_cameras([fa, None, fb], persist=t > 0, **KW)
        out = _model_b().track_cameras([fa, None, fb], persist=t > 0, crops=spec, **KW)
        assert out[1] is None
        for f, p, r in ((fa, plain[0], out[0]), (fb, plain[2], out[2])):
            assert np.array_equal(p.boxes.data.numpy(), r.boxes.data.numpy()) and p.crops is None
            _same(r.crops, _expected(f, r, spec), "cameras")
    assert sum(len(r) for r in (out[0], out[2])) > 0
    gated = [pose.track_cameras([fa, None, fb], persist=t > 0, crops=spec, motion_gate=True, **KW) for t in range(2)][1]
    assert gated[0].motion["skipped"] and gated[2].motion["skipped"] and gated[1] is None
    for f, r in ((fa, gated[0]), (fb, gated[2])):                # the same frames again: the carried rows, cut out of this tick's frame
        _same(r.crops, _expected(f, r, spec), "gated")
    assert sum(len(r) for r in (gated[0], gated[2])) > 0


_second = []


def _model_b():
    """a second engine with trackers of its own, so that the plain and the crops= ticks of a clip do not share tracker state"""
    if not _second:
        _second.append(_model())
    return _second[0]
