"""Evidence frames on the GPU (csrc/render_kernels.hip): the case table of tests/_render_cases.py through ``ops.render``
against the sequential numpy checker, bit for bit, and ``render=`` of predict / track / track_cameras against
``ops.render(frame, primitives(result))``.  The feature is integer arithmetic: nothing here has a tolerance."""
import numpy as np
import pytest
import torch

import _render_cases as K
import _render_numpy as R
from cvsd_amd import RenderSpec, YUVFrame, ops
from cvsd_amd.render import RECT, primitives
from tools import synth

pytestmark = pytest.mark.gpu

NAMES = sorted(K.CASES)


@pytest.fixture(scope="module")
def table():
    """every case of the table in ONE call: 40-odd frames of seven sizes, two launches"""
    pics = ops.render([K.CASES[n][0] for n in NAMES], [K.CASES[n][1] for n in NAMES], device=0)
    return dict(zip(NAMES, pics))


@pytest.mark.parametrize("name", NAMES)
def test_kernel_matches_checker(table, name):
    got, want = table[name], K.reference(name)
    bad = np.argwhere((got != want).any(axis=2))
    assert not len(bad), f"{len(bad)} pixels differ, first (y, x) = {bad[0]}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def test_single_calls_and_the_16_byte_path():
    """alone, a case takes the same bytes as in the batch; a 64 x 48 frame at a 16-byte aligned address moves as vectors, a 33 x 70 one
    by bytes, and a frame whose address is odd by bytes as well"""
    for name in ("200_on_a_tile", "33x70", "1x1", "mosaic_overlap_mixed"):
        f, p = K.CASES[name]
        assert np.array_equal(ops.render(f, p, device=0), K.reference(name)), name
    f, p = K.CASES["off_frame"]
    buf = np.zeros(f.size + 64, np.uint8)
    for shift in (0, 1, 5, 16):
        g = buf[shift:shift + f.size].reshape(f.shape)
        g[:] = f
        assert np.array_equal(ops.render(g, p, device=0), K.reference("off_frame")), shift


def test_three_sizes_in_one_call():
    names = ["33x70", "1x40", "corners"]
    got = ops.render([K.CASES[n][0] for n in names], [K.CASES[n][1] for n in names], device=0)
    assert [g.shape for g in got] == [(33, 70, 3), (1, 40, 3), (48, 64, 3)]
    for g, n in zip(got, names):
        assert np.array_equal(g, K.reference(n))


def test_pitched_cuda_view_is_read_in_place_and_left_unchanged():
    big = torch.from_numpy(K.frame(40, 100)).cuda()
    keep = big.cpu().numpy().copy()
    view = big[3:36, 7:77]                                        # 33 x 70, rows 300 bytes apart, first byte at offset 921
    p = K.CASES["33x70"][1]
    want = R.render(keep[3:36, 7:77], p)
    assert np.array_equal(ops.render(view, p, device=0), want)
    assert np.array_equal(big.cpu().numpy(), keep), "the source tensor was written"
    out = ops.render(view, p, device=0, out="cuda")
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(big.cpu().numpy(), keep)
    wide = torch.from_numpy(K.frame(48, 128)).cuda()              # a 16-byte aligned pitched view: the vector path on a caller's tensor
    assert np.array_equal(ops.render(wide[:, 32:96], K.CASES["off_frame"][1], device=0), R.render(wide.cpu().numpy()[:, 32:96], K.CASES["off_frame"][1]))


def test_out_cuda_for_a_list():
    names = ["label", "mosaic_edge_8"]
    outs = ops.render([K.CASES[n][0] for n in names], [K.CASES[n][1] for n in names], device=0, out="cuda")
    for o, n in zip(outs, names):
        assert o.is_cuda and np.array_equal(o.cpu().numpy(), K.reference(n))


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_yuv_sources_render_from_their_converted_frame(fmt):
    rng = np.random.default_rng(5)
    y = rng.integers(0, 256, (48, 64), dtype=np.uint8)
    if fmt == "nv12":
        f = YUVFrame(y, uv=rng.integers(0, 256, (24, 64), dtype=np.uint8), fmt="nv12")
    else:
        f = YUVFrame(y, u=rng.integers(0, 256, (24, 32), dtype=np.uint8), v=rng.integers(0, 256, (24, 32), dtype=np.uint8), fmt="i420")
    p = K.CASES["mosaic_under_line"][1]
    bgr = f.to_bgr(0)
    got = ops.render(f, p, device=0)
    assert np.array_equal(got, ops.render(bgr, p, device=0)) and np.array_equal(got, R.render(bgr, p))
    assert not np.array_equal(got, bgr)


def test_limit_plus_one_on_the_gpu_path():
    f = K.frame(48, 64)
    p = np.tile(K.P((K.DISC, 5, 5, 0, 0, 2, 0xFFFFFF)), (16385, 1))
    with pytest.raises(ValueError, match="16384"):
        ops.render(f, p, device=0)
    assert np.array_equal(ops.render(f, p[:-1], device=0), R.render(f, p[:1]))       # the limit itself: 512 mask words, two rounds of 256


# ---- render= of the detector's entry points ------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("hw,imgsz", [((64, 64), 64), ((240, 320), 320)])
def test_predict_render(pose, hw, imgsz):
    frames = synth.synthetic_frames(2, hw[0], hw[1], seed=3)
    keep = frames.copy()
    plain = pose.predict(frames, imgsz=imgsz, **KW)
    drawn = pose.predict(frames, imgsz=imgsz, render=True, **KW)
    assert np.array_equal(frames, keep), "the caller's frames were written"
    assert sum(len(r) for r in drawn) > 0, "nothing was detected: the test would compare copies"
    for f, a, b in zip(frames, plain, drawn):
        _same_rows(a, b)
        assert a.rendered is None and b.rendered.shape == f.shape and b.rendered.dtype == np.uint8
        p = primitives(b, RenderSpec())
        assert np.array_equal(b.rendered, ops.render(f, p, device=0))
        assert np.array_equal(b.rendered, R.render(f, p))
        assert np.array_equal(b.plot(), b.rendered) and np.array_equal(b.orig_img, f)
    spec = RenderSpec(anonymize="head", mosaic=8, color_by="class", labels=False)
    anon = pose.predict(frames, imgsz=imgsz, render=spec, **KW)
    for f, a, b in zip(frames, plain, anon):
        _same_rows(a, b)
        assert np.array_equal(b.rendered, R.render(f, primitives(b, spec)))
        assert np.array_equal(b.plot(anonymize="head", mosaic=8, color_by="class", labels=False), b.rendered)
    assert np.array_equal(frames, keep)


def test_predict_render_mixed_shapes(pose):
    a, b = synth.synthetic_frames(1, 240, 320, seed=4)[0], synth.synthetic_frames(1, 200, 300, seed=5)[0]
    plain = pose.predict([a, b], imgsz=320, **KW)
    drawn = pose.predict([a, b], imgsz=320, render=True, **KW)
    assert sum(len(r) for r in drawn) > 0
    for f, x, y in zip((a, b), plain, drawn):
        _same_rows(x, y)
        assert np.array_equal(y.rendered, ops.render(f, primitives(y), device=0))


def test_predict_render_from_cuda_frames(pose):
    a = synth.synthetic_frames(1, 240, 320, seed=4)[0]
    t = torch.from_numpy(np.stack([a, a[::-1].copy()])).cuda()                # frames on the GPU: no host image, the picture comes from the tensor
    keep = t.cpu().numpy().copy()
    dev = pose.predict(t, imgsz=320, render=True, **KW)
    assert sum(len(r) for r in dev) > 0
    for f, r in zip(keep, dev):
        assert r.orig_img is None and np.array_equal(r.rendered, ops.render(f, primitives(r), device=0))
        with pytest.raises(ValueError, match="render="):
            r.plot()
    assert np.array_equal(t.cpu().numpy(), keep), "the caller's tensor was written"


def test_predict_render_from_a_yuv_frame(pose):
    a = synth.synthetic_frames(1, 240, 320, seed=4)[0]
    yuv = YUVFrame(np.ascontiguousarray(a[..., 1]), uv=np.random.default_rng(9).integers(96, 160, (120, 320), dtype=np.uint8), fmt="nv12")
    r = pose.predict(yuv, imgsz=320, render=True, **KW)[0]
    _same_rows(pose.predict(yuv, imgsz=320, **KW)[0], r)
    assert len(r) > 0 and np.array_equal(r.rendered, ops.render(yuv.to_bgr(0), primitives(r), device=0))


def test_track_render_draws_ids(pose):
    clip = np.ascontiguousarray(synth.synthetic_clip(3, 240, 320, seed=3))
    plain = [pose.track(f, persist=i > 0, imgsz=320, **KW)[0] for i, f in enumerate(clip)]
    drawn = [pose.track(f, persist=i > 0, imgsz=320, render=True, **KW)[0] for i, f in enumerate(clip)]
    assert any(r.boxes.is_track for r in drawn), "no track came back: no id would be drawn"
    for f, a, b in zip(clip, plain, drawn):
        assert np.array_equal(a.boxes.data.numpy(), b.boxes.data.numpy()) and a.rendered is None
        p = primitives(b)
        assert np.array_equal(b.rendered, ops.render(f, p, device=0))
        if b.boxes.is_track:                                                   # "#id conf": the label starts with the '#' glyph
            assert ord("#") in p[p[:, 0] == 6][:, 3]


def test_track_cameras_render(pose):
    a, b = synth.synthetic_clip(2, 240, 320, seed=3), synth.synthetic_clip(2, 200, 300, seed=4)
    for t in range(2):
        fa, fb = np.ascontiguousarray(a[t]), np.ascontiguousarray(b[t])
        out = pose.track_cameras([fa, None, fb], persist=t > 0, imgsz=320, render=True, **KW)
        assert out[1] is None
        for f, r in ((fa, out[0]), (fb, out[2])):
            assert np.array_equal(r.rendered, ops.render(f, primitives(r), device=0))
    assert sum(len(r) for r in (out[0], out[2])) > 0
    with pytest.raises(TypeError):
        pose.track_cameras([fa, None, fb], rendr=True)
    gated = [pose.track_cameras([fa, None, fb], persist=t > 0, imgsz=320, render=True, motion_gate=True, **KW) for t in range(2)][1]
    assert gated[0].motion["skipped"] and gated[2].motion["skipped"]           # the same frames again: drawn with the rows the trackers stepped on
    for f, r in ((fa, gated[0]), (fb, gated[2])):
        assert np.array_equal(r.rendered, ops.render(f, primitives(r), device=0))


def test_tiled_predict_render_draws_merged_rows_in_frame_pixels(pose):
    f = synth.synthetic_frames(1, 480, 640, seed=6)[0]
    plain = pose.predict(f, imgsz=320, tile=320, **KW)[0]
    r = pose.predict(f, imgsz=320, tile=320, render=True, **KW)[0]
    assert np.array_equal(plain.boxes.data.numpy(), r.boxes.data.numpy()) and len(r) > 0
    p = primitives(r)
    assert np.array_equal(r.rendered, ops.render(f, p, device=0)) and r.rendered.shape == (480, 640, 3)
    boxes = p[p[:, 0] == RECT]
    assert np.array_equal(boxes[:, 1:5], np.floor(r.boxes.xyxy.numpy().astype(np.float64) + 0.5).astype(np.int32))   # frame pixels, not tile pixels


def test_two_engines_give_identical_pictures(pose):
    frames = synth.synthetic_frames(2, 240, 320, seed=8)
    spec = RenderSpec(anonymize="box", mosaic=4)
    one = pose.predict(frames, imgsz=320, render=spec, **KW)
    two = _model().predict(frames, imgsz=320, render=spec, **KW)
    for x, y in zip(one, two):
        assert np.array_equal(x.rendered, y.rendered) and not np.array_equal(x.rendered, x.orig_img)


def test_frames_of_overwritten_chunks_are_uploaded_again():
    """the staging area holds two chunks: of a three-chunk host call the first chunk's frame has left the GPU (mi355_yolo_last_frames
    says so) and ``render=`` passes the frames again; the pictures are what they are when every copy is still there"""
    import ctypes as C
    from cvsd_amd import _lib
    m = _model(batch_chunk=1)
    frames = synth.synthetic_frames(3, 64, 64, seed=3)
    for n, alive in ((2, [True, True]), (3, [False, True, True])):
        res = m.predict(frames[:n], imgsz=64, render=True, **KW)
        cnt = C.c_int()
        last = (_lib.RenderFrame * 3)()
        _lib.check(_lib.lib().mi355_yolo_last_frames(m._last_handle, last, 3, C.byref(cnt)))
        assert cnt.value == n and [bool(last[i].data) for i in range(n)] == alive
        assert all((last[i].height, last[i].width, last[i].row_stride) == (64, 64, 192) for i in range(n))
        for f, r in zip(frames, res):
            assert np.array_equal(r.rendered, ops.render(f, primitives(r), device=0))
    assert sum(len(r) for r in res) > 0
    with pytest.raises(LookupError):
        ops.render(None, [None] * 3, device=0, handle=m._last_handle)
