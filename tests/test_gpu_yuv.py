"""NV12 / I420 frames converted to BGR on the GPU at ingest.  The kernel against the numpy restatement of
tests/_yuv_numpy.py byte for byte, on both of its paths; then every entry point that takes YUV frames against the same entry point given
the restatement's BGR frames, bit for bit: the conversion writes the bytes the BGR path would have been handed, nothing after it changes."""
import numpy as np
import pytest
import torch

import _yuv_numpy as Y

pytestmark = pytest.mark.gpu

FMTS = ["nv12", "i420"]


# ---------------------------------------------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(Y.LAYOUT_CASES))
def test_kernel_layout_cases(name, fmt):
    frame, want = Y.layout_frame(name, fmt)
    np.testing.assert_array_equal(Y.convert_guarded([frame], device=0)[0], want)       # (the hook also checks guard bytes on the device)


@pytest.mark.parametrize("fmt", FMTS)
def test_kernel_every_triple(fmt):
    y, u, v = Y.all_triples()
    got = Y.convert_guarded([Y.make_frame(y, u, v, fmt)], device=0)[0]
    assert np.array_equal(got, Y.yuv_to_bgr(y, u, v))


def _content(h, w, seed):
    """(y, u, v) of a synthetic frame, and the BGR frame the conversion must make of them"""
    from tools import synth
    y, u, v = Y.bgr_to_yuv420(synth.synthetic_frames(1, h, w, seed=seed)[0])
    return (y, u, v), Y.yuv_to_bgr(y, u, v)


def test_kernel_mixed_call_equals_per_frame_results():
    a, wa = Y.layout_frame("2x2 minimum", "nv12")
    b, wb = Y.layout_frame("6x48 pitched vector", "i420")
    (y, u, v), wc = _content(240, 320, 4)
    c = Y.make_frame(y, u, v, "nv12")
    d, wd = Y.layout_frame("4x18 width not a multiple of 16", "i420")
    got = Y.convert_guarded([a, b, c, d], device=0)
    for g, w in zip(got, (wa, wb, wc, wd)):
        np.testing.assert_array_equal(g, w)
    for f, w in zip((a, b, c, d), (wa, wb, wc, wd)):
        np.testing.assert_array_equal(Y.convert_guarded([f], device=0)[0], w)


# ---------------------------------------------------------------------------------------------------- end to end
def _to_cuda(frame):
    """the same frame with its planes on the GPU, rows as far apart as on the host"""
    from cvsd_amd import YUVFrame

    def up(p):
        t = torch.empty((p.shape[0], p.strides[0]), dtype=torch.uint8, device="cuda")[:, :p.shape[1]]
        t.copy_(torch.from_numpy(np.ascontiguousarray(p)))
        return t
    if frame.fmt == "nv12":
        return YUVFrame(up(frame.y), uv=up(frame.uv), fmt="nv12")
    return YUVFrame(up(frame.y), u=up(frame.u), v=up(frame.v), fmt="i420")


def _assert_same_results(got, want):
    assert len(got) == len(want)
    for r, w in zip(got, want):
        assert r.orig_img is None
        assert r.orig_shape == w.orig_shape
        np.testing.assert_array_equal(r.anchor_idx, w.anchor_idx)
        np.testing.assert_array_equal(r.boxes.data.numpy(), w.boxes.data.numpy())
        if w.keypoints is not None:
            np.testing.assert_array_equal(r.keypoints.data.numpy(), w.keypoints.data.numpy())


@pytest.fixture(scope="module", params=["yolov8n", "yolov8n-pose"])
def models(request):
    from cvsd_amd import YOLO
    from tools import synth
    sd = synth.synthetic_checkpoint(request.param, seed=0)[1]
    return {"name": request.param, "model": YOLO.from_state_dict(request.param, sd), "chunk2": YOLO.from_state_dict(request.param, sd, batch_chunk=2)}


# name -> (model key, [(h, w, Y pitch or None, seed of the synthetic content)])
E2E = {
    "one 640x640": ("model", [(640, 640, None, 10)]),
    "one 240x320": ("model", [(240, 320, None, 10)]),
    "three 240x320, Y pitch 384": ("model", [(240, 320, 384, 11), (240, 320, 384, 10), (240, 320, 384, 12)]),
    "mixed 240x320 480x640 64x48": ("model", [(240, 320, None, 10), (480, 640, None, 11), (64, 48, None, 12)]),
    "five 64x64, batch_chunk 2": ("chunk2", [(64, 64, None, 10 + i) for i in range(5)]),
}
# the case whose first frame has rows at conf 0.25 under both models' random weights (yolov8n finds none in the seed-10 frames at any
# conf): the comparison of an all-empty result must not pass silently
NON_EMPTY = "three 240x320, Y pitch 384"


def _case(name, fmt):
    key, spec = E2E[name]
    frames, bgr = [], []
    for h, w, pitch, seed in spec:
        (y, u, v), want = _content(h, w, seed)
        frames.append(Y.make_frame(y, u, v, fmt, y_stride=pitch))
        bgr.append(want)
    return key, frames, bgr


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", list(E2E))
def test_predict_equals_the_bgr_call(models, name, fmt):
    key, frames, bgr = _case(name, fmt)
    model = models[key]
    want = model(bgr if len(bgr) > 1 else bgr[0], conf=0.25)
    if name == NON_EMPTY:
        assert len(want[0].boxes) > 0
    _assert_same_results(model(frames if len(frames) > 1 else frames[0], conf=0.25), want)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("name", ["three 240x320, Y pitch 384", "mixed 240x320 480x640 64x48"])
def test_predict_cuda_planes_equals_the_bgr_call(models, name, fmt):
    key, frames, bgr = _case(name, fmt)
    want = models[key](bgr, conf=0.25)
    assert sum(len(w.boxes) for w in want) > 0        # (the 480x640 frame of the mixed list, the first of the three)
    _assert_same_results(models[key].predict([_to_cuda(f) for f in frames], conf=0.25), want)


def test_predict_mixes_formats_in_one_call(models):
    _, nv12, bgr = _case("mixed 240x320 480x640 64x48", "nv12")
    _, i420, _ = _case("mixed 240x320 480x640 64x48", "i420")
    _assert_same_results(models["model"]([nv12[0], i420[1], nv12[2]], conf=0.25), models["model"](bgr, conf=0.25))


def test_infer_async_cuda_nv12(models):
    model = models["model"]
    frames, bgr = [], []
    for i in range(4):
        (y, u, v), want = _content(64, 64, 30 + i)
        frames.append(_to_cuda(Y.make_frame(y, u, v, "nv12")))
        bgr.append(want)
    out_w, out_g = model.new_device_rows(4), model.new_device_rows(4)
    model.infer_async(torch.from_numpy(np.stack(bgr)).cuda(), out_w, conf=0.05)
    model.sync()
    want = [t.cpu().numpy().copy() for t in out_w]
    model.infer_async(frames, out_g, conf=0.05)
    model.sync()
    got = [t.cpu().numpy() for t in out_g]
    total = int(want[2][0])
    assert total > 0 and int(got[2][0]) == total
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0][:total].view(np.uint32), want[0][:total].view(np.uint32))


def test_track_yuv_equals_track_bgr():
    from cvsd_amd import YOLO
    from tools import synth
    sd = synth.synthetic_checkpoint("yolov8n", seed=0)[1]
    clip = synth.synthetic_clip(4, 240, 320, seed=2)
    planes = [Y.bgr_to_yuv420(f) for f in clip]
    a, b = YOLO.from_state_dict("yolov8n", sd), YOLO.from_state_dict("yolov8n", sd)
    tracked = 0
    for y, u, v in planes:
        want = a.track(Y.yuv_to_bgr(y, u, v), persist=True)[0]
        got = b.track(Y.make_frame(y, u, v, "nv12"), persist=True)[0]
        np.testing.assert_array_equal(got.boxes.data.numpy(), want.boxes.data.numpy())
        assert (got.boxes.id is None) == (want.boxes.id is None)
        if want.boxes.id is not None:
            np.testing.assert_array_equal(got.boxes.id.numpy(), want.boxes.id.numpy())
            tracked += len(want.boxes.id)
    assert tracked > 0
