"""Frames of different sizes in one predict call (several cameras): every frame is letterboxed to the square imgsz x imgsz canvas
(Ultralytics' LetterBox auto=False for a batch whose shapes differ), the net runs once, and every frame's rows are scaled back against
its own shape.  Checked bit for bit against the canonical-order oracle composed per frame."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(240, 320), (720, 1280), (1080, 1920), (640, 640), (100, 331), (7, 5)]
S = 640


def _frames(seed=0):
    from tools import synth
    out = [synth.synthetic_frames(1, h, w, seed=seed + i)[0] for i, (h, w) in enumerate(SHAPES)]
    wide = synth.synthetic_frames(1, 100, 400, seed=seed + 99)[0]
    out[4] = wide[:, 30:361]                     # 100 x 331 whose rows are 400 * 3 bytes apart
    assert out[4].strides[0] == 1200
    return out


def _assert_rows_identical(res, want, pose):
    """bit-exact post-NMS rows: same anchors in the same order, same boxes, scores, classes, keypoints"""
    for r, w in zip(res, want):
        np.testing.assert_array_equal(r.anchor_idx, w["anchor_idx"].numpy())
        np.testing.assert_array_equal(r.boxes.data.numpy(), w["boxes"].numpy())
        if pose and len(r.anchor_idx):
            # Keypoints() zeroes x,y where conf < 0.5 (results.py); apply the same rule to the oracle rows
            k = w["kpts"].clone()
            k[..., :2][k[..., 2] < 0.5] = 0
            np.testing.assert_array_equal(r.keypoints.data.numpy(), k.numpy())


def _assert_same_results(a, b):
    assert len(a) == len(b)
    for r, w in zip(a, b):
        assert r.orig_shape == w.orig_shape
        np.testing.assert_array_equal(r.anchor_idx, w.anchor_idx)
        np.testing.assert_array_equal(r.boxes.data.numpy(), w.boxes.data.numpy())
        if r.keypoints is not None:
            np.testing.assert_array_equal(r.keypoints.data.numpy(), w.keypoints.data.numpy())


def _oracle(dm, frames, conf):
    """the square letterbox of every frame, the canonical-order net on the stack, NMS and the scale-back against each frame's shape"""
    from oracle import yolo_oracle as O
    lb = np.stack([O.letterbox(f, (S, S), auto=False) for f in frames])
    pred = dm.forward_u8(lb)
    rows, idxs = O.non_max_suppression(pred, conf, 0.7, max_det=300, nc=dm.nc, return_idxs=True)
    out = []
    for r, ai, f in zip(rows, idxs, frames):
        r = r.clone()
        r[:, :4] = O.scale_boxes(lb.shape[1:3], r[:, :4], f.shape)
        k = None
        if dm.pose:
            k = r[:, 6:].view(len(r), *dm.kpt_shape).clone()
            k = O.scale_coords(lb.shape[1:3], k, f.shape)
        out.append({"boxes": r[:, :6], "kpts": k, "anchor_idx": ai})
    return out, pred.numpy(), lb


@pytest.fixture(scope="module", params=["yolov8n", "yolov8n-pose"])
def case(request):
    from cvsd_amd import YOLO
    from oracle import det
    from tools import synth
    name = request.param
    ckpt = synth.synthetic_checkpoint(name, seed=0)
    frames = _frames()
    dm = det.DetOracleModel(name, ckpt[1])
    want, pred, lb = _oracle(dm, frames, 0.25)
    return {"name": name, "sd": ckpt[1], "model": YOLO.from_state_dict(name, ckpt[1]), "frames": frames, "want": want, "pred": pred,
            "lb": lb, "pose": dm.pose}


def test_letterbox_multi_equals_oracle_canvas():
    from cvsd_amd import ops
    from oracle import yolo_oracle as O
    frames = _frames(seed=5)
    got = ops.letterbox_multi(frames, S)
    want = np.stack([O.letterbox(f, (S, S), auto=False) for f in frames])
    np.testing.assert_array_equal(got, want)
    # the 7 x 5 frame pads 91 / 92 columns with 114, the 100 x 331 one 223 / 224 rows
    assert (got[5][:, :91] == 114).all() and (got[5][:, 91 + 457:] == 114).all() and not (got[5][:, 91] == 114).all()
    assert (got[4][:223] == 114).all() and (got[4][223 + 193:] == 114).all()


def test_raw_head_equals_oracle(case):
    got = case["model"].raw_head(case["frames"], imgsz=S)
    assert got.shape == case["pred"].shape and got.shape[2] == 8400
    np.testing.assert_array_equal(got, case["pred"])


def test_predict_rows_equal_composed_oracle(case):
    m, frames = case["model"], case["frames"]
    res = m.predict(frames, conf=0.25, imgsz=S)
    assert len(res) == len(frames)
    assert [r.orig_shape for r in res] == SHAPES
    assert all(r.orig_img is f for r, f in zip(res, frames))
    assert sum(len(r) for r in res) > 0
    _assert_rows_identical(res, case["want"], case["pose"])
    if case["pose"]:
        assert all(r.keypoints is not None for r in res)
    rows, shapes = m.detect_rows(m._as_batch(frames)[0], conf=0.25, imgsz=S)
    assert shapes == SHAPES
    for d, r in zip(rows, res):
        np.testing.assert_array_equal(d, r.boxes.data.numpy())


def test_chunked_mixed_batch_equals_one_chunk(case):
    from cvsd_amd import YOLO
    frames = case["frames"][1:]                  # 5 mixed frames; chunks of 2 split them at every other frame boundary
    one = case["model"].predict(frames, conf=0.25, imgsz=S)
    chunked = YOLO.from_state_dict(case["name"], case["sd"], batch_chunk=2).predict(frames, conf=0.25, imgsz=S)
    _assert_same_results(chunked, one)
    _assert_rows_identical(chunked, case["want"][1:], case["pose"])


def test_device_frames_equal_host_frames(case):
    m, frames = case["model"], case["frames"]
    from tools import synth
    dev = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]
    dev[4] = torch.from_numpy(synth.synthetic_frames(1, 100, 400, seed=99)[0]).cuda()[:, 30:361]     # the strided frame, on the GPU
    assert dev[4].stride(0) == 1200
    res = m.predict(dev, conf=0.25, imgsz=S)
    assert all(r.orig_img is None for r in res)
    _assert_same_results(res, m.predict(frames, conf=0.25, imgsz=S))
    _assert_rows_identical(res, case["want"], case["pose"])


def test_half_raw_head_equals_square_stack(case):
    m = case["model"]
    got = m.raw_head(case["frames"], imgsz=S, half=True)
    want = m.raw_head(case["lb"], imgsz=S, half=True)              # the host-letterboxed square canvases, 640 x 640: no letterbox left
    np.testing.assert_array_equal(got, want)


def test_infer_multi_same_shapes_is_the_rect_path(case):
    from cvsd_amd import YOLO
    from tools import synth
    m = case["model"]
    wide = synth.synthetic_frames(3, 240, 360, seed=31)
    frames = [np.ascontiguousarray(wide[0, :, :320]), wide[1, :, 20:340], np.ascontiguousarray(wide[2, :, 40:360])]
    stacked = np.stack(frames)
    want = m.predict(stacked, conf=0.25, imgsz=S)                 # rect letterbox: 480 x 640 canvas
    got = m._predict_batch(YOLO._Ragged(frames, False), frames, 0.25, 0.7, None, 300, S, None)
    _assert_same_results(got, want)
    assert got[0].orig_shape == (240, 320)
