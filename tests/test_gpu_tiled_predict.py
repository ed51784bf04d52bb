"""predict(frames, tile=...): the contract of DESIGN.md 3.17.  A tiled call returns, bit for bit, the rows of predict(entry_list) on
the entries cut out with numpy (every frame's tiles, row-major, then the frame itself), merged per frame by the sequential checker in
tests/_tile_merge_numpy.py -- for host frames, CUDA tensors and YUVFrames, across partial chunks, and for frames of different sizes
in one call.  imgsz 96 on a 160 x 224 frame with tile 96 / overlap 0.25: six identity-letterbox tiles plus the resized full frame."""
import numpy as np
import pytest
import torch

import _tile_merge_numpy as T

pytestmark = pytest.mark.gpu

S, TILE, OV, CONF = 96, 96, 0.25, 0.1


def _frame(h, w, seed):
    from tools import synth
    return synth.synthetic_frames(1, h, w, seed=seed)[0]


@pytest.fixture(scope="module", params=["yolov8n", "yolov8n-pose"])
def case(request):
    from cvsd_amd import YOLO
    from tools import synth
    name = request.param
    sd = synth.synthetic_checkpoint(name, seed=0)[1]
    return {"name": name, "sd": sd, "model": YOLO.from_state_dict(name, sd), "frame": _frame(160, 224, 3)}


def _expected(model, frames, tile=TILE, overlap=OV, full_frame=True, tile_iou=0.5, tile_metric="ios", conf=CONF, max_det=300, **kw):
    """predict() on the numpy crops of every frame's entries, then the checker's merge: per frame (rows [M, 58], tile_idx, entries)"""
    ents = [T.entries(f.shape[0], f.shape[1], tile, overlap, full_frame) for f in frames]
    crops = [np.ascontiguousarray(f[y:y + h, x:x + w]) for f, g in zip(frames, ents) for x, y, w, h in g]
    res = model.predict(crops, conf=conf, max_det=max_det, imgsz=S, **kw)
    nkpt, kdim = model.kpt_shape
    out, at = [], 0
    for f, g in zip(frames, ents):
        rows = np.zeros((len(g), max_det, T.DET_WORDS), np.float32)
        counts = np.zeros(len(g), np.int32)
        for e in range(len(g)):
            r = res[at + e]
            d = r.boxes.data.numpy()
            counts[e] = len(d)
            rows[e, :len(d), :5] = d[:, :5]
            iv = rows[e].view(np.int32)
            iv[:len(d), 5] = d[:, 5].astype(np.int32)
            iv[:len(d), 6] = r.anchor_idx
            if nkpt:
                rows[e, :len(d), 7:7 + nkpt * kdim] = r.keypoints_raw.reshape(len(d), -1)
        at += len(g)
        m, idx = T.merge_frame(rows, counts, g[:, :2], kdim, tile_metric, tile_iou, nk=nkpt * kdim)
        out.append((m, idx, g, counts))
    return out


def _assert_contract(model, res, want):
    nkpt, kdim = model.kpt_shape
    assert len(res) == len(want)
    for r, (m, idx, g, _) in zip(res, want):
        iv = m.view(np.int32)
        np.testing.assert_array_equal(r.tiles, g)
        assert r.tiles.dtype == np.int32 and r.tile_idx.dtype == np.int32
        np.testing.assert_array_equal(r.tile_idx, idx)
        np.testing.assert_array_equal(r.anchor_idx, iv[:, 6])
        d = r.boxes.data.numpy()
        assert np.array_equal(d[:, :5].view(np.uint32), m[:, :5].view(np.uint32))
        np.testing.assert_array_equal(d[:, 5], iv[:, 5].astype(np.float32))
        if nkpt:
            k = m[:, 7:7 + nkpt * kdim].reshape(len(m), nkpt, kdim)
            assert np.array_equal(r.keypoints_raw.view(np.uint32), k.view(np.uint32))
            k = k.copy()
            k[..., :2][k[..., 2] < 0.5] = 0                       # Keypoints() zeroes x, y where conf < 0.5, as ever
            np.testing.assert_array_equal(r.keypoints.data.numpy(), k)
        else:
            assert r.keypoints is None


def test_contract_host_frame(case):
    model, f = case["model"], case["frame"]
    want = _expected(model, [f])
    m, idx, g, counts = want[0]
    assert len(g) == 7 and g[-1].tolist() == [0, 0, 224, 160]
    assert (counts > 0).sum() > 1 and 0 < len(m) < counts.sum()   # several entries bring candidates, and the merge suppresses some of them
    res = model.predict(f, conf=CONF, imgsz=S, tile=TILE, overlap=OV)
    _assert_contract(model, res, want)
    assert res[0].orig_shape == (160, 224) and res[0].orig_img is f
    # a list, a stacked array and a (tile_h, tile_w) pair say the same
    _assert_contract(model, model.predict([f], conf=CONF, imgsz=S, tile=(TILE, TILE), overlap=OV), want)
    _assert_contract(model, model(f[None], conf=CONF, imgsz=S, tile=TILE, overlap=OV), want)


@pytest.mark.parametrize("metric,thr", [("iou", 0.5), ("ios", 0.2)])
def test_metric_and_threshold(case, metric, thr):
    model, f = case["model"], case["frame"]
    want = _expected(model, [f], tile_iou=thr, tile_metric=metric)
    _assert_contract(model, model.predict(f, conf=CONF, imgsz=S, tile=TILE, overlap=OV, tile_iou=thr, tile_metric=metric), want)


def test_without_full_frame_and_filters(case):
    """full_frame=False: six entries of one shape, the rect rule; classes and max_det apply per entry and to the merge"""
    model, f = case["model"], case["frame"]
    want = _expected(model, [f], full_frame=False)
    assert len(want[0][2]) == 6
    _assert_contract(model, model.predict(f, conf=CONF, imgsz=S, tile=TILE, overlap=OV, full_frame=False), want)
    # max_det 5 and a merge that removes near-copies only (IoU > 0.9): up to 35 candidates, the merge stops at 5
    kw = dict(max_det=5, iou=0.5, tile_metric="iou", tile_iou=0.9)
    want = _expected(model, [f], **kw)
    assert len(want[0][0]) <= 5 and want[0][3].max() <= 5
    if model.task == "pose":                                      # (its synthetic head fills every entry's five rows)
        assert len(want[0][0]) == 5 and want[0][3].sum() > 5
    _assert_contract(model, model.predict(f, conf=CONF, imgsz=S, tile=TILE, overlap=OV, **kw), want)
    kw = dict(classes=[0, 1, 2, 40], max_det=50)
    want = _expected(model, [f], **kw)
    assert all(c in (0, 1, 2, 40) for c in want[0][0].view(np.int32)[:, 5])
    _assert_contract(model, model.predict(f, conf=CONF, imgsz=S, tile=TILE, overlap=OV, **kw), want)


def test_two_frames_of_different_sizes(case):
    model = case["model"]
    small = np.ascontiguousarray(case["frame"][:90, 72:168])               # 90 x 96: no larger than the tile
    frames = [case["frame"], _frame(120, 100, 8), small]                  # 7, 5 and 2 entries
    want = _expected(model, frames)
    assert [len(w[2]) for w in want] == [7, 5, 2]
    m, _, g, counts = want[2]
    assert np.array_equal(g[0], g[1]) and counts[0] == counts[1]           # tile and full frame coincide, and so do their rows:
    assert len(m) <= counts[0]                                             # the merge removes the copies
    _assert_contract(model, model.predict(frames, conf=CONF, imgsz=S, tile=TILE, overlap=OV), want)


def test_entries_straddle_chunks(case):
    from cvsd_amd import YOLO
    model = YOLO.from_state_dict(case["name"], case["sd"], batch_chunk=4)
    frames = [case["frame"], _frame(160, 224, 11)]                        # 14 entries in chunks of 4: 4 + 3 | 1 + 4 | 4 + ... + 2
    want = _expected(model, frames)
    _assert_contract(model, model.predict(frames, conf=CONF, imgsz=S, tile=TILE, overlap=OV), want)
    _assert_contract(case["model"], case["model"].predict(frames, conf=CONF, imgsz=S, tile=TILE, overlap=OV), want)   # ... as one chunk


def test_many_frames_take_the_compacted_copy(case):
    """more than 16 frames: the merged rows are compacted on the GPU and copied, instead of written straight to pinned memory"""
    model = case["model"]
    frames = [_frame(100, 120, 20 + i) for i in range(17)] + [np.full((100, 120, 3), 114, np.uint8)]
    want = _expected(model, frames)
    _assert_contract(model, model.predict(frames, conf=CONF, imgsz=S, tile=TILE, overlap=OV), want)


def test_cuda_tensor_and_pitched_host_frame(case):
    model, f = case["model"], case["frame"]
    want = _expected(model, [f])
    t = torch.from_numpy(f).cuda()
    res = model.predict(t, conf=CONF, imgsz=S, tile=TILE, overlap=OV)
    _assert_contract(model, res, want)
    wide = torch.zeros((160, 300, 3), dtype=torch.uint8, device="cuda")
    wide[:, 40:264] = t
    _assert_contract(model, model.predict([wide[:, 40:264]], conf=CONF, imgsz=S, tile=TILE, overlap=OV), want)     # a pitched CUDA frame
    hw = np.zeros((160, 300, 3), np.uint8)
    hw[:, 40:264] = f
    pitched = hw[:, 40:264]
    assert pitched.strides[0] == 900 and not pitched.flags.c_contiguous
    _assert_contract(model, model.predict(pitched, conf=CONF, imgsz=S, tile=TILE, overlap=OV), want)


@pytest.mark.parametrize("where", ["host", "cuda"])
def test_nv12_frame(case, where):
    from cvsd_amd import YUVFrame
    model = case["model"]
    rng = np.random.default_rng(5)
    y = rng.integers(16, 236, (160, 224), dtype=np.uint8)
    uv = rng.integers(16, 241, (80, 224), dtype=np.uint8)
    yf = YUVFrame(y, uv=uv, fmt="nv12")
    bgr = yf.to_bgr(0)
    want = _expected(model, [bgr])
    if where == "cuda":
        yf = YUVFrame(torch.from_numpy(y).cuda(), uv=torch.from_numpy(uv).cuda(), fmt="nv12")
    res = model.predict(yf, conf=CONF, imgsz=S, tile=TILE, overlap=OV)
    _assert_contract(model, res, want)
    ref = model.predict(bgr, conf=CONF, imgsz=S, tile=TILE, overlap=OV)
    for a, b in zip(res, ref):
        np.testing.assert_array_equal(a.boxes.data.numpy(), b.boxes.data.numpy())
        np.testing.assert_array_equal(a.tile_idx, b.tile_idx)


def test_untiled_predict_is_unchanged_by_a_tiled_call(case):
    model, f = case["model"], case["frame"]
    before = model.predict(f, conf=CONF, imgsz=S)
    h0 = model.plan_info()
    model.predict(f, conf=CONF, imgsz=S, tile=TILE, overlap=OV)
    after = model.predict(f, conf=CONF, imgsz=S)
    h1 = model.plan_info()
    assert h0["plan_hash"] == h1["plan_hash"] and h0["launches_per_pass"] == h1["launches_per_pass"]
    assert h0["activation_bytes"] == h1["activation_bytes"]
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a.boxes.data.numpy(), b.boxes.data.numpy())
        np.testing.assert_array_equal(a.anchor_idx, b.anchor_idx)
        assert a.tile_idx is None and a.tiles is None and b.tile_idx is None
        if a.keypoints is not None:
            np.testing.assert_array_equal(a.keypoints.data.numpy(), b.keypoints.data.numpy())


def test_track_consumes_the_merged_rows(case):
    from cvsd_amd.tracker import BYTETracker
    from tools import synth
    model = case["model"]
    clip = synth.synthetic_clip(4, 160, 224, seed=2)
    tracker = BYTETracker(gmc_device=0)
    for i, f in enumerate(clip):
        got = model.track(f, persist=i > 0, tile=TILE, overlap=OV, imgsz=S)[0]
        r = model.predict(f, conf=0.1, imgsz=S, tile=TILE, overlap=OV)[0]
        tracks = tracker.update(r.boxes.data.numpy(), f)
        if len(tracks):
            r = r[tracks[:, -1].astype(int)]
            r.update(boxes=torch.as_tensor(tracks[:, :-1], dtype=torch.float32))
        np.testing.assert_array_equal(got.boxes.data.numpy(), r.boxes.data.numpy())
        np.testing.assert_array_equal(got.tile_idx, r.tile_idx)
        np.testing.assert_array_equal(got.tiles, r.tiles)
    model._tracker = None


def test_refusals(case):
    model, f = case["model"], case["frame"]
    kw = dict(conf=CONF, imgsz=S)
    with pytest.raises(ValueError, match="feats"):
        model.predict(f, tile=TILE, feats=True, **kw)
    with pytest.raises(ValueError, match="tile"):
        model.predict(f, tile=31, **kw)
    with pytest.raises(TypeError, match="tile"):
        model.predict(f, tile="96", **kw)
    for ov in (-0.01, 1.0):
        with pytest.raises(ValueError, match="overlap"):
            model.predict(f, tile=TILE, overlap=ov, **kw)
    with pytest.raises(ValueError, match="tile_metric"):
        model.predict(f, tile=TILE, tile_metric="giou", **kw)
    for thr in (-0.1, 1.01):
        with pytest.raises(ValueError, match="tile_iou"):
            model.predict(f, tile=TILE, tile_iou=thr, **kw)
    big = np.zeros((32 * 9, 32 * 9, 3), np.uint8)                          # 9 x 9 tiles of 32 + the frame = 82 entries
    with pytest.raises(ValueError, match="tile"):
        model.predict(big, tile=32, overlap=0, **kw)
    with pytest.raises(ValueError, match="tile"):
        model.predict(big, tile=32, overlap=0, full_frame=False, max_det=1000, **kw)          # 81 entries
    with pytest.raises(TypeError):
        model.track_cameras([f], tile=TILE)                                # out of scope, refused as any unknown argument
