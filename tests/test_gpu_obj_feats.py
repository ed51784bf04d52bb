"""Object features on the GPU: the gather kernel alone against tests/_obj_feats_numpy.py (exact equality, fp32 and fp16
maps), ``Results.feats`` end to end against the canonical-order CPU oracle's Detect inputs (bit for bit in fp32; within the fp16 storage
contract's own noise with half=True), and ``track`` / ``track_cameras`` with ``with_reid`` against the same steps written by hand."""
import ctypes as C

import numpy as np
import pytest
import torch

import _obj_feats_numpy as R
from cvsd_amd import _lib, ops
from tools import synth

pytestmark = pytest.mark.gpu

POSE = "yolov8n-pose"


def _model(name, **kw):
    from cvsd_amd import YOLO
    _, sd = synth.synthetic_checkpoint(name, seed=0)
    return YOLO.from_state_dict(name, sd, device=0, **kw)


# ---------------------------------------------------------------------------------------------------------------- the op alone
SIZES = {"square": [(8, 8), (4, 4), (2, 2)], "oblong": [(6, 10), (3, 5), (2, 3)]}


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("sizes", sorted(SIZES))
@pytest.mark.parametrize("chans", [(64, 128, 256), (192, 384, 576), (16, 16, 16), (32,)], ids=lambda c: "x".join(map(str, c)))
def test_gather_kernel_equals_the_sequential_group_mean(chans, sizes, half):
    """g = 1 / 2 / 4, g = 3 (192, 384, 576), g = 1 on every level, one level alone.  The maps are channel views (cs = C + 16, c_off = 8)
    whose pad channels hold NaN; n = 3 frames keep (cap, 0, 1) rows; frame 0's anchors include the first and the last of every level;
    slots at or beyond a frame's count keep the sentinel's bits."""
    rng = np.random.default_rng(sum(chans) + len(sizes) + 2 * half)
    n, pad, c_off = 3, 16, 8
    hw = SIZES[sizes][:len(chans)]
    dt = np.float16 if half else np.float32
    levels, starts, a = [], [], 0
    for c, (h, w) in zip(chans, hw):
        buf = np.full((n, h, w, c + pad), np.nan, dt)
        buf[..., c_off:c_off + c] = rng.normal(0, 2, (n, h, w, c)).astype(dt)
        levels.append((buf, c_off, c))
        starts.append(a)
        a += h * w
    edge = sorted(set(starts + [s - 1 for s in starts[1:]] + [a - 1]))                # first and last anchor of every level
    cap = len(edge) + 7
    idx = rng.integers(0, a, (n, cap)).astype(np.int32)
    idx[0, :len(edge)] = edge
    idx[0] = rng.permutation(idx[0])
    counts = np.array([cap, 0, 1], np.int32)
    got = ops.obj_feats(levels, idx, counts, half=half)
    want = R.obj_feats(levels, idx, counts, ops.SENTINEL)
    assert got.shape == (n, cap, min(chans)) and got.dtype == np.float32
    assert np.isfinite(want[0]).all() and np.isfinite(want[2, :1]).all()              # no pad channel leaked into the reference
    assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    assert (got.view(np.uint32)[1] == ops.SENTINEL_BITS).all() and (got.view(np.uint32)[2, 1:] == ops.SENTINEL_BITS).all()


def test_gather_op_refuses_what_the_launcher_cannot_address():
    buf = np.zeros((1, 2, 2, 24), np.float32)
    idx, cnt = np.zeros((1, 2), np.int32), np.array([1], np.int32)
    with pytest.raises(ValueError):
        ops.obj_feats([(buf, 2, 16)], idx, cnt)                                       # c_off not a multiple of 4
    with pytest.raises(ValueError):
        ops.obj_feats([(buf, 0, 16), (buf, 0, 24)], idx, cnt)                         # 16 does not divide 24
    with pytest.raises(ValueError):
        ops.obj_feats([(buf, 0, 16)], idx + 4, cnt)                                   # anchor beyond the map
    with pytest.raises(ValueError):
        ops.obj_feats([(buf, 0, 16)], idx, np.array([3], np.int32))                   # count beyond cap


# ---------------------------------------------------------------------------------------------------------------- end to end, fp32
FRAMES = dict(n=3, size=128, seed=31, conf=0.05)


@pytest.fixture(scope="module")
def pose():
    return _model(POSE, feats=True, batch_chunk=2)


@pytest.fixture(scope="module")
def pose_results(pose):
    frames = synth.synthetic_frames(FRAMES["n"], FRAMES["size"], FRAMES["size"], seed=FRAMES["seed"])
    return frames, pose.predict(frames, conf=FRAMES["conf"], imgsz=FRAMES["size"])      # two chunks: frames 0-1, then frame 2 alone


def _oracle_tables(frames, size, half=False, mkldnn=True):
    """per frame [A, s]: the group means of the oracle's Detect inputs, levels concatenated in anchor order"""
    from oracle import det
    from oracle import yolo_oracle as O
    _, sd = synth.synthetic_checkpoint(POSE, seed=0)
    if half:
        om = O.OracleModel(POSE, sd, half=True)
        with torch.backends.mkldnn.flags(enabled=mkldnn):
            maps = om.forward(O.preprocess(list(frames), size), return_features=True)
    else:
        om = det.DetOracleModel(POSE, sd)
        lb = np.stack([O.letterbox(f, (size, size)) for f in frames])
        om._u8 = np.ascontiguousarray(lb)                                               # as forward_u8 does
        try:
            maps = om.forward(torch.zeros((len(lb), 3, *lb.shape[1:3])), return_features=True)
        finally:
            om._u8 = None
    nhwc = [np.ascontiguousarray(m.permute(0, 2, 3, 1).numpy()) for m in maps]
    s = min(m.shape[-1] for m in nhwc)
    table = np.concatenate([R.group_mean(m.reshape(len(frames), -1, m.shape[-1]), s) for m in nhwc], axis=1)
    return table, np.cumsum([0] + [m.shape[1] * m.shape[2] for m in nhwc])


def test_results_feats_are_the_oracles_detect_inputs_bit_for_bit(pose, pose_results):
    frames, res = pose_results
    table, starts = _oracle_tables(frames, FRAMES["size"])
    assert table.shape[2] == 64
    for i, r in enumerate(res):
        per_level = np.histogram(r.anchor_idx, bins=starts)[0]
        print(f"[obj_feats] frame {i}: {len(r)} rows, per level {per_level.tolist()}")
        assert len(r) >= 20 and (per_level >= 1).all(), "the check needs rows from every level"
        assert r.feats.shape == (len(r), 64) and r.feats.dtype == np.float32
        want = table[i, r.anchor_idx]
        assert r.feats.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), f"frame {i}"
        sub = r[np.array([2, 0])]                                                       # Results.__getitem__ carries the features
        np.testing.assert_array_equal(sub.feats, r.feats[[2, 0]])


def test_feats_off_returns_the_same_rows(pose, pose_results):
    frames, res = pose_results
    off = pose.predict(frames, conf=FRAMES["conf"], imgsz=FRAMES["size"], feats=False)   # the second engine, without the option
    for a, b in zip(res, off):
        assert b.feats is None
        assert a.boxes.data.numpy().tobytes() == b.boxes.data.numpy().tobytes()
        assert a.keypoints.data.numpy().tobytes() == b.keypoints.data.numpy().tobytes()
        np.testing.assert_array_equal(a.anchor_idx, b.anchor_idx)


def test_feats_do_not_depend_on_sharing_arena_bytes(pose_results):
    frames, res = pose_results
    plain = _model(POSE, feats=True, batch_chunk=2, flags=_lib.OPT_NO_MEM_REUSE)
    for a, b in zip(res, plain.predict(frames, conf=FRAMES["conf"], imgsz=FRAMES["size"])):
        assert a.boxes.data.numpy().tobytes() == b.boxes.data.numpy().tobytes()
        assert a.feats.tobytes() == b.feats.tobytes()


def test_frames_of_two_sizes_in_one_call_equal_each_frame_alone(pose):
    """128 x 128 and 96 x 96: both letterbox to the 128 x 128 canvas alone (rect path) and together (square canvas of the mixed path)"""
    a = synth.synthetic_frames(2, 128, 128, seed=5)
    b = synth.synthetic_frames(1, 96, 96, seed=6)
    frames = [a[0], b[0], a[1]]                                                        # chunks of two: a mixed chunk, then a tail
    together = pose.predict(frames, conf=0.05, imgsz=128)
    rows = 0
    for f, r in zip(frames, together):
        alone = pose.predict(f, conf=0.05, imgsz=128)[0]
        assert r.boxes.data.numpy().tobytes() == alone.boxes.data.numpy().tobytes()
        assert r.feats.shape == alone.feats.shape and r.feats.tobytes() == alone.feats.tobytes()
        rows += len(r)
    assert rows >= 20


def test_chunks_on_several_streams_keep_their_own_maps():
    """passes of six frames or more are dealt to several HIP streams along the op DAG: two full chunks of 6 and a tail of 2 in one call,
    every chunk's gather running between its NMS and the next chunk's pass, against each frame run alone (one in-order stream)"""
    m = _model(POSE, feats=True, batch_chunk=6)
    frames = synth.synthetic_frames(14, 128, 128, seed=77)
    together = m.predict(frames, conf=0.05, imgsz=128)
    rows = 0
    for f, r in zip(frames, together):
        alone = m.predict(f, conf=0.05, imgsz=128)[0]
        assert r.boxes.data.numpy().tobytes() == alone.boxes.data.numpy().tobytes()
        assert r.feats.shape == alone.feats.shape and r.feats.tobytes() == alone.feats.tobytes()
        rows += len(r)
    assert rows >= 14 * 20
    assert [x.feats.tobytes() for x in m.predict(frames, conf=0.05, imgsz=128)] == [x.feats.tobytes() for x in together]


def test_device_frames_and_no_direct_rows_give_the_same_features(pose, pose_results):
    """the rows reach the host three ways (written by the NMS kernel into pinned memory; compacted and copied; from frames on the device):
    the features follow each of them"""
    frames, res = pose_results
    dev = pose.predict(torch.from_numpy(frames).cuda(), conf=FRAMES["conf"], imgsz=FRAMES["size"])
    copied = _model(POSE, feats=True, flags=_lib.OPT_NO_DIRECT_ROWS)                     # one chunk of three, rows copied
    for a, b, c in zip(res, dev, copied.predict(frames, conf=FRAMES["conf"], imgsz=FRAMES["size"])):
        assert a.feats.tobytes() == b.feats.tobytes() == c.feats.tobytes()
        assert a.boxes.data.numpy().tobytes() == c.boxes.data.numpy().tobytes()
    one = pose.predict(frames[1], conf=FRAMES["conf"], imgsz=FRAMES["size"])[0]          # a single frame: direct rows
    assert one.feats.tobytes() == res[1].feats.tobytes()


def test_abi_without_the_option_and_after_an_asynchronous_call(pose):
    lib = _lib.lib()
    plain = _model(POSE)
    dim = C.c_int(-1)
    _lib.check(lib.mi355_yolo_feat_dim(plain._h, C.byref(dim)))
    assert dim.value == 0
    frames = synth.synthetic_frames(1, 128, 128, seed=1)
    plain.predict(frames, imgsz=128)
    out = np.empty((1, 300, 64), np.float32)
    assert lib.mi355_yolo_last_feats(plain._h, out.ctypes.data, 300, 1) == -1           # MI355_EINVAL: option off
    _lib.check(lib.mi355_yolo_feat_dim(pose._h, C.byref(dim)))
    assert dim.value == 64
    pose.predict(frames, imgsz=128)
    assert lib.mi355_yolo_last_feats(pose._h, out.ctypes.data, 300, 1) == 0
    assert lib.mi355_yolo_last_feats(pose._h, out.ctypes.data, 300, 2) == -1            # n of another call
    bufs = pose.new_device_rows(1)
    pose.infer_async(torch.from_numpy(frames).cuda(), bufs, imgsz=128)                  # runs unchanged, produces no features
    pose.sync()
    assert lib.mi355_yolo_last_feats(pose._h, out.ctypes.data, 300, 1) == -1


# ---------------------------------------------------------------------------------------------------------------- half=True
def _q(d):
    d = np.abs(d).ravel()
    return np.array([np.median(d), np.quantile(d, 0.99), d.max()])


def test_half_feats_within_the_storage_contracts_own_noise():
    """Rows matched by anchor_idx against OracleModel(half=True)'s Detect inputs.  The yardstick is that of
    tests/test_gpu_half.py::test_raw_head_within_the_contracts_own_noise: the oracle's own distance between two fp32 summation orders
    (mkldnn on / off), taken at the same anchors, with that test's margins 1.5 / 1.5 / 4.0 on median / p99 / max.
    Measured on MI355X (453 rows): noise 9.8e-4 / 1.4e-2 / 4.1e-2, error 9.8e-4 / 1.4e-2 / 4.3e-2: err / noise = 1.00 at the median and
    the p99, 1.05 at the max."""
    size, n = 320, 2
    frames = synth.synthetic_frames(n, size, size, seed=31)
    res = _model(POSE, half=True, feats=True).predict(frames, conf=0.05, imgsz=size)
    a, _ = _oracle_tables(frames, size, half=True, mkldnn=True)
    b, _ = _oracle_tables(frames, size, half=True, mkldnn=False)
    got = np.concatenate([r.feats for r in res])
    ra = np.concatenate([a[i, r.anchor_idx] for i, r in enumerate(res)])
    rb = np.concatenate([b[i, r.anchor_idx] for i, r in enumerate(res)])
    assert len(got) >= 40 and got.shape[1] == 64 and np.isfinite(got).all()
    noise, err = _q(ra - rb), _q(got - ra)
    print(f"[obj_feats half] {len(got)} rows: noise median / p99 / max {noise}, error {err}, ratios {err / np.maximum(noise, 1e-12)}")
    assert err[0] <= 1.5 * noise[0] + 1e-6, ("median", err, noise)
    assert err[1] <= 1.5 * noise[1] + 1e-5, ("p99", err, noise)
    assert err[2] <= 4.0 * noise[2] + 1e-4, ("max", err, noise)


# ---------------------------------------------------------------------------------------------------------------- tracking
def _same(got, want):
    assert got.boxes.data.numpy().tobytes() == want.boxes.data.numpy().tobytes()
    assert got.keypoints.data.numpy().tobytes() == want.keypoints.data.numpy().tobytes()
    assert (got.feats is None) == (want.feats is None) and (got.feats is None or got.feats.tobytes() == want.feats.tobytes())
    return got.boxes.id.numpy().astype(int).tolist() if got.boxes.is_track else []


def _by_hand(res, tracks):
    if len(tracks):
        res = res[tracks[:, -1].astype(int)]
        res.update(boxes=torch.as_tensor(tracks[:, :-1], dtype=torch.float32))
    return res


def test_track_with_reid_is_predict_plus_the_tracker_by_hand():
    from cvsd_amd import gmc
    from cvsd_amd.tracker import BYTETracker
    clip = np.ascontiguousarray(synth.synthetic_clip(10, 240, 320, seed=5))
    a, b = _model(POSE), _model(POSE)
    hand, motion = BYTETracker(gmc_method=None, with_reid=True), gmc.GMC(device=0)
    ids, with_feats = [], 0
    for f in clip:
        got = a.track(f, persist=True, tracker={"with_reid": True})[0]
        res = b.predict(f, conf=0.1, feats=True)[0]
        with_feats += len(res)
        want = _by_hand(res, hand.update(res.boxes.data.numpy(), warp=motion.apply(f), feats=res.feats))
        ids += _same(got, want)
    assert ids and with_feats > 0
    assert a._tracker.with_reid and all(a._tracker.smooth_feat(t.track_id) is not None for t in a._tracker.tracked_stracks)
    with pytest.raises(ValueError, match="match_thresh"):
        a.track(clip[0], tracker={"match_thresh": 0.5})
    frame_id = a._tracker.frame_id
    with pytest.raises(ValueError, match="differ"):                              # a continued tracker does not silently keep other settings
        a.track(clip[0], persist=True, tracker={"with_reid": True, "appearance_thresh": 0.5})
    with pytest.raises(ValueError, match="differ"):
        a.track(clip[0], persist=True, tracker={"with_reid": False})
    assert a._tracker.frame_id == frame_id                                       # the refused calls stepped nothing
    a.track(clip[0], persist=True)                                               # no argument: continues as it is
    a.track(clip[0], persist=True, tracker={"tracker_type": "botsort", "with_reid": True, "proximity_thresh": 0.5})    # the same settings
    assert a._tracker.frame_id == frame_id + 2 and a._tracker.with_reid


def test_track_cameras_with_reid_is_one_such_tracker_per_camera():
    from cvsd_amd import gmc
    from cvsd_amd.tracker import BYTETracker
    sizes = [(240, 320), (200, 300)]
    clips = [np.ascontiguousarray(synth.synthetic_clip(8, h, w, seed=3 + i)) for i, (h, w) in enumerate(sizes)]
    a, b = _model(POSE), _model(POSE)
    hand = [BYTETracker(gmc_method=None, with_reid=True) for _ in sizes]
    motion = [gmc.GMC(device=0) for _ in sizes]
    ids = []
    for t in range(8):
        frames = [c[t] for c in clips]
        if t == 3:
            frames[1] = None
        got = a.track_cameras(frames, persist=True, tracker={"tracker_type": "botsort", "with_reid": True, "model": "auto"})
        present = [i for i, f in enumerate(frames) if f is not None]
        res = b.predict([frames[i] for i in present], conf=0.1, feats=True)
        for r, i in zip(res, present):
            ids += _same(got[i], _by_hand(r, hand[i].update(r.boxes.data.numpy(), warp=motion[i].apply(frames[i]), feats=r.feats)))
        assert got[1] is not None or t == 3
    assert ids


def test_yolo11n_feats():
    m = _model("yolo11n", feats=True)
    frames = synth.synthetic_frames(2, 160, 160, seed=9)
    r1 = m.predict(frames, conf=0.001, imgsz=160)
    r2 = m.predict(frames, conf=0.001, imgsz=160)
    for a, b in zip(r1, r2):
        assert a.feats.shape == (len(a), 64) and a.feats.dtype == np.float32 and np.isfinite(a.feats).all()
        assert a.feats.tobytes() == b.feats.tobytes()
    print(f"[obj_feats] yolo11n rows {[len(r) for r in r1]}")
    assert sum(len(r) for r in r1) > 0
