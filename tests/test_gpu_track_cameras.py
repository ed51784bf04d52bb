"""Several cameras per call on the GPU.  ``gmc.MultiGMC(device=0)`` (descriptor-driven kernels, one launch per stage for all cameras)
against one ``gmc.GMC(device=0)`` per camera: bit for bit.  ``YOLO.track_cameras`` against the composition a user writes without it --
``model.predict(present_frames, conf=0.1)`` and, per camera, ``BYTETracker(gmc_device=0).update(rows, frame)`` on a tracker of its own:
``boxes.data`` (ids included), ``keypoints.data`` and ``orig_shape`` equal per camera and tick.  The feature adds no arithmetic, so
nothing here has a tolerance of its own; the device-vs-host bound is the one tests/test_gpu_gmc.py uses."""
import ctypes as C

import numpy as np
import pytest
import torch

from cvsd_amd import gmc
from tools import synth

pytestmark = pytest.mark.gpu

MIXED = [(240, 320), (480, 640), (360, 640), (200, 300)]
EQUAL = [(240, 320)] * 4


def _clips(n, sizes, seed=3):
    return [np.ascontiguousarray(synth.synthetic_clip(n, h, w, seed=seed + i)) for i, (h, w) in enumerate(sizes)]


def _model(name, **kw):
    from cvsd_amd import YOLO
    _, sd = synth.synthetic_checkpoint(name, seed=0)
    return YOLO.from_state_dict(name, sd, device=0, **kw)


def _device_bytes(ptr, nbytes):
    back = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(C.c_void_p(back.data_ptr()), C.c_void_p(ptr), C.c_size_t(nbytes), C.c_int(3)) == 0      # device -> device
    return back.cpu().numpy()


@pytest.mark.parametrize("layout", ["mixed", "equal"])
def test_multi_gmc_is_one_single_object_per_camera_bit_for_bit(layout):
    """24 ticks, four cameras: a 1-pixel-high plane, a plane below the 21 x 21 window (no pyramid level), an odd size and a larger one --
    or four of one size; cameras skip ticks, one is reset, one changes size.  Warps, previous planes and corner lists equal those of four
    GMC(device=0) objects exactly, and follow four host objects within the bound of tests/test_gpu_gmc.py (2e-3 on the warp where small or
    large planes are involved, 1e-3 on 240 x 320; planes and corner lists exactly)."""
    n = 24
    if layout == "mixed":
        sizes = [(2, 80), (40, 48), (97, 131), (480, 640)]
        clips = [np.ascontiguousarray(synth.synthetic_clip(n, 64, 96, seed=2)[:, 30:32, :80]), *_clips(n, sizes[1:], seed=7)]
        other = np.ascontiguousarray(synth.synthetic_clip(n, 120, 160, seed=19))
    else:
        clips = _clips(n, EQUAL, seed=11)
        other = None
    multi = gmc.MultiGMC(4, device=0)
    dev, host = [gmc.GMC(device=0) for _ in range(4)], [gmc.GMC() for _ in range(4)]
    moved = 0
    for t in range(n):
        frames = [c[t] for c in clips]
        if other is not None and 9 <= t < 15:
            frames[2] = other[t]                                                    # camera 2 changes size, and back
        if t % 5 == 3:
            frames[1] = None
        if t in (6, 7):
            frames[3] = None
        if t == 12:
            multi.reset(camera=0); dev[0].reset(); host[0].reset()
        multi.begin(frames)
        ptrs = multi.pending_device_frames()
        assert [p is None for p in ptrs] == [f is None for f in frames]
        if t in (0, 10):
            for p, f in zip(ptrs, frames):
                if f is not None:
                    assert p % 16 == 0
                    np.testing.assert_array_equal(_device_bytes(p, f.size), f.ravel())
        H = multi.apply(frames)
        for i in range(4):
            if frames[i] is None:
                np.testing.assert_array_equal(H[i], np.eye(2, 3))
                continue
            np.testing.assert_array_equal(H[i], dev[i].apply(frames[i]))
            np.testing.assert_allclose(H[i], host[i].apply(frames[i]), atol=1e-3 if frames[i].shape[:2] == (240, 320) else 2e-3)
        for i in range(4):
            a = multi.prev_frame(i)
            assert (a is None) == (dev[i].prev_frame is None)
            if a is not None:
                np.testing.assert_array_equal(a, dev[i].prev_frame)
                np.testing.assert_array_equal(multi.prev_points(i), dev[i].prev_points)
                np.testing.assert_array_equal(a, host[i].prev_frame)
                np.testing.assert_array_equal(multi.prev_points(i), host[i].prev_points)
        moved += int(np.abs(H - np.eye(2, 3)).max() > 0.05)
    assert moved >= n // 3                                                          # the clips pan: not an equality of identities
    if layout == "mixed":
        assert multi.prev_frame(0).shape == (1, 40)


def _oracle_tick(model, trackers, frames, conf, **kw):
    """what a user writes without track_cameras: one predict over the present frames, one tracker (with its own GMC) per camera"""
    present = [i for i, f in enumerate(frames) if f is not None]
    out = [None] * len(frames)
    if not present:
        return out
    res = model.predict([frames[i] for i in present], conf=conf, **kw)
    for r, i in zip(res, present):
        tracks = trackers[i].update(r.boxes.data.numpy(), frames[i])
        if len(tracks):
            r = r[tracks[:, -1].astype(int)]
            r.update(boxes=torch.as_tensor(tracks[:, :-1], dtype=torch.float32))
        out[i] = r
    return out


def _same_results(got, want):
    ids = []
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is None:
            continue
        np.testing.assert_array_equal(g.boxes.data.numpy(), w.boxes.data.numpy())
        assert tuple(g.orig_shape) == tuple(w.orig_shape)
        assert (g.keypoints is None) == (w.keypoints is None)
        if g.keypoints is not None:
            np.testing.assert_array_equal(g.keypoints.data.numpy(), w.keypoints.data.numpy())
        assert g.boxes.is_track == w.boxes.is_track
        if g.boxes.is_track:
            ids.extend(g.boxes.id.numpy().astype(int).tolist())
    return ids


@pytest.mark.parametrize("layout", ["mixed", "equal"])
@pytest.mark.parametrize("name", ["yolov8n", "yolov8n-pose"])
def test_track_cameras_is_predict_plus_one_tracker_per_camera(name, layout):
    """30 ticks of four cameras (mixed sizes: the square-canvas path; one size: the rect path), a camera absent on some ticks, a flat frame,
    and a tick at conf = 1.0 where no camera's frame yields a detection (the trackers still step)"""
    from cvsd_amd.tracker import BYTETracker
    n = 30
    sizes = MIXED if layout == "mixed" else EQUAL
    clips = _clips(n, sizes)
    model = _model(name)
    trackers = [BYTETracker(gmc_device=0) for _ in range(4)]
    ids, empty_ticks = [], 0
    for t in range(n):
        frames = [c[t] for c in clips]
        if t % 7 == 4:
            frames[2] = None
        if t in (10, 11, 12):
            frames[0] = None
        if t == 15:
            frames[1] = np.zeros_like(frames[1])
        conf = 1.0 if t == 20 else None
        got = model.track_cameras(frames, persist=True, conf=conf)
        want = _oracle_tick(model, trackers, frames, 0.1 if conf is None else conf)
        ids.append(_same_results(got, want))
        if t == 20:
            assert all(len(g.boxes) == 0 and not g.boxes.is_track for g in got if g is not None)
            empty_ticks += 1
    assert empty_ticks == 1
    assert sum(len(i) for i in ids) > 0 and min(min(i) for i in ids if i) == 1       # ids did appear, the first of a camera is 1
    assert any(ids[t] for t in range(21, n))                                        # ... and after the empty tick too


def test_one_camera_is_track():
    """track_cameras([f])[0] against model.track(f, persist=True)[0] of a second YOLO object on the same weights"""
    clip = _clips(16, [(240, 320)], seed=5)[0]
    a, b = _model("yolov8n-pose"), _model("yolov8n-pose")
    ids = []
    for f in clip:
        got, want = a.track_cameras([f], persist=True), b.track(f, persist=True)
        assert len(got) == 1
        ids += _same_results(got, want)
    assert ids


def test_rows_do_not_depend_on_sharing_the_uploaded_frames(monkeypatch):
    clips = _clips(10, MIXED)
    outs = []
    for share in ("1", "0"):
        monkeypatch.setenv("MI355_TRACK_SHARED_FRAME", share)
        model = _model("yolov8n")
        outs.append([model.track_cameras([c[t] if (t + i) % 6 else None for i, c in enumerate(clips)], persist=True) for t in range(10)])
    ids = []
    for got, want in zip(*outs):
        ids += _same_results(got, want)
    assert ids


def test_ids_are_per_camera_and_persist_false_restarts_them():
    """Every camera's ids come from its own tracker's counter (``_ids_issued``, which starts at 0 per tracker): no id of a camera exceeds
    the number its tracker has issued, which a counter shared between cameras would break as soon as two cameras have tracks, and cameras
    use the same id values.  (The FIRST id a camera shows need not be 1: a track that is created unconfirmed and not matched again
    is never reported.)"""
    clips = _clips(8, MIXED)
    model = _model("yolov8n")
    seen = [set() for _ in range(4)]
    for t in range(6):
        res = model.track_cameras([c[t] for c in clips], persist=True)
        for i, r in enumerate(res):
            if r.boxes.is_track:
                seen[i].update(r.boxes.id.numpy().astype(int).tolist())
    trackers = model._cameras[0]
    assert all(tr.frame_id == 6 for tr in trackers)
    assert sum(1 for s in seen if s) >= 2
    for s, tr in zip(seen, trackers):
        assert not s or (min(s) >= 1 and max(s) <= tr._ids_issued)
    with_ids = [s for s in seen if s]
    assert any(a & b for k, a in enumerate(with_ids) for b in with_ids[k + 1:])     # two cameras use the same id value: separate id spaces
    with pytest.raises(ValueError):
        model.track_cameras([c[6] for c in clips][:3], persist=True)                # the list length is the number of cameras
    with pytest.raises(ValueError):
        model.track_cameras([clips[0][6][:, :, 0], None, None, None], persist=True)
    assert all(tr.frame_id == 6 for tr in model._cameras[0])                        # the refused calls stepped nothing
    again = []
    for t in range(6, 8):
        res = model.track_cameras([c[t] for c in clips], persist=(t > 6))           # tick 6: persist=False starts all cameras afresh
        if t == 6:
            assert all(tr is not old for tr, old in zip(model._cameras[0], trackers))
            assert all(tr.frame_id == 1 for tr in model._cameras[0])
        for i, r in enumerate(res):
            if r.boxes.is_track:
                ids = r.boxes.id.numpy().astype(int)
                assert ids.min() >= 1 and ids.max() <= model._cameras[0][i]._ids_issued
                again += ids.tolist()
    assert again and all(tr.frame_id == 2 for tr in model._cameras[0])
    assert all(r is None for r in model.track_cameras([None] * 4, persist=True))
    # track() and predict() still refuse / accept mixed lists as before
    with pytest.raises(ValueError):
        model.track([clips[0][0], clips[1][0]])
    assert len(model.predict([clips[0][0], clips[1][0]])) == 2
