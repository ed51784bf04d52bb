"""Several cameras stepped together on the host (``gmc.MultiGMC(device=None)``, ``mi355_gmc_multi_*`` with device -1) against one
``gmc.GMC(device=None)`` object per camera fed the same frames: the same warps, previous planes and corner lists, bit for bit -- with
cameras of different sizes, cameras that skip ticks, a reset and a size change mid-stream; argument checks; the supplied-warp form of
``BYTETracker.update`` that ``YOLO.track_cameras`` steps its trackers with.  No GPU."""
import numpy as np
import pytest

from cvsd_amd import gmc
from cvsd_amd.gmc import GMC, MultiGMC
from tools import synth

SIZES = [(240, 320), (480, 640), (90, 160)]


def _clips(n, sizes=SIZES):
    return [synth.synthetic_clip(n, h, w, seed=5 + i) for i, (h, w) in enumerate(sizes)]


def _same_state(multi, singles):
    for i, s in enumerate(singles):
        a, b = multi.prev_frame(i), s.prev_frame
        assert (a is None) == (b is None)
        if a is not None:
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(multi.prev_points(i), s.prev_points)


def test_three_cameras_of_different_sizes_equal_three_single_objects():
    clips = _clips(14)
    multi, singles = MultiGMC(3, device=None), [GMC(device=None) for _ in range(3)]
    moved = 0
    for t in range(14):
        frames = [c[t] for c in clips]
        H = multi.apply(frames)
        assert H.shape == (3, 2, 3) and H.dtype == np.float64
        for i, s in enumerate(singles):
            np.testing.assert_array_equal(H[i], s.apply(frames[i]))
        _same_state(multi, singles)
        moved += int(np.abs(H - np.eye(2, 3)).max() > 0.05)
        if t == 0:
            np.testing.assert_array_equal(H, np.tile(np.eye(2, 3), (3, 1, 1)))       # every camera's first frame
    assert moved >= 4                                                               # the clips pan: the equality is not one of identities
    assert len(multi.prev_points(0)) > 50


def test_begin_then_apply_of_the_same_list_collects_the_enqueued_tick():
    clips = _clips(4)
    multi, ref = MultiGMC(3), MultiGMC(3)
    for t in range(4):
        frames = [c[t] for c in clips]
        multi.begin(frames)
        assert multi.pending_device_frames() is None                                # host object: nothing on a device
        np.testing.assert_array_equal(multi.apply(frames), ref.apply([c[t] for c in clips]))


def test_absent_cameras_keep_their_state_and_get_the_identity():
    clips = _clips(13)
    multi, singles = MultiGMC(3), [GMC() for _ in range(3)]
    for t in range(13):
        frames = [c[t] for c in clips]
        if t % 3 == 1:
            frames[1] = None
        if t in (4, 5):
            frames[2] = None
        if t == 7:
            frames = [None, None, None]
        H = multi.apply(frames)
        for i, s in enumerate(singles):
            if frames[i] is None:
                np.testing.assert_array_equal(H[i], np.eye(2, 3))
            else:
                np.testing.assert_array_equal(H[i], s.apply(frames[i]))
        _same_state(multi, singles)


def test_reset_of_one_camera_mid_stream():
    clips = _clips(12)
    multi, singles = MultiGMC(3), [GMC() for _ in range(3)]
    for t in range(12):
        if t == 5:
            multi.reset(camera=1)
            singles[1].reset()
            assert multi.prev_frame(1) is None and multi.prev_frame(0) is not None
        if t == 9:
            multi.reset()
            for s in singles:
                s.reset()
        frames = [c[t] for c in clips]
        H = multi.apply(frames)
        for i, s in enumerate(singles):
            np.testing.assert_array_equal(H[i], s.apply(frames[i]))
        if t in (5, 9):
            np.testing.assert_array_equal(H[1], np.eye(2, 3))
        _same_state(multi, singles)


def test_a_camera_that_changes_size_mid_stream_restarts_like_a_single_object():
    clips = _clips(12)
    other = synth.synthetic_clip(12, 200, 300, seed=21)
    multi, singles = MultiGMC(3), [GMC() for _ in range(3)]
    for t in range(12):
        frames = [c[t] for c in clips]
        if 4 <= t < 8:
            frames[0] = other[t]                                                    # smaller from tick 4, back to the first size at 8
        H = multi.apply(frames)
        for i, s in enumerate(singles):
            np.testing.assert_array_equal(H[i], s.apply(frames[i]))
        if t in (4, 8):
            np.testing.assert_array_equal(H[0], np.eye(2, 3))
        _same_state(multi, singles)
    assert multi.prev_frame(0).shape == (120, 160)


def test_method_none_gives_identities_and_creates_nothing():
    m = MultiGMC(2, method=None)
    f = synth.synthetic_clip(1, 64, 96, seed=1)[0]
    np.testing.assert_array_equal(m.apply([f, None]), np.tile(np.eye(2, 3), (2, 1, 1)))
    m.begin([f, f])
    assert m._h is None and m.pending_device_frames() is None and m.prev_frame(0) is None


def test_bad_arguments():
    m = MultiGMC(3)
    f = synth.synthetic_clip(1, 64, 96, seed=1)[0]
    with pytest.raises(ValueError):
        m.apply([f, f])                                                             # wrong list length
    with pytest.raises(ValueError):
        m.apply([f, f[:, :, 0], f])                                                 # a 2-D frame
    with pytest.raises(ValueError):
        m.begin([f, f, f, f])
    with pytest.raises(ValueError):
        m.reset(camera=3)
    with pytest.raises(ValueError):
        MultiGMC(0)
    with pytest.raises(ValueError):
        MultiGMC(2, method="orb")
    # the checks left the object usable
    np.testing.assert_array_equal(m.apply([f, None, f])[0], np.eye(2, 3))


def test_c_abi_call_order_is_checked():
    import ctypes as C
    from cvsd_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.mi355_gmc_multi_create(-1, 0, C.byref(h)) == -1
    assert lib.mi355_gmc_multi_create(-1, 2, C.byref(h)) == 0
    H = np.zeros((2, 6))
    assert lib.mi355_gmc_multi_finish(h, H.ctypes.data) == -1                       # nothing begun
    f = np.ascontiguousarray(synth.synthetic_clip(1, 64, 96, seed=1)[0])
    ptrs = (C.c_void_p * 2)(f.ctypes.data, None)
    hs, ws = (C.c_int * 2)(64, 0), (C.c_int * 2)(96, 0)
    assert lib.mi355_gmc_multi_begin(h, ptrs, hs, ws, 2) == 0
    assert lib.mi355_gmc_multi_begin(h, ptrs, hs, ws, 2) == -1                      # one tick at a time
    assert lib.mi355_gmc_multi_frames(h, (C.c_void_p * 2)()) == -1                  # host object: no device frames
    assert lib.mi355_gmc_multi_finish(h, H.ctypes.data) == 0
    assert lib.mi355_gmc_multi_finish(h, H.ctypes.data) == -1                       # a tick is collected once
    np.testing.assert_array_equal(H[0], [1, 0, 0, 0, 1, 0])
    np.testing.assert_array_equal(H[1], 0)                                          # absent camera: untouched
    bad = (C.c_int * 2)(0, 0)
    assert lib.mi355_gmc_multi_begin(h, ptrs, bad, ws, 2) == -1
    lib.mi355_gmc_multi_destroy(h)


def test_track_cameras_needs_a_gpu_like_every_other_entry_point():
    """no fallback: without a visible GPU the engine cannot be created (Mi355Error, as for predict / track), and the motion compensation
    of the call raises RuntimeError as GMC(device=k) does (tests/test_gmc.py); the method exists and checks its arguments"""
    import torch
    from cvsd_amd import YOLO
    from cvsd_amd._lib import Mi355Error
    assert callable(YOLO.track_cameras)
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU")
    _, sd = synth.synthetic_checkpoint("yolov8n", seed=0)
    with pytest.raises(Mi355Error, match="device"):
        YOLO.from_state_dict("yolov8n", sd, device=0)
    f = synth.synthetic_clip(1, 64, 96, seed=1)[0]
    m = MultiGMC(2, device=0)
    with pytest.raises(RuntimeError, match="mi355_gmc_multi"):
        m.apply([f, None])
    m.reset()


def test_a_tick_that_was_begun_and_never_collected_is_not_taken_for_the_next():
    """what track_cameras relies on when its detector pass raises: begin() for another list discards the stale tick and starts over"""
    clips = _clips(4)
    multi, ref = MultiGMC(3), MultiGMC(3)
    for t in range(2):
        np.testing.assert_array_equal(multi.apply([c[t] for c in clips]), ref.apply([c[t] for c in clips]))
    multi.begin([c[2] for c in clips])                                              # ... and the caller never comes back for it
    frames = [clips[0][3], None, clips[2][3]]
    multi.begin(frames)
    H = multi.apply(frames)
    np.testing.assert_array_equal(H, np.tile(np.eye(2, 3), (3, 1, 1)))              # started over, like GMC.apply with a stale step
    assert multi.prev_frame(0).shape == (120, 160) and multi.prev_frame(1) is None


def test_tracker_stepped_with_a_supplied_warp_equals_the_image_path():
    from cvsd_amd.tracker import BYTETracker
    clip = synth.synthetic_clip(10, 240, 320, seed=9)
    people = np.array([[60, 60, 100, 180], [150, 40, 190, 170], [240, 80, 275, 200]], np.float32)
    by_image, by_warp, g = BYTETracker(), BYTETracker(), GMC()
    ids = set()
    for k, frame in enumerate(clip):
        shift = np.array([k // 2, 0, k // 2, 0], np.float32)
        det = np.concatenate([people - shift, np.full((3, 1), 0.9, np.float32), np.zeros((3, 1), np.float32)], axis=1).astype(np.float32)
        if k == 6:
            det = det[:0]                                                           # an empty frame still steps
        a = by_image.update(det, frame)
        b = by_warp.update(det, warp=g.apply(frame))
        np.testing.assert_array_equal(a, b)
        ids.update(a[:, 4].astype(int).tolist())
    assert ids == {1, 2, 3}
    assert by_warp.gmc.prev_frame is None                                           # its own motion compensation never ran
