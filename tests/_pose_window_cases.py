"""TEST INFRASTRUCTURE shared by test_pose_windows.py (host twin) and test_gpu_pose_windows.py (kernel): seeded edge windows, the
fixture clip as a PoseLift dict, a many-camera tick scenario, and stub models.  Reads only the repository."""
import os

import numpy as np

from _poselift_windows import unflatten
from cvsd_amd import ops
from cvsd_amd import shopformer as SF

GOLD = os.path.join(os.path.dirname(__file__), "golden")
MODES = ("plain", "all_zero", "one_valid", "sparse40", "left_missing", "right_missing", "both_missing", "tiny_shoulders", "zero_y",
         "huge")
# (V_src, V, neck): what the offline loaders produce, and a detector that delivers fewer joints than the model reads
CONFIGS = ((17, 17, False), (17, 18, True), (17, 18, False), (12, 17, False))


def edge_window(mode, T, v_src, dtype, rng):
    """one window as the list of T keypoint arrays (v_src, 3) a loader would hand to ``_window_tensor``"""
    k = rng.uniform(1.0, 640.0, (T, v_src, 3))
    if mode == "all_zero":
        k[:, :, :2] = 0
    elif mode == "one_valid":
        keep = k[T // 2, 3, :2].copy()
        k[:, :, :2] = 0
        k[T // 2, 3, :2] = keep
    elif mode == "sparse40":
        k[rng.random((T, v_src)) < 0.4, :2] = 0
    elif mode == "left_missing":
        k[:, 5, :2] = 0
    elif mode == "right_missing":
        k[::2, 6, :2] = 0
    elif mode == "both_missing":
        k[:, 5:7, :2] = 0
    elif mode == "tiny_shoulders":                                   # np.allclose(., 0) calls +-1e-9 missing, yet the joint is "valid" (!= 0)
        k[:, 5:7, :2] = rng.choice([1e-9, -1e-9], (T, 2, 2))
        k[1, 5, :2] = (1e-7, 0)                                      # above the 1e-8 line: a shoulder that counts
    elif mode == "zero_y":
        k[:, :, 1] = 0
    elif mode == "huge":                                             # sums and offsets overflow: inf / inf -> NaN -> np.nan_to_num's 0
        k[:, :5, :2] = 0.9 * float(np.finfo(dtype).max)
        k[3, 2, 0] = -0.9 * float(np.finfo(dtype).max)
    return [np.ascontiguousarray(k[t], dtype) for t in range(T)]


def edge_set(T, v_src, dtype, per_mode=3, seed=0):
    rng = np.random.default_rng([seed, T, v_src])
    return [edge_window(m, T, v_src, dtype, rng) for m in MODES for _ in range(per_mode)]


def flatten(windows):
    """windows (lists of (v_src, 3) arrays) -> (poses [n * T, v_src, 2], starts): the kernel's input for the same windows"""
    T = len(windows[0])
    return np.stack([k[:, :2] for w in windows for k in w]), np.arange(len(windows), dtype=np.int32) * T


def host_windows(windows, V, neck):
    with np.errstate(all="ignore"):                                  # the "huge" windows overflow on purpose
        return np.stack([SF._window_tensor(w, V, neck) for w in windows])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def fixture_clip():
    pf = np.load(os.path.join(GOLD, "poselift_fixture.npz"))
    data = unflatten(pf["frame_keys"], pf["row_frame"], pf["row_pid"], pf["row_bbox"], pf["row_kpts"])
    return pf, data, int(pf["meta"][6]), int(pf["meta"][7])


def gap_dict():
    """the clip of test_shopformer.py::test_gap_rule_and_nan_poses: one person, 12 frames, an 18-frame hole, 12 frames"""
    k = np.ones((17, 3), np.float32)
    k[:, 0] = np.arange(17)
    return {f: {1: [np.zeros(4, np.float32), k * (1 + 0.01 * f)]} for f in list(range(12)) + [30] + list(range(31, 42))}


def camera_ticks(data, n_ticks=40, n_cameras=3):
    """-> [(frame numbers, cams)] for ``MultiStreamScorer.update``: every camera plays the clip (twice over, the ids go on), camera c
    numbers its frames from 100 c, camera 1 has no frame on every seventh tick, camera 2 loses one id for 9 ticks (> max_gap)"""
    frames = sorted(data)
    lost = next(iter(data[frames[0]]))
    ticks = []
    for t in range(n_ticks):
        people = data[frames[t % len(frames)]]
        cams = []
        for c in range(n_cameras):
            if c == 1 and t % 7 == 3:
                cams.append(None)
                continue
            ids = [p for p in people if not (c == 2 and p == lost and 10 <= t < 19)]
            rows = np.asarray([[people[p][0][0], people[p][0][1], people[p][0][0] + people[p][0][2], people[p][0][1] + people[p][0][3], p]
                               for p in ids], np.float32).reshape(-1, 5)
            kpts = np.asarray([people[p][1] for p in ids], np.float32).reshape(-1, 17, 3) * np.float32(1 + 0.01 * c)
            cams.append((rows, kpts))
        ticks.append(([t + 100 * c for c in range(n_cameras)], cams))
    return ticks


def play(model, ticks, n_cameras=3):
    """-> (what MultiStreamScorer returned per tick, what one StreamScorer per camera returned for the same sequence)"""
    multi, singles = SF.MultiStreamScorer(model, n_cameras), [SF.StreamScorer(model) for _ in range(n_cameras)]
    got, want = [], []
    for frames, cams in ticks:
        got.append(multi.update(frames, cams))
        want.append([s.update(f, *c) if c is not None else [] for s, f, c in zip(singles, frames, cams)])
    return got, want


class StubModel:
    """the ``_StubModel`` idea of test_shopformer.py: a score that depends on every bit of the window, no ``score_poses``"""
    seq_len, num_keypoints, neck = 12, 17, False

    def score(self, w):
        return np.asarray(w, np.float64).reshape(len(w), 2 * self.seq_len * self.num_keypoints).sum(1).astype(np.float32)


class TwinModel(StubModel):
    """the stub with ``score_poses`` on the kernel's host twin: the device branch of the Python layer without a GPU"""

    def __init__(self, num_keypoints=17, neck=False):
        self.num_keypoints, self.neck, self.pose_calls, self.score_calls = num_keypoints, neck, 0, 0

    def score(self, w):
        self.score_calls += 1
        return StubModel.score(self, w)

    def score_poses(self, poses, starts, reduction="mean"):
        self.pose_calls += 1
        return StubModel.score(self, ops.pose_windows(poses, starts, self.seq_len, self.num_keypoints, neck=self.neck, device=-1))
