#!/usr/bin/env python
"""Pose windows on the device against the host path they stand in for, end to end on the host clock (every call
here ends in a stream synchronise):

  offline   ``score_poselift_many(model, tree)`` (one upload of the poses, the window launch, the score launch) against the host path,
            ``windows_from_poselift`` + ``model.score`` per video, on the same synthetic tree of ``--sizes`` windows;
  live      one tick of ``MultiStreamScorer`` over N cameras against N ``StreamScorer``s fed the same rows (``--cameras``, about
            ``--tracks`` tracks each, their cut positions staggered so that every tick completes windows).

The two sides alternate call by call in one process; after warm-up each cell records the median of ``--reps`` calls with min and max.
The host side is the comparison base: its own spread (max - min over median) is printed beside every ratio.  ``--profile-n N`` instead
runs ``score_poses`` on N windows a few times and nothing else, for a kernel trace taken around this script.
Prints one JSON line per cell; ``--out`` also appends them to a file.

    python tools/pose_windows_bench.py --out profiles/pose_windows_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PERSONS, FRAMES = 8, 54                     # one synthetic video: 8 persons x 54 frames = 8 windows each at seq_len 12, stride 6


def synthetic_tree(n_windows: int, seed: int = 0):
    """-> a list of PoseLift dicts that cut into ``n_windows`` windows (64 per video), float32 (17, 3) keypoints in pixels"""
    rng = np.random.default_rng(seed)
    tree = []
    for _ in range(max(1, n_windows // (PERSONS * 8))):
        k = rng.uniform(1, 640, (FRAMES, PERSONS, 17, 3)).astype(np.float32)
        k[rng.random((FRAMES, PERSONS, 17)) < 0.05, :2] = 0
        box = np.zeros(4, np.float32)
        tree.append({f: {p: [box, k[f, p]] for p in range(PERSONS)} for f in range(FRAMES)})
    return tree


def timed_pair(fn_a, fn_b, reps, warmup):
    for _ in range(warmup):
        fn_a()
        fn_b()
    sa, sb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); fn_a(); t1 = time.perf_counter(); fn_b(); t2 = time.perf_counter()
        sa.append((t1 - t0) * 1e3)
        sb.append((t2 - t1) * 1e3)
    return np.asarray(sa), np.asarray(sb)


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max())}


def cell(kind, key, base, new, extra):
    b, d = stats(base), stats(new)
    row = {"bench": "pose_windows", "kind": kind, **key, "host_ms": b, "device_ms": d, "speedup": b["median"] / d["median"],
           "host_spread": (b["max"] - b["min"]) / b["median"], "device_not_slower": d["median"] <= b["median"] + (b["max"] - b["min"]), **extra}
    return row


def offline(model, SF, n, reps, warmup):
    tree = synthetic_tree(n)
    host = lambda: [SF.score_poselift(model, d) for d in tree]
    dev = lambda: SF.score_poselift_many(model, tree, on_device=True)
    same = all(i == j and np.array_equal(a.view(np.uint32), b.view(np.uint32)) for (a, i), (b, j) in zip(host(), dev()))
    windows = sum(len(i) for _, i in dev())
    t0 = time.perf_counter()
    packed = [SF.pack_poselift(d, model.seq_len) for d in tree]
    pack_ms = (time.perf_counter() - t0) * 1e3
    poses = np.concatenate([p[0] for p in packed])
    starts = np.concatenate([p[1] + o for p, o in zip(packed, np.cumsum([0] + [len(p[0]) for p in packed]))]).astype(np.int32)
    t0 = time.perf_counter()
    model.score_poses(poses, starts)
    call_ms = (time.perf_counter() - t0) * 1e3
    base, new = timed_pair(host, dev, reps, warmup)
    return cell("offline", {"windows": windows, "videos": len(tree)}, base, new,
                {"same_bits": bool(same), "reps": reps, "pack_ms_once": pack_ms, "score_poses_ms_once": call_ms, "pose_bytes": int(poses.nbytes),
                 "window_bytes": int(windows * 2 * model.seq_len * model.num_keypoints * 4)})


def live(model, SF, n_cams, tracks, reps, warmup):
    rng = np.random.default_rng(n_cams)
    n_ticks = 12 + 6 + warmup + reps
    kp = rng.uniform(1, 640, (n_ticks, n_cams, tracks, 17, 3)).astype(np.float32)
    rows = np.zeros((tracks, 5), np.float32)
    rows[:, 4] = np.arange(tracks)
    multi, singles = SF.MultiStreamScorer(model, n_cams), [SF.StreamScorer(model) for _ in range(n_cams)]

    def cams_of(t):                                             # track i enters at tick i % 6: every later tick completes windows
        keep = np.arange(tracks) % 6 <= t
        return [(rows[keep], kp[t, c][keep]) for c in range(n_cams)]

    sa, sb, same, done = [], [], True, 0
    for t in range(n_ticks):
        cams = cams_of(t)
        t0 = time.perf_counter()
        want = [s.update(t, *c) for s, c in zip(singles, cams)]
        t1 = time.perf_counter()
        got = multi.update(t, cams)
        t2 = time.perf_counter()
        same &= got == want
        if t >= n_ticks - reps:
            sa.append((t1 - t0) * 1e3)
            sb.append((t2 - t1) * 1e3)
            done += sum(len(w) for w in want)
    return cell("live", {"cameras": n_cams, "tracks": tracks}, np.asarray(sa), np.asarray(sb),
                {"same_floats": bool(same), "reps": reps, "windows_per_tick": done / reps})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,4096,65536")
    ap.add_argument("--cameras", default="1,4,16")
    ap.add_argument("--tracks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-n", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from tools import synth_shopformer as R
    from cvsd_amd import Shopformer
    from cvsd_amd import shopformer as SF
    cfg, sd, _ = R.fixture_model(R.load_fixture(), "default")
    model = Shopformer.from_state_dict(sd, cfg, device=0)
    if args.profile_n:
        rng = np.random.default_rng(0)
        poses = rng.uniform(1, 640, (args.profile_n * 6 + 6, 17, 2)).astype(np.float32)
        starts = (np.arange(args.profile_n) * 6).astype(np.int32)
        for _ in range(8):
            model.score_poses(poses, starts)
        print(json.dumps({"bench": "pose_windows", "kind": "profile", "windows": args.profile_n, "pose_bytes": int(poses.nbytes),
                          "window_bytes": int(args.profile_n * 2 * model.seq_len * model.num_keypoints * 4)}))
        return
    lines = []
    for n in (int(s) for s in args.sizes.split(",") if s):
        lines.append(json.dumps(offline(model, SF, n, args.reps, args.warmup)))
        print(lines[-1], flush=True)
    for c in (int(s) for s in args.cameras.split(",") if s):
        lines.append(json.dumps(live(model, SF, c, args.tracks, args.reps, args.warmup)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write("".join(line + "\n" for line in lines))


if __name__ == "__main__":
    main()
