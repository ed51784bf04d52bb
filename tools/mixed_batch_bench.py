"""Cost of one predict call over frames of different sizes (several cameras) against one call per size.

    python tools/mixed_batch_bench.py [--model yolov8n-pose] [--reps 20] [--warmup 3]

Prints one JSON object:
  mixed64       64 frames, 16 each of 240x320, 720x1280, 1080x1920 and 640x640, as ONE call (square 640 x 640 canvas for all):
                wall ms per call, the engine's device ms and its letterbox ms (profiling run)
  split64       the same 64 frames as four calls of 16, one per shape (rect letterbox per shape): wall ms for the four
  cams4_mixed   4 cameras x 1 frame (one frame of each shape) as one mixed call: wall ms
  cams4_split   the same 4 frames as four batch-1 calls: wall ms for the four
Host frames throughout (decoded frames arrive on the host); the median over --reps calls is reported.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(240, 320), (720, 1280), (1080, 1920), (640, 640)]


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="yolov8n-pose")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--imgsz", type=int, default=640)
    args = ap.parse_args()
    from cvsd_amd import YOLO
    from tools import synth
    _, sd = synth.synthetic_checkpoint(args.model, seed=0)
    m = YOLO.from_state_dict(args.model, sd)
    per_shape = [list(synth.synthetic_frames(16, h, w, seed=i)) for i, (h, w) in enumerate(SHAPES)]
    mixed = [f for i in range(16) for f in (per_shape[0][i], per_shape[1][i], per_shape[2][i], per_shape[3][i])]   # cameras interleaved
    stacks = [np.stack(p) for p in per_shape]
    kw = dict(conf=0.25, imgsz=args.imgsz)
    out = {"model": args.model, "imgsz": args.imgsz, "reps": args.reps}

    ragged = m._as_batch(mixed)[0]
    out["mixed64_ms"] = _median_ms(lambda: m.detect_rows(ragged, **kw), args.reps, args.warmup)
    out["split64_ms"] = _median_ms(lambda: [m.detect_rows(s, **kw) for s in stacks], args.reps, args.warmup)
    m.set_profiling(True)
    m.detect_rows(ragged, **kw)
    t = m.last_timing()
    out["mixed64_device_ms"], out["mixed64_letterbox_ms"] = t["total_ms"], t["letterbox_ms"]
    lb = 0.0
    for s in stacks:
        m.detect_rows(s, **kw)
        lb += m.last_timing()["letterbox_ms"]
    out["split64_letterbox_ms"] = lb
    m.set_profiling(False)

    cams = [p[0] for p in per_shape]
    cams_ragged = m._as_batch(cams)[0]
    singles = [c[None] for c in cams]
    out["cams4_mixed_ms"] = _median_ms(lambda: m.detect_rows(cams_ragged, **kw), args.reps, args.warmup)
    out["cams4_split_ms"] = _median_ms(lambda: [m.detect_rows(s, **kw) for s in singles], args.reps, args.warmup)
    out["mixed64_frames_per_s"] = 64e3 / out["mixed64_ms"]
    out["split64_frames_per_s"] = 64e3 / out["split64_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
