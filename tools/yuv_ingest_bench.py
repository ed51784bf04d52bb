"""What the NV12 ingest costs or saves against the BGR call on the same content.

    python tools/yuv_ingest_bench.py [--model yolov8n-pose] [--reps 20] [--warmup 3] [--out profiles/yuv_ingest_bench.json]

For 640x640 and 240x320 frames at batch 1, 8 and 64, the BGR call and the NV12 call alternate call by call in one process:
  host     frames from host memory (the comparison baseline is the BGR host-frame call): wall ms per call, median of --reps with
           [min, max]; NV12 uploads 1.5 bytes per pixel instead of 3 and adds one conversion launch per chunk
  device   the same with BGR frames / NV12 planes already in HBM
  preprocess_ms   the engine's letterbox_ms span of one profiled call of each kind: letterbox alone for BGR, conversion + letterbox for
           NV12 (640x640 needs no letterbox: there the span is the conversion launch)
Prints one JSON object and, with --out, writes it to that file.
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

SIZES = [(640, 640), (240, 320)]
BATCHES = [1, 8, 64]


def _nv12_planes(bgr):
    """float BT.601 limited range, 2x2 chroma averaging -> (y [H, W], uv [H/2, W]); only makes plausible content"""
    f = bgr.astype(np.float64)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    h, w = b.shape
    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    pool = lambda a: a.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    u, v = pool(128 - 0.148 * r - 0.291 * g + 0.439 * b), pool(128 + 0.439 * r - 0.368 * g - 0.071 * b)
    return q(16 + 0.257 * r + 0.504 * g + 0.098 * b), q(np.stack([u, v], -1).reshape(h // 2, w))


def _alternate(fa, fb, reps, warmup):
    """fa and fb in turn, call by call -> ({median, min, max} of fa, of fb) in ms"""
    for _ in range(warmup):
        fa(); fb()
    ta, tb = [], []
    for _ in range(reps):
        for f, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e3)
    stat = lambda ts: {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}
    return stat(ta), stat(tb)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="yolov8n-pose")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from cvsd_amd import YOLO, YUVFrame
    from tools import synth
    _, sd = synth.synthetic_checkpoint(args.model, seed=0)
    m = YOLO.from_state_dict(args.model, sd)
    kw = dict(conf=0.25, imgsz=args.imgsz)
    out = {"model": args.model, "imgsz": args.imgsz, "reps": args.reps, "cases": []}
    for h, w in SIZES:
        src = synth.synthetic_frames(8, h, w, seed=1)
        frames8 = [YUVFrame(y, uv=uv) for y, uv in map(_nv12_planes, src)]
        bgr8 = [f.to_bgr(-1) for f in frames8]                                    # the same content: what the conversion makes of the planes
        for n in BATCHES:
            nv12 = [frames8[i % 8] for i in range(n)]
            bgr = np.stack([bgr8[i % 8] for i in range(n)])
            bgr_b, yuv_b = m._as_batch(bgr)[0], m._as_batch(nv12)[0]
            same = all(np.array_equal(a, b) for a, b in zip(m.detect_rows(bgr_b, **kw)[0], m.detect_rows(yuv_b, **kw)[0]))
            case = {"height": h, "width": w, "batch": n, "rows_identical": bool(same)}
            case["host_bgr"], case["host_nv12"] = _alternate(lambda: m.detect_rows(bgr_b, **kw), lambda: m.detect_rows(yuv_b, **kw), args.reps, args.warmup)
            bgr_d = torch.from_numpy(bgr).cuda()
            nv12_d = m._as_batch([YUVFrame(torch.from_numpy(f.y).cuda(), uv=torch.from_numpy(f.uv).cuda())
                                  for f in nv12])[0]
            case["device_bgr"], case["device_nv12"] = _alternate(lambda: m.detect_rows(bgr_d, **kw), lambda: m.detect_rows(nv12_d, **kw), args.reps,
                                                                 args.warmup)
            m.set_profiling(True)
            m.detect_rows(bgr_b, **kw)
            case["preprocess_ms_bgr"] = m.last_timing()["letterbox_ms"]
            m.detect_rows(yuv_b, **kw)
            t = m.last_timing()
            case["preprocess_ms_nv12"], case["device_total_ms_nv12"] = t["letterbox_ms"], t["total_ms"]
            m.set_profiling(False)
            case["host_nv12_over_bgr"] = case["host_nv12"]["median_ms"] / case["host_bgr"]["median_ms"]
            case["device_nv12_over_bgr"] = case["device_nv12"]["median_ms"] / case["device_bgr"]["median_ms"]
            out["cases"].append(case)
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
