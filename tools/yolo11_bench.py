"""TEST/BENCH INFRASTRUCTURE -- yolo11n next to yolov8n, measured the way bench.py's timed region measures: distinct frames resident
in HBM (bench.make_frames), one ``_infer_rows`` call per step (letterbox .. NMS, rows back on the host), frames/s over `steps`
steps after `warmup`.  Prints one JSON line per (model, batch).

    python tools/yolo11_bench.py [--batches 1 512] [--steps 20] [--warmup 5] [--models yolo11n yolov8n]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(name: str, batch: int, size: int, steps: int, warmup: int) -> dict:
    import torch
    from bench import make_frames
    from cvsd_amd import YOLO
    from cvsd_amd.weights import build_from_state_dict
    from tools import synth
    _, sd = synth.synthetic_checkpoint(name, seed=0)
    model = YOLO(build_from_state_dict(name, sd), device=torch.cuda.current_device(), batch_chunk=batch)
    frames, _ = make_frames(batch, size, seed=2000 + batch)
    for _ in range(warmup):
        model._infer_rows(frames, 0.25, 0.7, None, 300, size)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        model._infer_rows(frames, 0.25, 0.7, None, 300, size)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"model": name, "batch": batch, "size": size, "frames_per_s": round(batch * steps / dt, 1),
            "ms_per_step": round(dt / steps * 1e3, 3), "plan_source": model.plan_info()["plan_source"]}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--models", nargs="+", default=["yolo11n", "yolov8n"])
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 512])
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args(argv)
    for b in a.batches:
        for m in a.models:
            print(json.dumps(measure(m, b, a.size, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
