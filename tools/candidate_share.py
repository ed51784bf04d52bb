"""Share of anchors that reach NMS, per head level, on the benchmark's frames (CPU, torch oracle).

    python -m tools.candidate_share [--model yolov8n] [--conf 0.25] [--frames 16] [--seed 1000]

p = share of anchors whose best class score clears conf (the candidates `nms_collect` would select);
q = share of positions in the 3x3 dilation of that set (what a gathered first box conv would have to compute).
Printed for tools.synth.synthetic_frames(frames, 640, 640, seed) and for the +-24 uniform-noise variants that
bench.py:make_frames derives from them (same distribution; bench.py draws its noise with the GPU generator).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def shares(model, frames: np.ndarray, conf: float, size: int):
    from oracle import yolo_oracle as yo
    out = []
    levels = [(size // s) for s in (8, 16, 32)]
    for f in frames:
        pred = model.forward(yo.preprocess([f], size))[0]              # [4 + nc (+nk), A]
        best = pred[4:4 + model.nc].amax(0)
        row, off = [], 0
        for n in levels:
            m = (best[off:off + n * n] > conf).view(1, 1, n, n).float()
            d = F.max_pool2d(m, 3, 1, 1)
            row.append((float(m.mean()), float(d.mean())))
            off += n * n
        out.append(row)
    return np.asarray(out)                                               # [frames, 3, 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="yolov8n")
    ap.add_argument("--conf", type=float, default=0.25)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--size", type=int, default=640)
    a = ap.parse_args()
    from oracle import yolo_oracle as yo
    from tools import synth
    _, sd = synth.synthetic_checkpoint(a.model, seed=0)
    model = yo.OracleModel(a.model, sd)
    base = synth.synthetic_frames(a.frames, a.size, a.size, seed=a.seed)
    rng = np.random.default_rng(a.seed)
    noisy = np.clip(base.astype(np.int16) + rng.integers(-24, 25, size=base.shape), 0, 255).astype(np.uint8)
    for name, fr in (("base", base), ("noise+-24", noisy)):
        s = shares(model, fr, a.conf, a.size)
        for li, n in enumerate((a.size // 8, a.size // 16, a.size // 32)):
            p, q = s[:, li, 0], s[:, li, 1]
            print(f"{name:10s} {n}x{n}: p mean {p.mean():.4f} max {p.max():.4f}   q mean {q.mean():.4f} max {q.max():.4f}   q/p {q.mean() / max(p.mean(), 1e-9):.2f}")


if __name__ == "__main__":
    main()
