"""What the motion gate of ``YOLO.track_cameras`` buys and costs: 16 cameras, half 480x640 and half 1080x1920, of which
0 %, 50 % or 90 % show an unchanged scene (the same frame under +-1 of sensor noise) while the others pan 2 px per tick.

  * ticks/s of the gated call (``motion_gate=True``) against the ungated call -- same model object class, same frames, same process, the
    two sides alternating ``--repeats`` times; median, min and max over the repeats.  The ungated side is the call as it was before the
    gate existed: compare it with the same figure of the parent commit to see that nothing moved.
  * the gate alone on frames that already sit on the GPU: time of one ``MotionGate.update`` (host clock around a call that ends in a
    stream wait: launch + kernel + one small copy back) for 16 and for 64 cameras, the bytes it reads, and the MARGINAL rate
    (bytes of the extra 48 cameras / extra time), which leaves the fixed cost of a call out.  Against 8 TB/s (HBM3E peak; about 6.3
    achievable) -- frames of this size may be served by the 256 MiB Infinity Cache when they were written just before.

    python tools/motion_gate_bench.py --ticks 40 --repeats 5

One JSON line per static share, one for the gate alone."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(480, 640), (1080, 1920)]
HBM_PEAK = 8.0e12


class Camera:
    """one camera: a textured scene; a moving camera pans 2 px per tick, a static one repeats its first view under +-1 of noise"""
    def __init__(self, h, w, ticks, static, rng):
        base = rng.integers(0, 256, size=(h // 8 + 2, (w + 2 * ticks) // 8 + 2, 3), dtype=np.uint8)
        self.big, self.w, self.static = np.kron(base, np.ones((8, 8, 1), np.uint8))[:h, :w + 2 * ticks], w, static
        self.rng = np.random.default_rng(int(rng.integers(1 << 30)))

    def __getitem__(self, t):
        if not self.static:
            return np.ascontiguousarray(self.big[:, 2 * t:2 * t + self.w])
        f = self.big[:, :self.w].astype(np.int16) + self.rng.integers(-1, 2, size=(self.big.shape[0], self.w, 3), dtype=np.int16)
        return np.clip(f, 0, 255).astype(np.uint8)


def make_cameras(n, ticks, static_share):
    rng = np.random.default_rng(0)
    n_static = int(round(static_share * n))
    # static cameras are spread over both sizes: camera i is static when it is among the first n_static of the order 0, 1, 2, ...
    return [Camera(*SIZES[i % 2], ticks, i < n_static, rng) for i in range(n)]


def run(model, clips, warmup, gate):
    spent, skipped = 0.0, 0
    kw = {"motion_gate": True} if gate else {}
    for t, frames in enumerate(clips):
        t0 = time.perf_counter()
        res = model.track_cameras(frames, persist=t > 0, **kw)
        if t >= warmup:
            spent += time.perf_counter() - t0
            skipped += sum(bool(r.motion and r.motion["skipped"]) for r in res if r is not None)
    return (len(clips) - warmup) / spent, skipped / ((len(clips) - warmup) * len(clips[0]))


def gate_alone(device, n, reps):
    import torch
    from cvsd_amd import MotionGate
    rng = np.random.default_rng(1)
    frames = [torch.from_numpy(rng.integers(0, 256, (*SIZES[i % 2], 3), dtype=np.uint8)).to(f"cuda:{device}") for i in range(n)]
    nbytes = sum(int(f.numel()) for f in frames)
    g = MotionGate(n, device=device, max_skip=None)
    for _ in range(5):
        g.update(frames)
    torch.cuda.synchronize(device)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        g.update(frames)
        ts.append(time.perf_counter() - t0)
    return nbytes, float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=16)
    ap.add_argument("--static", type=float, nargs="+", default=[0.0, 0.5, 0.9])
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--model", default="yolov8n-pose")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--gate-only", action="store_true", help="the gate alone; no model is built")
    a = ap.parse_args()
    from cvsd_amd import YOLO
    from tools import synth
    model = None
    if not a.gate_only:
        _, sd = synth.synthetic_checkpoint(a.model, seed=0)
        model = YOLO.from_state_dict(a.model, sd, device=a.device)
    for share in ([] if a.gate_only else a.static):
        cams = make_cameras(a.cameras, a.ticks, share)
        clips = [[c[t] for c in cams] for t in range(a.ticks)]   # building the frames is not part of a tick
        tps = {"ungated": [], "gated": []}
        skipped = 0.0
        for _ in range(a.repeats):                               # the sides alternate
            tps["ungated"].append(run(model, clips, a.warmup, False)[0])
            r, skipped = run(model, clips, a.warmup, True)
            tps["gated"].append(r)
        row = {"static_share": share, "cameras": a.cameras, "model": a.model, "ticks": a.ticks, "repeats": a.repeats,
               "skipped_share_measured": round(skipped, 3)}
        for k, v in tps.items():
            row[f"{k}_ticks_per_s_median"] = round(float(np.median(v)), 2)
            row[f"{k}_ticks_per_s_min"], row[f"{k}_ticks_per_s_max"] = round(float(min(v)), 2), round(float(max(v)), 2)
        row["gated_over_ungated"] = round(row["gated_ticks_per_s_median"] / row["ungated_ticks_per_s_median"], 3)
        print(json.dumps(row), flush=True)
    b16, t16, m16 = gate_alone(a.device, 16, 200)
    b64, t64, m64 = gate_alone(a.device, 64, 200)
    print(json.dumps({"gate_alone": True, "bytes_16": b16, "call_us_16_median": round(t16 * 1e6, 1), "call_us_16_min": round(m16 * 1e6, 1),
                      "bytes_64": b64, "call_us_64_median": round(t64 * 1e6, 1), "call_us_64_min": round(m64 * 1e6, 1),
                      "call_rate_64_TBps": round(b64 / t64 / 1e12, 3), "marginal_rate_TBps": round((b64 - b16) / max(t64 - t16, 1e-9) / 1e12, 3),
                      "marginal_share_of_hbm_peak": round((b64 - b16) / max(t64 - t16, 1e-9) / HBM_PEAK, 3)}), flush=True)


if __name__ == "__main__":
    main()
