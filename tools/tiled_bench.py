"""What tiled predict costs against doing it by hand: 1080 x 1920 host frames, ``tile=640``, ``overlap=0.2``,
``imgsz=640`` -- 8 tiles plus the frame itself per frame -- at 1 and 8 frames per call.

    tiled      ``model.predict(frames, tile=640, overlap=0.2)``: one upload per frame, one detector pass, the merge on the GPU
    baseline   what a user writes without it: ``model.predict(list of the 9 crops of every frame)`` (numpy views, no copy on the host)
               and the merge of the sequential checker (tests/_tile_merge_numpy.py) over the rows that come back

Same weights, same frames, same process, the sides alternating; median wall time per call over ``--calls`` calls after warm-up, and
the baseline's own run-to-run spread (its min and max).  ``--side baseline`` runs the baseline alone and needs nothing of the feature
but the checker file, so the same tool measures a checkout of the parent commit.

    python tools/tiled_bench.py --frames 1 8 --calls 20

One JSON line with the untiled call's launch plan (``plan_info``), then one per batch size."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TILE, OVERLAP, IMGSZ, CONF = 640, 0.2, 640, 0.25


def baseline_call(model, frames, T):
    ents = [T.entries(f.shape[0], f.shape[1], TILE, OVERLAP, True) for f in frames]
    crops = [f[y:y + h, x:x + w] for f, g in zip(frames, ents) for x, y, w, h in g]
    res = model.predict(crops, conf=CONF, imgsz=IMGSZ)
    nkpt, kdim = model.kpt_shape
    out, at = [], 0
    for g in ents:
        rows = np.zeros((len(g), 300, T.DET_WORDS), np.float32)
        counts = np.zeros(len(g), np.int32)
        for e in range(len(g)):
            r = res[at + e]
            d = r.boxes.data.numpy()
            counts[e] = len(d)
            rows[e, :len(d), :5] = d[:, :5]
            iv = rows[e].view(np.int32)
            iv[:len(d), 5] = d[:, 5].astype(np.int32)
            iv[:len(d), 6] = r.anchor_idx
            if nkpt:
                rows[e, :len(d), 7:7 + nkpt * kdim] = r.keypoints_raw.reshape(len(d), -1)
        at += len(g)
        out.append(T.merge_frame(rows, counts, g[:, :2], kdim, "ios", 0.5, nk=nkpt * kdim))
    return out


def tiled_call(model, frames):
    return model.predict(frames, conf=CONF, imgsz=IMGSZ, tile=TILE, overlap=OVERLAP)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--side", choices=["both", "baseline"], default="both")
    ap.add_argument("--model", default="yolov8n-pose")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import _tile_merge_numpy as T
    from cvsd_amd import YOLO
    from tools import synth
    _, sd = synth.synthetic_checkpoint(a.model, seed=0)
    model = YOLO.from_state_dict(a.model, sd, device=a.device)
    # the untiled call's launch plan first, on the fresh engine: the arena of a handle only grows, so later it carries the handle's history
    model.predict(synth.synthetic_frames(1, 1080, 1920, seed=11), conf=CONF, imgsz=IMGSZ)
    info = model.plan_info()
    print(json.dumps({"section": "untiled_plan", "frame": [1080, 1920],
                      **{k: info[k] for k in ("plan_hash", "launches_per_pass", "activation_bytes")}}), flush=True)
    sides = {"baseline": lambda fr: baseline_call(model, fr, T)}
    if a.side == "both":
        sides["tiled"] = lambda fr: tiled_call(model, fr)
    for n in a.frames:
        frames = list(synth.synthetic_frames(n, 1080, 1920, seed=11))
        wall = {k: [] for k in sides}
        for i in range(a.warmup + a.calls):
            for k, fn in sides.items():
                t0 = time.perf_counter()
                fn(frames)
                dt = time.perf_counter() - t0
                if i >= a.warmup:
                    wall[k].append(1e3 * dt)
        ents = T.entries(1080, 1920, TILE, OVERLAP, True)
        frame_bytes = 1080 * 1920 * 3
        row = {"section": "tiled_predict", "model": a.model, "frames_per_call": n, "entries_per_frame": len(ents), "calls": a.calls,
               "h2d_bytes_per_call": {"baseline": n * int(sum(w * h * 3 for _, _, w, h in ents)), "tiled": n * frame_bytes}}
        for k, v in wall.items():
            row[f"{k}_ms_per_call_median"] = round(float(np.median(v)), 3)
            row[f"{k}_ms_per_call_min_max"] = [round(float(min(v)), 3), round(float(max(v)), 3)]
            row[f"{k}_ms_per_frame_median"] = round(float(np.median(v)) / n, 3)
        if "tiled" in sides:
            # the two sides give the same rows; and the NMS span's device time (HIP events) with and without the merge launch behind it
            got, want = tiled_call(model, frames), baseline_call(model, frames, T)
            row["rows_per_frame"] = [len(r) for r in got]
            row["same_rows"] = all(np.array_equal(r.boxes.data.numpy()[:, :5], w[0][:, :5]) and np.array_equal(r.tile_idx, w[1])
                                   for r, w in zip(got, want))
            model.set_profiling(True)
            spans = {"tiled": [], "baseline": []}
            for _ in range(5):
                tiled_call(model, frames)
                spans["tiled"].append(model.last_timing()["nms_ms"])
                baseline_call(model, frames, T)
                spans["baseline"].append(model.last_timing()["nms_ms"])
            model.set_profiling(False)
            row["nms_span_ms_median"] = {k: round(float(np.median(v)), 4) for k, v in spans.items()}
            row["merge_launch_ms"] = round(float(np.median(spans["tiled"]) - np.median(spans["baseline"])), 4)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
