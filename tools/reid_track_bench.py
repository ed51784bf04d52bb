"""What BoT-SORT's appearance matching costs: the frame-by-frame ``model.track`` loop and ``model.track_cameras``, each
with and without ``tracker={"with_reid": True}``, on the synthetic clips the tests use -- same weights, same frames, same process, the
sides alternating ``--repeats`` times -- and, per batch size, what the feature output adds to a detector call: the launch plans of the
two engines (``plan_info``), the arena growth, and the device time of the NMS span (NMS + scale-back + the gather launch behind it,
HIP events) with the option off and on, whose difference is the gather.

    python tools/reid_track_bench.py --frames 120 --cameras 4 --batches 1 512 --repeats 5

One JSON line per section.  On a checkout without the feature (no ``feats`` argument) only the sides without it run, so the same file
measures the parent commit."""
from __future__ import annotations

import argparse
import inspect
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def long_clip(n, h, w, seed):
    """``n`` frames of ``synth.synthetic_clip``: its 32-frame drift played forwards and backwards, so consecutive frames stay one step apart"""
    from tools import synth
    base = np.ascontiguousarray(synth.synthetic_clip(32, h, w, seed=seed))
    order = list(range(32)) + list(range(30, 0, -1))
    return [base[order[t % len(order)]] for t in range(n)]


def run_track(model, clip, warmup, tracker):
    model._tracker = None
    kw = {"tracker": tracker} if tracker else {}
    spent = 0.0
    for t, f in enumerate(clip):
        t0 = time.perf_counter()
        model.track(f, persist=True, **kw)
        if t >= warmup:
            spent += time.perf_counter() - t0
    return (len(clip) - warmup) / spent


def run_cameras(model, clips, warmup, tracker):
    kw = {"tracker": tracker} if tracker else {}
    spent = 0.0
    for t in range(len(clips[0])):
        frames = [c[t] for c in clips]
        t0 = time.perf_counter()
        model.track_cameras(frames, persist=t > 0, **kw)
        if t >= warmup:
            spent += time.perf_counter() - t0
    return (len(clips[0]) - warmup) * len(clips) / spent


def summary(row, fps):
    for k, v in fps.items():
        row[f"{k}_fps_median"] = round(float(np.median(v)), 1)
        row[f"{k}_fps_min"], row[f"{k}_fps_max"] = round(float(min(v)), 1), round(float(max(v)), 1)
    return row


def detector_call(models, batch, h, w, repeats):
    """plan_info and the NMS span's device time of one predict over ``batch`` frames, feature output off / on, alternating"""
    from tools import synth
    frames = np.tile(synth.synthetic_frames(min(batch, 8), h, w, seed=7), (max(1, batch // 8), 1, 1, 1))[:batch]
    row = {"section": "detector_call", "batch": batch, "frame": [h, w]}
    spans = {k: [] for k in models}
    total = {k: [] for k in models}
    for k, m in models.items():
        m.predict(frames, conf=0.1)                                # plans, buffers
        m.set_profiling(True)
    for _ in range(repeats):
        for k, m in models.items():
            m.predict(frames, conf=0.1, feats=(k == "on"))
            t = m.last_timing()
            spans[k].append(t["nms_ms"])
            total[k].append(t["total_ms"])
    for k, m in models.items():
        m.set_profiling(False)
        m.predict(frames, conf=0.1, feats=(k == "on"))
        info = m.plan_info()
        row[f"{k}_plan"] = {x: info[x] for x in ("plan_hash", "launches_per_pass", "activation_bytes")}
        row[f"{k}_nms_span_ms_median"] = round(float(np.median(spans[k])), 4)
        row[f"{k}_nms_span_ms_min_max"] = [round(float(min(spans[k])), 4), round(float(max(spans[k])), 4)]
        row[f"{k}_total_ms_median"] = round(float(np.median(total[k])), 3)
    if "on" in models:
        chunks = -(-batch // 64)
        row["gather_ms_per_call"] = round(row["on_nms_span_ms_median"] - row["off_nms_span_ms_median"], 4)
        row["gather_us_per_chunk"] = round(1e3 * row["gather_ms_per_call"] / chunks, 2)
        # the arena of a handle only grows, so plan_info's bytes carry the handle's history; the growth is taken from the planner itself
        from cvsd_amd import ops
        m, per_pass = models["on"], min(batch, 64)
        a0 = ops.memory_plan_ex(m._blob, per_pass, h, w, obj_feats=False)[2]
        a1, maps = (lambda r: (r[2], int(sum(r[1][d] for d in r[4]))))(ops.memory_plan_ex(m._blob, per_pass, h, w, obj_feats=True))
        row["arena_bytes_off_on"], row["arena_growth_bytes"], row["detect_input_map_bytes"] = [a0, a1], a1 - a0, maps
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cameras", type=int, default=4)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 512])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--model", default="yolov8n-pose")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    from cvsd_amd import YOLO
    from tools import synth
    _, sd = synth.synthetic_checkpoint(a.model, seed=0)
    has_feats = "feats" in inspect.signature(YOLO.__init__).parameters
    model = YOLO.from_state_dict(a.model, sd, device=a.device)
    sides = {"iou": None}
    if has_feats:
        sides["reid"] = {"with_reid": True}

    clip = long_clip(a.frames, 480, 640, 5)
    fps = {k: [] for k in sides}
    for _ in range(a.repeats + 1):                                 # the first round warms both engines and is dropped
        for k, cfg in sides.items():
            fps[k].append(run_track(model, clip, a.warmup, cfg))
    print(json.dumps(summary({"section": "track", "model": a.model, "frame": [480, 640], "frames": a.frames, "repeats": a.repeats},
                             {k: v[1:] for k, v in fps.items()})), flush=True)

    clips = [long_clip(a.frames, 240, 320, 3 + i) for i in range(a.cameras)]
    fps = {k: [] for k in sides}
    for _ in range(a.repeats + 1):
        for k, cfg in sides.items():
            fps[k].append(run_cameras(model, clips, a.warmup, cfg))
    print(json.dumps(summary({"section": "track_cameras", "model": a.model, "cameras": a.cameras, "frame": [240, 320], "ticks": a.frames,
                              "repeats": a.repeats}, {k: v[1:] for k, v in fps.items()})), flush=True)

    models = {"off": model}
    if has_feats:
        models["on"] = YOLO.from_state_dict(a.model, sd, device=a.device, feats=True)
    for batch in a.batches:
        print(json.dumps(detector_call(models, batch, 480, 640, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
