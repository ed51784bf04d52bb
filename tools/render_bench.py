"""What an evidence frame costs, on one 1080 x 1920 frame with synthetic people (box, ``#id conf`` label, 19 limbs,
17 joints, a pixelated head each):

  * the render launches alone -- the bins' memset, the bin launch and the draw launch, timed with events inside the call
    (``ops.render(..., timing=)``), source and output on the GPU -- with 10 and with 100 people, next to a plain device-to-device copy of
    the same frame measured in the same run: the floor of any out-of-place pass.  Median, min and max over ``--repeats``; the ratio is
    quoted, not gated on.
  * ``predict(render=True)`` against ``predict()`` followed by a rendering of the same primitives on the host in vectorised numpy
    (bounding-box windows, int64 -- the rules of tests/_render_numpy.py, which is exact but too slow to be a fair opponent), the two
    sides alternating.
  * the step time of ``predict()`` without ``render``: compare it with the same figure of the parent commit (the call as it was).

    python tools/render_bench.py --repeats 30

One JSON line per measurement."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W = 1080, 1920


def people(n, seed=0):
    """a tracked pose ``Results`` of n people spread over the frame, every joint visible"""
    import torch
    from cvsd_amd import Results
    rng = np.random.default_rng(seed)
    boxes, kpts = [], []
    for i in range(n):
        bw, bh = int(rng.integers(80, 200)), int(rng.integers(200, 480))
        x, y = int(rng.integers(0, W - bw)), int(rng.integers(0, H - bh))
        boxes.append([x, y, x + bw, y + bh, i + 1, 0.5 + 0.4 * rng.random(), 0])
        k = np.empty((17, 3), np.float32)
        k[:, 0] = x + rng.random(17) * bw
        k[:, 1] = y + np.sort(rng.random(17)) * bh
        k[:5, 1] = y + rng.random(5) * bh * 0.12
        k[:, 2] = 0.9
        kpts.append(k)
    return Results(None, "bench.jpg", {0: "person"}, boxes=torch.tensor(boxes, dtype=torch.float32), keypoints=torch.tensor(np.stack(kpts)),
                   orig_shape=(H, W))


def stats(v):
    v = np.sort(np.asarray(v, np.float64))
    return {"median": round(float(np.median(v)), 4), "min": round(float(v[0]), 4), "max": round(float(v[-1]), 4)}


def launches(frame_dev, prims, repeats):
    import torch
    from cvsd_amd import ops
    ms, copy = [], []
    dst = torch.empty_like(frame_dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(repeats + 3):
        t = []
        ops.render(frame_dev, prims, device=0, out="cuda", timing=t)
        e0.record(); dst.copy_(frame_dev); e1.record(); torch.cuda.synchronize()
        if r >= 3:
            ms.append(t[0]); copy.append(e0.elapsed_time(e1))
    return ms, copy


_GLYPHS = {}


def glyph(ch):
    """the font's 7 x 5 bitmap of a character, read off the rasteriser's host twin"""
    if ch not in _GLYPHS:
        from cvsd_amd import ops
        rec = np.array([[6, 0, 0, ch, 0, 1, 0xFFFFFF, 0]], np.int32)
        _GLYPHS[ch] = ops.render(np.zeros((7, 5, 3), np.uint8), rec, device=-1)[..., 0] != 0
    return _GLYPHS[ch]


def host_render(frame, prims):
    """the rasteriser's rules in vectorised numpy over each primitive's clipped bounding box (int64: the frame keeps products small)"""
    out = frame.copy()
    means = {}
    h, w = frame.shape[:2]

    def window(x0, y0, x1, y1):
        return max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
    for p in prims:
        if p[0] != 1:
            continue
        B = int(p[5])
        if B not in means:
            hh, ww = -(-h // B) * B, -(-w // B) * B
            pad = np.zeros((hh, ww, 3), np.int64); pad[:h, :w] = frame
            cnt = np.zeros((hh, ww), np.int64); cnt[:h, :w] = 1
            s = pad.reshape(hh // B, B, ww // B, B, 3).sum(axis=(1, 3)); n = cnt.reshape(hh // B, B, ww // B, B).sum(axis=(1, 3))[..., None]
            means[B] = ((2 * s + n) // (2 * n)).astype(np.uint8)
        x0, y0, x1, y1 = window(*p[1:5])
        if x1 >= x0 and y1 >= y0:
            ys, xs = np.arange(y0, y1 + 1) // B, np.arange(x0, x1 + 1) // B
            out[y0:y1 + 1, x0:x1 + 1] = means[B][ys[:, None], xs[None, :]]
    for p in prims:
        t, a, b, c, d, size, col = (int(v) for v in p[:7])
        if t == 1:
            continue
        bgr = (col & 255, (col >> 8) & 255, (col >> 16) & 255)
        if t == 4:
            r = (size + 1) // 2
            box = (min(a, c) - r, min(b, d) - r, max(a, c) + r, max(b, d) + r)
        elif t == 5:
            box = (a - size, b - size, a + size, b + size)
        elif t == 6:
            box = (a, b, a + 5 * size - 1, b + 7 * size - 1)
        else:
            box = (a, b, c, d)
        x0, y0, x1, y1 = window(*box)
        if x1 < x0 or y1 < y0:
            continue
        py, px = np.arange(y0, y1 + 1, dtype=np.int64)[:, None], np.arange(x0, x1 + 1, dtype=np.int64)[None, :]
        if t == 3:
            m = np.ones((y1 - y0 + 1, x1 - x0 + 1), bool)
        elif t == 2:
            m = ~((px >= a + size) & (px <= c - size) & (py >= b + size) & (py <= d - size))
        elif t == 5:
            m = (px - a) ** 2 + (py - b) ** 2 <= size * size
        elif t == 4:
            dx, dy, qx, qy = c - a, d - b, px - a, py - b
            u, l2, cr = qx * dx + qy * dy, dx * dx + dy * dy, dx * qy - dy * qx
            m = np.where(u <= 0, 4 * (qx * qx + qy * qy) <= size * size,
                         np.where(u >= l2, 4 * ((px - c) ** 2 + (py - d) ** 2) <= size * size, 4 * cr * cr <= size * size * l2))
        else:
            g = glyph(c)
            m = g[((py - b) // size).clip(0, 6), ((px - a) // size).clip(0, 4)] & (px >= a) & (py >= b) & (px < a + 5 * size) & (py < b + 7 * size)
        out[y0:y1 + 1, x0:x1 + 1][np.broadcast_to(m, (y1 - y0 + 1, x1 - x0 + 1))] = bgr
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--model", default="yolov8n-pose")
    args = ap.parse_args()
    import torch
    from cvsd_amd import YOLO, RenderSpec, ops
    from cvsd_amd.render import primitives
    from tools import synth
    frame = synth.synthetic_frames(1, H, W, seed=1)[0]
    dev = torch.from_numpy(frame).cuda()
    spec = RenderSpec(anonymize="head")
    for n in (10, 100):
        prims = primitives(people(n), spec)
        got = ops.render(frame, prims, device=0)
        assert np.array_equal(got, host_render(frame, prims)), "the host rendering of this tool disagrees with the kernel"
        ms, copy = launches(dev, prims, args.repeats)
        print(json.dumps({"what": "render launches, 1080x1920", "people": n, "primitives": int(len(prims)), "render_ms": stats(ms), "d2d_copy_ms": stats(copy),
                          "ratio_to_copy": round(float(np.median(ms) / np.median(copy)), 2)}), flush=True)
    _, sd = synth.synthetic_checkpoint(args.model, seed=0)
    model = YOLO.from_state_dict(args.model, sd, device=0)
    kw = dict(conf=0.05, max_det=100)
    for _ in range(3):
        model.predict(frame, **kw); model.predict(frame, render=spec, **kw)
    plain, gpu, host = [], [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter(); r = model.predict(frame, **kw)[0]; t1 = time.perf_counter()
        pic = host_render(frame, primitives(r, spec)); t2 = time.perf_counter()
        r2 = model.predict(frame, render=spec, **kw)[0]; t3 = time.perf_counter()
        assert np.array_equal(pic, r2.rendered)
        plain.append((t1 - t0) * 1e3); host.append((t2 - t0) * 1e3); gpu.append((t3 - t2) * 1e3)
    print(json.dumps({"what": "predict, one 1080x1920 host frame", "model": args.model, "rows": len(r), "primitives": int(len(primitives(r, spec))),
                      "predict_ms": stats(plain), "predict_render_ms": stats(gpu), "predict_then_numpy_render_ms": stats(host)}), flush=True)


if __name__ == "__main__":
    main()
