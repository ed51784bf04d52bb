"""What person crops cost: 16 frames of 1080 x 1920 with 8 person-sized boxes each, cut to ``size=(256, 128)`` and at
native size, the frames starting in HBM (CUDA tensors -- where YUV, JPEG and CUDA sources leave them):

  * ``gpu``        ``ops.crop_resize(out="cuda")``: one launch, nothing crosses the bus.  The launch alone (events inside the call) and the
                   whole call (host clock around a call that ends in a stream synchronise).
  * ``gpu+jpeg``   the same plus ONE ``ops.jpeg_encode`` call over the crops: only the streams' bytes come back.
  * ``gpu->host``  ``ops.crop_resize(out="numpy")``: the crops' pixels come back.
  * ``host``       the route without the feature: the whole frames to the host, then slicing and cv2.resize(INTER_LINEAR)'s fixed point
                   in vectorised numpy (``resize_u8`` below, checked against the kernel's bytes before anything is timed).

The sides alternate inside one loop; median, min and max over ``--repeats``.  PCIe bytes are counted from shapes.  The launch's effective
rate is (source rectangle bytes + output bytes) / launch time, next to the 8 TB/s HBM peak: the launch moves a few MB, so this is a
statement about latency, not about bandwidth.

    python tools/crops_bench.py --repeats 20

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
N_FRAMES, N_BOXES = 16, 8
HBM_PEAK = 8e12


def boxes(seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N_BOXES):
        bw, bh = int(rng.integers(80, 200)), int(rng.integers(200, 480))
        x, y = int(rng.integers(0, W - bw)), int(rng.integers(0, H - bh))
        out.append([x, y, x + bw, y + bh])
    return np.array(out, np.float32)


def stats(v):
    v = np.sort(np.asarray(v, np.float64))
    return {"median": round(float(np.median(v)), 4), "min": round(float(v[0]), 4), "max": round(float(v[-1]), 4)}


def _taps(dn, sn):
    d = np.arange(dn, dtype=np.float64)
    fx = ((d + 0.5) * (sn / dn) - 0.5).astype(np.float32)
    s = np.floor(fx).astype(np.int64)
    fx = fx - s.astype(np.float32)
    lo, hi = s < 0, s >= sn - 1
    s = np.where(lo, 0, np.where(hi, sn - 1, s))
    fx = np.where(lo | hi, np.float32(0), fx).astype(np.float32)
    a0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(fx * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, sn - 1), a0, a1


def resize_u8(img, dw, dh):
    """cv2.resize(img, (dw, dh), INTER_LINEAR) for uint8 [h, w, 3] in OpenCV's 11-bit fixed point, vectorised"""
    sh, sw = img.shape[:2]
    if (sw, sh) == (dw, dh):
        return img.copy()
    x0, x1, a0, a1 = _taps(dw, sw)
    y0, y1, b0, b1 = _taps(dh, sh)
    src = img.astype(np.int32)
    hor = src[:, x0] * a0[None, :, None].astype(np.int32) + src[:, x1] * a1[None, :, None].astype(np.int32)
    out = (((b0[:, None, None] * (hor[y0] >> 4)) >> 16) + ((b1[:, None, None] * (hor[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    import torch
    from cvsd_amd import ops
    from cvsd_amd.crops import crop_rects
    from tools import synth
    if not torch.cuda.is_available():
        raise SystemExit("crops_bench needs an MI355X: there is no timing without one")
    host = synth.synthetic_frames(N_FRAMES, H, W, seed=1)
    dev = [torch.from_numpy(f).cuda() for f in host]
    rects = [crop_rects(boxes(i), (H, W)) for i in range(N_FRAMES)]
    src_bytes = int(sum(int((r[2] - r[0]) * (r[3] - r[1]) * 3) for rr in rects for r in rr))
    frame_bytes = N_FRAMES * H * W * 3

    def host_route(size):
        frames = [d.cpu().numpy() for d in dev]                        # the whole frames cross the bus
        out = []
        for f, rr in zip(frames, rects):
            for x1, y1, x2, y2 in rr.tolist():
                cut = f[y1:y2, x1:x2]
                out.append(cut.copy() if size is None else resize_u8(cut, size[1], size[0]))
        return out

    for size in ((256, 128), None):
        name = "native" if size is None else f"{size[0]}x{size[1]}"
        got = ops.crop_resize(dev, rects, size=size, device=0)
        flat = [c for g in got for c in g]
        assert all(np.array_equal(a, b) for a, b in zip(flat, host_route(size))), "the numpy route of this tool disagrees with the kernel"
        out_bytes = int(sum(c.size for c in flat))
        for _ in range(3):                                             # every shape of the timed window, warm
            cc = ops.crop_resize(dev, rects, size=size, device=0, out="cuda")
            ops.jpeg_encode([c for g in cc for c in g], device=0)
            ops.crop_resize(dev, rects, size=size, device=0)
            ops.crop_resize(list(host), rects, size=size, device=0)
        launch, gpu, gpu_jpeg, gpu_host, from_host, cpu = [], [], [], [], [], []
        jpeg_bytes = 0
        for _ in range(args.repeats):
            t = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.crop_resize(dev, rects, size=size, device=0, out="cuda", timing=t)
            t1 = time.perf_counter()
            cc = ops.crop_resize(dev, rects, size=size, device=0, out="cuda")
            streams = ops.jpeg_encode([c for g in cc for c in g], device=0)
            t2 = time.perf_counter()
            ops.crop_resize(dev, rects, size=size, device=0)
            t3 = time.perf_counter()
            ops.crop_resize(list(host), rects, size=size, device=0)
            t4 = time.perf_counter()
            host_route(size)
            t5 = time.perf_counter()
            jpeg_bytes = sum(len(s) for s in streams)
            launch.append(t[0]); gpu.append((t1 - t0) * 1e3); gpu_jpeg.append((t2 - t1) * 1e3); gpu_host.append((t3 - t2) * 1e3)
            from_host.append((t4 - t3) * 1e3); cpu.append((t5 - t4) * 1e3)
        moved = src_bytes + out_bytes
        print(json.dumps({"what": f"{N_FRAMES} frames 1080x1920 in HBM, {N_BOXES} boxes each", "size": name, "crops": len(flat),
                          "source_rect_bytes": src_bytes, "output_bytes": out_bytes,
                          "launch_ms": stats(launch), "launch_GBps": round(moved / (np.median(launch) * 1e-3) / 1e9, 1),
                          "share_of_hbm_peak": round(moved / (np.median(launch) * 1e-3) / HBM_PEAK, 4),
                          "gpu_call_ms": stats(gpu), "gpu_call_pcie_bytes": 0,
                          "gpu_call_plus_jpeg_ms": stats(gpu_jpeg), "gpu_call_plus_jpeg_pcie_bytes": int(jpeg_bytes),
                          "gpu_call_pixels_to_host_ms": stats(gpu_host), "gpu_call_pixels_to_host_pcie_bytes": out_bytes,
                          "host_route_ms": stats(cpu), "host_route_pcie_bytes": frame_bytes,
                          "host_frames_gpu_call_ms": stats(from_host)}), flush=True)


if __name__ == "__main__":
    main()
