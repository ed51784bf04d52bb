"""What JPEG ingest costs, on 16 streams of 1080 x 1920 at 4:2:0 and quality 85, once without restart markers (what most
cameras send) and once with a restart marker per MCU row (what the project's own encoder writes).  Four routes to 16 BGR frames on the
GPU, measured in the same run, the sides alternating:

  (a) the parent's only route: Pillow decodes every stream on the calling thread and the frames are uploaded at 3 bytes per pixel;
  (b) ``ops.jpeg_decode(..., entropy="host", as_tensor=True)``: Huffman decoding on the calling thread, coefficients uploaded, idct and
      colour on the GPU;
  (c) ``ops.jpeg_decode(..., entropy="gpu", as_tensor=True)``: one GPU lane per restart segment (without restart markers: one lane per
      frame -- measured because it is how the kernel runs on any stream, not because anyone should use it);
  (d) ``ops.jpeg_decode(..., entropy="sync", as_tensor=True)``: many GPU lanes per restart segment, the self-synchronising parallel
      Huffman decoder -- once per subsequence length of ``--sub-bytes`` (the library reads MI355_JPEG_SYNC_SUB_BYTES at every call;
      the first value is reported as route (d)); the streams' round counts come from ``ops.jpeg_sync``.

Wall time around the call, which ends in a device synchronise; the launches' device time from the events inside the call; and the bytes
each route moves over PCIe, computed from the shapes.  Every route's frames are compared with Pillow's before anything is timed.

    python tools/jpeg_decode_bench.py --repeats 20

One JSON line per stream kind."""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.render_bench import H, W, stats  # noqa: E402


def pillow_route(streams, device):
    import torch
    from PIL import Image
    out = []
    for d in streams:
        with Image.open(io.BytesIO(d)) as im:
            bgr = np.ascontiguousarray(np.asarray(im.convert("RGB"), np.uint8)[..., ::-1])
        out.append(torch.from_numpy(bgr).to(f"cuda:{device}"))
    torch.cuda.synchronize(device)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sub-bytes", default="128,64,256", help="subsequence lengths of route (d), the first is the one reported as (d)")
    args = ap.parse_args()
    from PIL import Image
    from cvsd_amd import JPEGFrame, ops
    from tools import synth
    subs = [int(s) for s in args.sub_bytes.split(",")]

    def sync_route(sub, timing=None):
        os.environ["MI355_JPEG_SYNC_SUB_BYTES"] = str(sub)
        try:
            return ops.jpeg_decode(streams, device=args.device, entropy="sync", as_tensor=True, timing=timing)
        finally:
            del os.environ["MI355_JPEG_SYNC_SUB_BYTES"]
    frames = synth.synthetic_frames(args.frames, H, W, seed=1)
    for kind, opts in (("no restart markers", {}), ("restart marker per MCU row", {"restart_marker_rows": 1})):
        streams = []
        for f in frames:
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(f[..., ::-1])).save(buf, "JPEG", quality=args.quality, subsampling=2, **opts)
            streams.append(JPEGFrame(buf.getvalue()))
        raw = [s.data for s in streams]
        ref = pillow_route(raw, args.device)
        for e in ("host", "gpu"):
            for a, b in zip(ref, ops.jpeg_decode(streams, device=args.device, entropy=e, as_tensor=True)):
                assert bool((a == b).all()), f"entropy={e} disagrees with Pillow"
        for sub in subs:
            for a, b in zip(ref, sync_route(sub)):
                assert bool((a == b).all()), f"entropy=sync with subsequences of {sub} bytes disagrees with Pillow"
        rounds = {sub: [ops.jpeg_sync(s, args.device, sub, 256)["stats"] for s in streams] for sub in subs}
        wall = {"pillow": [], "host": [], "gpu": [], **{f"sync{sub}": [] for sub in subs}}
        dev_ms = {"host": [], "gpu": [], **{f"sync{sub}": [] for sub in subs}}
        for r in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            pillow_route(raw, args.device)
            t1 = time.perf_counter()
            th = []
            ops.jpeg_decode(streams, device=args.device, entropy="host", as_tensor=True, timing=th)
            t2 = time.perf_counter()
            tg = []
            ops.jpeg_decode(streams, device=args.device, entropy="gpu", as_tensor=True, timing=tg)
            t3 = time.perf_counter()
            for sub in subs:
                ts = []
                t4 = time.perf_counter()
                sync_route(sub, ts)
                t5 = time.perf_counter()
                if r >= args.warmup:
                    wall[f"sync{sub}"].append((t5 - t4) * 1e3); dev_ms[f"sync{sub}"].append(ts[0]["ms"])
            if r >= args.warmup:
                wall["pillow"].append((t1 - t0) * 1e3); wall["host"].append((t2 - t1) * 1e3); wall["gpu"].append((t3 - t2) * 1e3)
                dev_ms["host"].append(th[0]["ms"]); dev_ms["gpu"].append(tg[0]["ms"])
        comp = sum(len(d) for d in raw)
        med = {k: float(np.median(v)) for k, v in wall.items()}
        print(json.dumps({
            "what": f"{args.frames} streams of {H}x{W}, 4:2:0, quality {args.quality}, {kind}", "segments_per_stream": streams[0].segments,
            "compressed_bytes": comp,
            "a_pillow_then_upload_ms": stats(wall["pillow"]), "b_entropy_host_ms": stats(wall["host"]), "c_entropy_gpu_ms": stats(wall["gpu"]),
            "d_entropy_sync_ms": stats(wall[f"sync{subs[0]}"]), "d_launches_ms": stats(dev_ms[f"sync{subs[0]}"]),
            "d_by_sub_bytes": {str(sub): {"wall_ms": stats(wall[f"sync{sub}"]), "launches_ms": stats(dev_ms[f"sync{sub}"]),
                                          "nsub": [s["nsub"] for s in rounds[sub]], "nseq": [s["nseq"] for s in rounds[sub]],
                                          "rounds_local": [s["rounds_local"] for s in rounds[sub]],
                                          "rounds_global": [s["rounds_global"] for s in rounds[sub]]} for sub in subs},
            "d_over_b": round(float(np.median(wall[f"sync{subs[0]}"])) / med["host"], 3),
            "b_launches_ms": stats(dev_ms["host"]), "c_launches_ms": stats(dev_ms["gpu"]),
            "b_over_a": round(med["host"] / med["pillow"], 3), "c_over_a": round(med["gpu"] / med["pillow"], 3),
            "pcie_bytes": {"a": args.frames * H * W * 3, "b": sum(s.blocks for s in streams) * 128, "c": comp, "d": comp}}), flush=True)


if __name__ == "__main__":
    main()
