"""What a JPEG evidence frame costs, on one 1080 x 1920 frame with 10 and with 100 synthetic people drawn in
(tools/render_bench.py's people):

  * the encode launches alone -- transform, code and pack, timed with events inside the call (``ops.jpeg_encode(..., timing=)``), the
    rendered picture on the GPU -- next to a plain device-to-device copy of the same frame measured in the same run, the floor
    DESIGN.md 3.19 uses.  Median, min and max over ``--repeats``; the ratio is quoted, not gated on.
  * ``predict(render=..., encode="jpeg")`` against today's alternative, ``predict(render=...)`` followed by Pillow encoding
    ``Results.rendered`` on the host at the same quality and subsampling, the two sides alternating; and the bytes each side brings
    back from the GPU.
  * the step time of ``predict()`` without ``encode``: compare it with the same figure of the parent commit (the call as it was).

    python tools/jpeg_bench.py --repeats 30

One JSON line per measurement."""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.render_bench import H, W, people, stats  # noqa: E402


def launches(pic_dev, repeats, quality, subsampling):
    import torch
    from cvsd_amd import ops
    ms, copy, size = [], [], 0
    dst = torch.empty_like(pic_dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(repeats + 3):
        t = []
        size = len(ops.jpeg_encode(pic_dev, quality=quality, subsampling=subsampling, device=0, timing=t))
        e0.record(); dst.copy_(pic_dev); e1.record(); torch.cuda.synchronize()
        if r >= 3:
            ms.append(t[0]); copy.append(e0.elapsed_time(e1))
    return ms, copy, size


def pillow_encode(bgr, quality, subsampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(bgr[..., ::-1]).save(buf, "JPEG", quality=quality, subsampling={"420": 2, "444": 0}[subsampling])
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--model", default="yolov8n-pose")
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--subsampling", default="420")
    args = ap.parse_args()
    import torch
    from cvsd_amd import YOLO, JpegSpec, RenderSpec, ops
    from cvsd_amd.render import primitives
    from tools import synth
    frame = synth.synthetic_frames(1, H, W, seed=1)[0]
    spec = RenderSpec(anonymize="head")
    jspec = JpegSpec(quality=args.quality, subsampling=args.subsampling)
    for n in (10, 100):
        pic = ops.render(frame, primitives(people(n), spec), device=0)
        dev = torch.from_numpy(pic).cuda()
        assert ops.jpeg_encode(dev, args.quality, args.subsampling, device=0) == ops.jpeg_encode(pic, args.quality, args.subsampling, device=-1), \
            "the kernels disagree with the host twin"
        ms, copy, size = launches(dev, args.repeats, args.quality, args.subsampling)
        print(json.dumps({"what": "encode launches, 1080x1920", "people": n, "quality": args.quality, "subsampling": args.subsampling, "jpeg_bytes": size,
                          "pillow_bytes": len(pillow_encode(pic, args.quality, args.subsampling)), "encode_ms": stats(ms), "d2d_copy_ms": stats(copy),
                          "ratio_to_copy": round(float(np.median(ms) / np.median(copy)), 2)}), flush=True)
    _, sd = synth.synthetic_checkpoint(args.model, seed=0)
    model = YOLO.from_state_dict(args.model, sd, device=0)
    kw = dict(conf=0.05, max_det=100)
    for _ in range(3):
        model.predict(frame, **kw); model.predict(frame, render=spec, **kw); model.predict(frame, render=spec, encode=jspec, **kw)
    plain, gpu, host, src = [], [], [], []
    for _ in range(args.repeats):
        t0 = time.perf_counter(); r = model.predict(frame, **kw)[0]; t1 = time.perf_counter()
        r1 = model.predict(frame, render=spec, **kw)[0]; theirs = pillow_encode(r1.rendered, args.quality, args.subsampling); t2 = time.perf_counter()
        r2 = model.predict(frame, render=spec, encode=jspec, **kw)[0]; t3 = time.perf_counter()
        r3 = model.predict(frame, encode=jspec, **kw)[0]; t4 = time.perf_counter()
        assert r2.rendered is None and r2.jpeg[:2] == b"\xff\xd8" and len(r) == len(r2)
        plain.append((t1 - t0) * 1e3); host.append((t2 - t1) * 1e3); gpu.append((t3 - t2) * 1e3); src.append((t4 - t3) * 1e3)
    print(json.dumps({"what": "predict, one 1080x1920 host frame", "model": args.model, "rows": len(r), "predict_ms": stats(plain),
                      "predict_render_encode_ms": stats(gpu), "predict_render_then_pillow_ms": stats(host), "predict_encode_source_ms": stats(src),
                      "bytes_back_encode": len(r2.jpeg), "bytes_back_render": int(r1.rendered.nbytes), "pillow_bytes": len(theirs),
                      "source_jpeg_bytes": len(r3.jpeg)}), flush=True)


if __name__ == "__main__":
    main()
