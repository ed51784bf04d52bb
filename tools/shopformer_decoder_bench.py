#!/usr/bin/env python
"""GCAE decoder throughput: ``forward`` with and without poses, ``decode`` alone, and the reference decoder as
torch-ROCm operators on the same folded weights (linear, matmul per parity, relu, F.interpolate), for the ``shopformer/`` default
and the ``shopformer_2/`` paper config.

Windows and tokens are resident in HBM; the paths of a pair are timed alternately, call by call (hip events around one call, after
warm-up); each cell records the median, min, max and quartiles of ``--reps`` samples.  Prints one JSON line; ``--out`` also writes it.

    python tools/shopformer_decoder_bench.py --out profiles/shopformer_decoder_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.shopformer_bench import stats, timed_pair  # noqa: E402


class TorchDecoder:
    """the folded decoder, operator by operator: what moving the reference's ``gcae.decoder`` to the GPU runs, BatchNorms folded"""

    def __init__(self, geo, tensors, dev):
        self.g = geo
        self.t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in tensors.items() if k.startswith("dec.")}

    @torch.no_grad()
    def __call__(self, tokens):
        g, t = self.g, self.t
        V, H, n = g["V"], g["H"], tokens.shape[0]
        x = F.linear(tokens, t["dec.ip.w"][:, 0, :], t["dec.ip.b"][:V * H]).reshape(n, g["ntok"], V, H)
        for i in range(4):
            w = t[f"dec.l{i}.w"]
            co, f = w.shape[0], w.shape[1]
            y = torch.matmul(x, w.reshape(co * f, H).t()).reshape(n, x.shape[1], V, co, f) + t[f"dec.l{i}.b"][:co, None]
            x = y.permute(0, 1, 4, 2, 3).reshape(n, x.shape[1] * f, V, co)
            if i < 3:
                x = torch.relu(x)
        x = x.permute(0, 3, 1, 2)
        if g["interp"]:
            x = F.interpolate(x, size=(g["T"], V), mode="bilinear", align_corners=False)
        return x.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,4096,65536")
    ap.add_argument("--configs", default="default,paper")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from tools import synth_shopformer_decoder as SD
    from cvsd_amd import Shopformer
    from cvsd_amd import shopformer as SF
    dev = torch.device("cuda:0")
    cells = []
    for name in args.configs.split(","):
        cfg, sd, x = SD.fixture_model(name)
        model = Shopformer.from_state_dict(sd, cfg, device=0, decoder=True)
        ref = TorchDecoder(*SF.parse_image(SF.image_from_state_dict(sd, cfg, decoder=True)), dev)
        di = model.decoder_info
        rows = []
        for n in (int(s) for s in args.sizes.split(",")):
            xd = torch.from_numpy(x[np.arange(n) % len(x)]).to(dev)
            sc = torch.empty(n, device=dev)
            tk = torch.empty((n, model.n_tokens, model.token_dim), device=dev)
            pose, err = torch.empty_like(xd), torch.empty((n,) + tuple(xd.shape[2:]), device=dev)
            st = torch.cuda.current_stream().cuda_stream
            plain = lambda: model.score_device_async(xd.data_ptr(), n, sc.data_ptr(), stream=st, tokens_dev=tk.data_ptr())
            full = lambda: model.score_device_async(xd.data_ptr(), n, sc.data_ptr(), stream=st, tokens_dev=tk.data_ptr(),
                                                    poses_dev=pose.data_ptr(), pose_error_dev=err.data_ptr())
            a, b = timed_pair(plain, full, args.reps, args.warmup)
            dec, tor = timed_pair(lambda: model.decode_device_async(tk.data_ptr(), n, pose.data_ptr(), stream=st), lambda: ref(tk),
                                  args.reps, args.warmup)
            agree = float((pose - ref(tk)).abs().max())
            s = {k: stats(v) for k, v in (("forward", a), ("forward_poses", b), ("decode", dec), ("torch_decode", tor))}
            rows.append({"n": n, **{k + "_us": v["median"] for k, v in s.items()}, **{k + "_us_spread": v for k, v in s.items()},
                         "poses_add_to_forward": s["forward_poses"]["median"] / s["forward"]["median"] - 1.0,
                         "decode_speedup_vs_torch": s["torch_decode"]["median"] / s["decode"]["median"],
                         "decode_tflops": 2 * int(di.macs_per_window) * n / s["decode"]["median"] / 1e6, "max_abs_diff_vs_torch": agree})
        cells.append({"config": name, "variant": model.variant, "decoder_group": int(di.group), "decoder_lds_bytes": int(di.lds_bytes),
                      "decoder_macs_per_window": int(di.macs_per_window), "score_macs_per_window": int(model.info.macs_per_window),
                      "factors": list(di.factors), "frames": int(di.frames), "interpolate": int(di.interpolate), "rows": rows})
    out = {"bench": "shopformer_decoder", "reps": args.reps, "row_group_env": os.environ.get("MI355_SFD_ROW_GROUP"), "cells": cells}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
