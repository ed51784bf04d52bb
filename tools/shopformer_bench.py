#!/usr/bin/env python
"""Shopformer scoring throughput: (a) the fused HIP kernel, (b) the same folded network as torch-ROCm operators on the same GPU
(a restatement in this tool of what moving the reference model to ``device='cuda'`` runs: conv2d, matmul, layer_norm, softmax).

Windows are resident in HBM; the two paths are timed alternately, call by call (hip events around one call, after warm-up); each
cell records the median, min, max and quartiles of ``--reps`` samples, and the worst case for the kernel (its slowest call against
torch's fastest).
Prints one JSON line; ``--out`` also writes it to a file.

    python tools/shopformer_bench.py --out profiles/shopformer_bench.json
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
PEAK_F32_MATRIX_TFLOPS = 157.3


class TorchFolded:
    """the folded score path, operator by operator, batch-first like the reference"""

    def __init__(self, geo, tensors, dev):
        self.g = geo
        self.t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in tensors.items()}
        V = geo["V"]
        adj = np.zeros((V, V), np.float32)
        for v in range(V):
            for c, a in zip(tensors["adj_col"][v].astype(int), tensors["adj_val"][v]):
                adj[v, c] += a
        self.adj = torch.from_numpy(adj).to(dev)

    def lin(self, x, n):
        w = self.t[n + ".w"][:, 0, :]
        return F.linear(x, w, self.t[n + ".b"][:w.shape[0]])

    def mha(self, q_in, kv_in, n):
        d, h = q_in.shape[-1], self.g["heads"]
        q, kv = self.lin(q_in, n + ".q"), self.lin(kv_in, n + ".kv")
        sp = lambda a: a.reshape(a.shape[0], a.shape[1], h, d // h).transpose(1, 2)
        o = F.scaled_dot_product_attention(sp(q), sp(kv[..., :d]), sp(kv[..., d:]))
        return self.lin(o.transpose(1, 2).reshape(q_in.shape), n + ".out")

    def ln(self, x, n):
        d = x.shape[-1]
        return F.layer_norm(x, (d,), self.t[n + ".g"][:d], self.t[n + ".b"][:d], 1e-5)

    @torch.no_grad()
    def __call__(self, x):
        g, t = self.g, self.t
        V, H, L, D = g["V"], g["H"], g["L"], g["D"]
        x = x * t["in_scale"][:2 * V].reshape(1, 2, 1, V) + t["in_shift"][:2 * V].reshape(1, 2, 1, V)
        chans = [2, H, H, H, L]
        for i in range(4):
            s, co = g[f"s{i}"], chans[i + 1]
            res = x
            if f"b{i}.rw" in t:
                res = F.conv2d(x, t[f"b{i}.rw"][:, 0, :, None, None], t[f"b{i}.rb"][:co], stride=(s, 1))
            h = torch.matmul(self.adj, x.permute(0, 2, 3, 1))
            h = torch.relu(torch.matmul(h, t[f"b{i}.gw"][:, 0, :].t()) + t[f"b{i}.gb"][:co]).permute(0, 3, 1, 2).contiguous()
            y = F.conv2d(h, t[f"b{i}.tw"].permute(0, 2, 1)[..., None], t[f"b{i}.tb"][:co], stride=(s, 1), padding=(4, 0))
            x = torch.relu(y + res)
        n = x.shape[0]
        tokens = x.permute(0, 2, 1, 3).reshape(n, g["ntok"], D)
        src = tokens + t["pe_in"]
        for e in range(g["layers"]):
            src = self.ln(src + self.mha(src, src, f"e{e}.sa"), f"e{e}.n1")
            src = self.ln(src + self.lin(torch.relu(self.lin(src, f"e{e}.f1")), f"e{e}.f2"), f"e{e}.n2")
        tgt = torch.cat([torch.zeros_like(tokens[:, :1]), tokens[:, :-1]], 1) + t["pe_in"]
        for e in range(g["layers"]):
            tgt = self.ln(tgt + self.mha(tgt, tgt, f"d{e}.sa"), f"d{e}.n1")
            tgt = self.ln(tgt + self.mha(tgt, src, f"d{e}.ca"), f"d{e}.n2")
            tgt = self.ln(tgt + self.lin(torch.relu(self.lin(tgt, f"d{e}.f1")), f"d{e}.f2"), f"d{e}.n3")
        rec = self.lin(tgt, "proj")
        return ((rec - (tokens + t["pe_score"])) ** 2).mean(dim=(1, 2))


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def timed_pair(fn_a, fn_b, reps, warmup):
    """the two paths ALTERNATED call by call (clock and cache drift hit both alike); -> per path the samples in us"""
    for _ in range(warmup):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    sa, sb = [], []
    for _ in range(reps):
        sa.append(one(fn_a))
        sb.append(one(fn_b))
    return np.asarray(sa), np.asarray(sb)


def stats(us):
    q1, med, q3 = (float(v) for v in np.percentile(us, [25, 50, 75]))
    return {"median": med, "min": float(us.min()), "max": float(us.max()), "q1": q1, "q3": q3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,4096,65536")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from tools import synth_shopformer as R
    from cvsd_amd import Shopformer
    from cvsd_amd import shopformer as SF
    fix = R.load_fixture()
    cfg, sd, x = R.fixture_model(fix, "default")
    model = Shopformer.from_state_dict(sd, cfg, device=0)
    dev = torch.device("cuda:0")
    ref = TorchFolded(*SF.parse_image(SF.image_from_state_dict(sd, cfg)), dev)
    flop = 2 * int(model.info.macs_per_window)
    rows = []
    for n in (int(s) for s in args.sizes.split(",")):
        xd = torch.from_numpy(x[np.arange(n) % len(x)]).to(dev)
        sc = torch.empty(n, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        hip, tor = timed_pair(lambda: model.score_device_async(xd.data_ptr(), n, sc.data_ptr(), stream=stream), lambda: ref(xd),
                              args.reps, args.warmup)
        agree = float((sc - ref(xd)).abs().max())
        h, t = stats(hip), stats(tor)
        rows.append({"n": n, "hip_us": h["median"], "torch_us": t["median"], "hip_us_spread": h, "torch_us_spread": t,
                     "hip_windows_per_s": n / h["median"] * 1e6, "torch_windows_per_s": n / t["median"] * 1e6,
                     "speedup": t["median"] / h["median"], "slowest_hip_vs_fastest_torch": t["min"] / h["max"],
                     "max_abs_diff_vs_torch": agree, "hip_tflops": flop * n / h["median"] / 1e6,
                     "fraction_of_f32_matrix_peak": flop * n / h["median"] / 1e6 / PEAK_F32_MATRIX_TFLOPS})
    out = {"bench": "shopformer_score", "config": cfg, "flop_per_window": flop, "group": int(model.info.group),
           "lds_bytes": int(model.info.lds_bytes), "reps": args.reps, "rows": rows,
           "hip_not_slower_at_every_n": all(r["hip_us"] <= r["torch_us"] for r in rows)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
