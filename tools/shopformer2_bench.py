#!/usr/bin/env python
"""shopformer_2 scoring throughput: (a) the two fused HIP launches, (b) the same folded network as torch-ROCm
operators on the same GPU (conv2d, matmul, layer_norm, scaled_dot_product_attention, erf gelu) -- the baseline is not the code
under test.  Same method as tools/shopformer_bench.py: windows resident in HBM, the two paths alternated call by call, hip events
around one call, median / min / max / quartiles of ``--reps`` samples per cell.  Configs ``paper`` and ``default24``.

``--row-groups 16,8,3``: the row-group A/B.  Each value is measured in a fresh child process (the handle reads the experiment
variable MI355_SF2_ROW_GROUP once, at create); only the HIP path is timed there.

    python tools/shopformer2_bench.py --out profiles/shopformer2_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.shopformer_bench import PEAK_F32_MATRIX_TFLOPS, TorchFolded, one, stats, timed_pair  # noqa: E402


class TorchFolded2(TorchFolded):
    """the folded shopformer_2 score path, operator by operator, batch-first like the reference"""

    def tokens(self, x):
        g, t = self.g, self.t
        V, H, L = g["V"], g["H"], g["L"]
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
        return x.permute(0, 2, 1, 3).reshape(x.shape[0], g["ntok"], L * V)

    @torch.no_grad()
    def __call__(self, x):
        g, t = self.g, self.t
        tokens = self.tokens(x)
        x0 = (self.lin(tokens, "inp") if g["in_proj"] else tokens) + t["pe_in"]
        src = x0
        for e in range(g["layers"]):
            y = self.ln(src, f"e{e}.n1")
            src = src + self.mha(y, y, f"e{e}.sa")
            src = src + self.lin(F.gelu(self.lin(self.ln(src, f"e{e}.n2"), f"e{e}.f1")), f"e{e}.f2")
        mem = self.ln(src, "en")
        tgt = x0
        for e in range(g["layers"]):
            y = self.ln(tgt, f"d{e}.n1")
            tgt = tgt + self.mha(y, y, f"d{e}.sa")
            tgt = tgt + self.mha(self.ln(tgt, f"d{e}.n2"), mem, f"d{e}.ca")
            tgt = tgt + self.lin(F.gelu(self.lin(self.ln(tgt, f"d{e}.n3"), f"d{e}.f1")), f"d{e}.f2")
        rec = self.ln(tgt, "dn")
        if g["out_proj"]:
            rec = self.lin(rec, "outp")
        return ((tokens - rec) ** 2).mean(dim=(1, 2))


def bench_config(name, sizes, reps, warmup, hip_only=False):
    from tools import synth_shopformer2 as R
    from cvsd_amd import Shopformer
    from cvsd_amd import shopformer as SF
    fix = R.load_fixture()
    cfg, sd, x = R.fixture_model(fix, name)
    model = Shopformer.from_state_dict(sd, cfg, device=0)
    dev = torch.device("cuda:0")
    ref = None if hip_only else TorchFolded2(*SF.parse_image(SF.image_from_state_dict(sd, cfg)), dev)
    flop = 2 * int(model.info.macs_per_window)
    rows = []
    for n in sizes:
        xd = torch.from_numpy(x[np.arange(n) % len(x)]).to(dev)
        sc = torch.empty(n, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        run = lambda: model.score_device_async(xd.data_ptr(), n, sc.data_ptr(), stream=stream)
        if hip_only:
            for _ in range(warmup):
                run()
            torch.cuda.synchronize()
            h = stats(np.asarray([one(run) for _ in range(reps)]))
            rows.append({"n": n, "hip_us": h["median"], "hip_us_spread": h, "hip_tflops": flop * n / h["median"] / 1e6})
            continue
        hip, tor = timed_pair(run, lambda: ref(xd), reps, warmup)
        agree = float((sc - ref(xd)).abs().max())
        h, t = stats(hip), stats(tor)
        rows.append({"n": n, "hip_us": h["median"], "torch_us": t["median"], "hip_us_spread": h, "torch_us_spread": t,
                     "hip_windows_per_s": n / h["median"] * 1e6, "torch_windows_per_s": n / t["median"] * 1e6,
                     "speedup": t["median"] / h["median"], "slowest_hip_vs_fastest_torch": t["min"] / h["max"],
                     "max_abs_diff_vs_torch": agree, "hip_tflops": flop * n / h["median"] / 1e6,
                     "fraction_of_f32_matrix_peak": flop * n / h["median"] / 1e6 / PEAK_F32_MATRIX_TFLOPS})
    return {"config": name, "flop_per_window": flop, "group": int(model.info.group), "row_group": int(model.info.group_transformer),
            "lds_bytes": int(model.info.lds_bytes), "launches_per_call": 2, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,4096,65536")
    ap.add_argument("--configs", default="paper,default24")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--row-groups", default="", help="comma list: also time the HIP path with these transformer row groups (child processes)")
    ap.add_argument("--hip-only", action="store_true", help="(child of --row-groups) time the HIP path alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    cells = [bench_config(c, sizes, args.reps, args.warmup, args.hip_only) for c in args.configs.split(",")]
    out = {"bench": "shopformer2_score", "reps": args.reps, "configs": cells}
    if not args.hip_only:
        out["hip_faster_at_every_n"] = all(r["speedup"] > 1 for c in cells for r in c["rows"])
    if args.row_groups:
        ab = {}
        for g in args.row_groups.split(","):
            env = dict(os.environ, MI355_SF2_ROW_GROUP=g)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--hip-only", "--sizes", args.sizes, "--configs", args.configs,
                                "--reps", str(args.reps), "--warmup", str(args.warmup)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"row group {g}: exit {r.returncode}\n{r.stderr[-2000:]}")
            ab[g] = json.loads(r.stdout.strip().splitlines()[-1])["configs"]
        out["row_group_ab"] = ab
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
