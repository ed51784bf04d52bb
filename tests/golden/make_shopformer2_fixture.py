#!/usr/bin/env python
"""Generate tests/golden/shopformer2_fixture*.npz -- runs in the BUILD CONTAINER ONLY (it imports the reference).

What it pins: the REFERENCE'S OWN ``shopformer_2`` network (``build_shopformer`` in ``eval()`` mode), evaluated on seeded synthetic
weights and windows (tools/synth_shopformer2.py, so no weight is committed).  Per config (``paper``, ``default24``, ``paper_t24``):

    adj, pe                              the two buffers of a freshly built reference model (data the generator must not restate)
    config, seeds                        integers
    tokens / recon / score / token_scores    the reference's outputs in float32, and those of a ``.double()`` copy in float64
                                         (score = compute_anomaly_score(reduction='mean'), token_scores = reduction='none')

for the paper config also the same outputs for ``s2_test_xy_x`` of tests/golden/poselift_fixture.npz (prefix ``poselift_``); the
results of the reference's ``_compute_strides`` for seq_len in {12, 24, 36, 48} x num_tokens in {2, 3, 4}
(``strides_table``: seq_len, num_tokens, four strides, final length, pooling flag); and hand-made poses with their
``add_neck_keypoint`` outputs (``neck_in`` / ``neck_out``: both shoulders, left missing, right missing, both missing, 15 joints).
Only arrays are stored; nothing of the reference is copied.  Arrays above 64 KiB go one per file, shopformer2_fixture.<key>.npz.

    python tests/golden/make_shopformer2_fixture.py
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "shopformer2_fixture.npz")
N_WINDOWS, SEED_W, SEED_X = 256, 23, 31


def outputs(model, x):
    with torch.no_grad():
        _, tokens, recon = model(x, return_all=True)
        return {"tokens": tokens.numpy(), "recon": recon.numpy(), "score": model.compute_anomaly_score(x, "mean").numpy(),
                "token_scores": model.compute_anomaly_score(x, "none").numpy()}


def main():
    sys.path.insert(0, REF)
    from shopformer_2.models.shopformer import build_shopformer          # the reference's own builder, imported where it lies
    from shopformer_2.models.gcae import GCAEEncoder
    from shopformer_2.data.poselift_dataset import add_neck_keypoint
    from cvsd_amd.shopformer import resolve_config_2
    from tools import synth_shopformer2 as S
    store = {}
    for i, (name, cfg) in enumerate(S.CONFIGS.items()):
        ref_cfg = copy.deepcopy(cfg)
        model = build_shopformer(ref_cfg)
        adj = model.gcae.encoder.layers[0].gcn.adj.numpy().copy()
        pe = model.transformer.pos_encoder.pe.numpy().copy()
        sd = S.synthetic_state_dict(cfg, adj, pe, seed=SEED_W + i)
        full = model.state_dict()
        missing = [k for k in full if k not in sd and not k.startswith("gcae.decoder.")]
        assert not missing and all(k in full for k in sd), (missing, [k for k in sd if k not in full])
        full.update({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        model.load_state_dict(full)
        model.eval()
        sets = {"": S.synthetic_windows(N_WINDOWS, cfg, seed=SEED_X + i)}
        if name == "paper":
            sets["poselift_"] = np.load(os.path.join(ROOT, "tests", "golden", "poselift_fixture.npz"))["s2_test_xy_x"]
        m64 = copy.deepcopy(model).double()
        for tag, xs in sets.items():
            for sfx, o in (("f32", outputs(model, torch.from_numpy(xs))), ("f64", outputs(m64, torch.from_numpy(xs).double()))):
                for k, v in o.items():
                    store[f"{name}.{tag}{k}_{sfx}"] = v
        flat = resolve_config_2(cfg)
        store[f"{name}.adj"], store[f"{name}.pe"] = adj, pe[:, :8]          # only the first rows of the table are ever read
        store[f"{name}.config"] = np.asarray([flat[k] for k in S.CONFIG_KEYS], np.int64)
        store[f"{name}.seeds"] = np.asarray([SEED_W + i, SEED_X + i, N_WINDOWS], np.int64)
        s = store[f"{name}.score_f64"]
        print(f"{name}: tokens {store[f'{name}.tokens_f32'].shape}, score {s.min():.3f} .. {s.max():.3f}, "
              f"fp32 mean err {np.abs(store[f'{name}.score_f32'] - s).mean():.2e}")
    store["config_keys"] = np.asarray(S.CONFIG_KEYS)
    rows = []
    for T in (12, 24, 36, 48):
        for nt in (2, 3, 4):
            e = GCAEEncoder.__new__(GCAEEncoder)                              # the rule is a method that reads nothing but its arguments
            st = GCAEEncoder._compute_strides(e, T, nt, 4)
            rows.append([T, nt, *st, e._final_len, int(e._needs_pooling)])
    store["strides_table"] = np.asarray(rows, np.int64)
    rng = np.random.default_rng(41)
    poses = rng.uniform(10, 200, (5, 17, 3))
    poses[1, 5, :2] = 0
    poses[2, 6, :2] = 0
    poses[3, 5, :2] = 0
    poses[3, 6, :2] = 0
    poses[4, 15:] = 0                                                         # delivered as 15 joints below
    store["neck_in"] = poses
    store["neck_out"] = np.stack([add_neck_keypoint(p if j != 4 else p[:15]) for j, p in enumerate(poses)])
    big = {k: v for k, v in store.items() if v.nbytes > 65536}
    np.savez_compressed(OUT, **{k: v for k, v in store.items() if k not in big})
    for k, v in big.items():
        part = OUT[:-4] + "." + k + ".npz"
        np.savez_compressed(part, **{k: v})
        assert os.path.getsize(part) < (1 << 20), (part, os.path.getsize(part))
    print(f"wrote {OUT} and {len(big)} part files")


if __name__ == "__main__":
    main()
