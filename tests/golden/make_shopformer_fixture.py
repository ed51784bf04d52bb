#!/usr/bin/env python
"""Generate tests/golden/shopformer_fixture.npz -- runs in the BUILD CONTAINER ONLY (it imports the reference).

What it pins: the REFERENCE'S OWN network, ``/root/reference/shopformer/models`` (``Shopformer`` in ``eval()`` mode), evaluated on
seeded synthetic weights and windows (tools/synth_shopformer.py, so no weight is committed).  Per config it stores

    adj, pe                  the two buffers of a freshly built reference model (data the generator must not restate)
    tokens / recon / score   the reference's outputs in float32, and those of a ``.double()`` copy of the same model in float64

for the default config and two others, plus the reference's scores (default config) for the windows the reference loader cut from
the bridge dict in tests/golden/poselift_fixture.npz (``train_xy_x``).  Only arrays are stored; nothing of the reference is copied.  Arrays above 64 KiB are written one per file,
shopformer_fixture.<key>.npz, so that no committed file exceeds 1 MiB.

    python tests/golden/make_shopformer_fixture.py
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = "/root/reference/shopformer"
OUT = os.path.join(ROOT, "tests", "golden", "shopformer_fixture.npz")

CONFIGS = {
    "default": {},
    "kp18_t24": {"num_keypoints": 18, "seq_len": 24},
    "h32_l4": {"hidden_channels": 32, "latent_channels": 4, "transformer_heads": 4, "transformer_layers": 1},
}
N_WINDOWS, SEED_W, SEED_X = 256, 7, 11


def main():
    sys.path.insert(0, REF)
    from models import Shopformer as RefShopformer          # the reference's own class, imported where it lies
    from cvsd_amd.shopformer import resolve_config
    from tools import synth_shopformer as S
    store = {}
    for i, (name, over) in enumerate(CONFIGS.items()):
        cfg = resolve_config(over)
        model = RefShopformer(in_channels=2, hidden_channels=cfg["hidden_channels"], latent_channels=cfg["latent_channels"],
                              num_keypoints=cfg["num_keypoints"], seq_len=cfg["seq_len"], num_tokens=cfg["num_tokens"],
                              transformer_heads=cfg["transformer_heads"], transformer_layers=cfg["transformer_layers"], dropout=0.1)
        adj = model.gcae.encoder.layers[0].gcn.adj.numpy().copy()
        pe = model.pos_encoder.pe.numpy().copy()
        assert np.array_equal(pe, model.transformer.pos_encoder.pe.numpy())
        sd = S.synthetic_state_dict(cfg, adj, pe, seed=SEED_W + i)
        full = model.state_dict()
        missing = [k for k in full if k not in sd and not k.startswith("gcae.decoder.")]
        assert not missing and all(k in full for k in sd), (missing, [k for k in sd if k not in full])
        full.update({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        model.load_state_dict(full)
        model.eval()
        x = S.synthetic_windows(N_WINDOWS, cfg, seed=SEED_X + i)
        sets = {"": x}
        if name == "default":
            sets["poselift_"] = np.load(os.path.join(ROOT, "tests", "golden", "poselift_fixture.npz"))["train_xy_x"]
        m64 = copy.deepcopy(model).double()
        for tag, xs in sets.items():
            with torch.no_grad():
                o32 = model(torch.from_numpy(xs), return_tokens=True)
                o64 = m64(torch.from_numpy(xs).double(), return_tokens=True)
            for sfx, o in (("f32", o32), ("f64", o64)):
                store[f"{name}.{tag}tokens_{sfx}"] = o["tokens"].numpy()
                store[f"{name}.{tag}recon_{sfx}"] = o["reconstructed_tokens"].numpy()
                store[f"{name}.{tag}score_{sfx}"] = o["normality_score"].numpy()
        store[f"{name}.adj"], store[f"{name}.pe"] = adj, pe[:, :8]          # only the first rows of the table are ever read
        store[f"{name}.config"] = np.asarray([cfg[k] for k in sorted(cfg)], np.int64)
        store[f"{name}.seeds"] = np.asarray([SEED_W + i, SEED_X + i, N_WINDOWS], np.int64)
        s = store[f"{name}.score_f64"]
        print(f"{name}: tokens {store[f'{name}.tokens_f32'].shape}, score {s.min():.3f} .. {s.max():.3f}")
    store["config_keys"] = np.asarray(sorted(resolve_config(None)))
    # no committed file may exceed 1 MiB: the big arrays go one per file (tools/synth_shopformer.py:load_fixture merges them)
    big = {k: v for k, v in store.items() if v.nbytes > 65536}
    np.savez_compressed(OUT, **{k: v for k, v in store.items() if k not in big})
    for k, v in big.items():
        part = OUT[:-4] + "." + k + ".npz"
        np.savez_compressed(part, **{k: v})
        assert os.path.getsize(part) < (1 << 20), (part, os.path.getsize(part))
    print(f"wrote {OUT} and {len(big)} part files")


if __name__ == "__main__":
    main()
