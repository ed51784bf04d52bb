#!/usr/bin/env python
"""Generate tests/golden/shopformer_decoder_fixture*.npz -- runs in the BUILD CONTAINER ONLY (it imports the reference).

What it pins: the GCAE decoder of the REFERENCE'S OWN networks (``shopformer/`` and ``shopformer_2/``, ``eval()`` mode) on seeded
synthetic weights: the score-path weights of the existing fixtures (tools/synth_shopformer.py, tools/synth_shopformer2.py) plus
the decoder's (tools/synth_shopformer_decoder.py), so no weight is committed.  For five configs (``shopformer/`` default, kp18_t24,
h32_l4; ``shopformer_2/`` paper, default24) and 64 seeded windows it stores

    tokens_f32 / tokens_f64      ``gcae.encode(windows)`` of the model and of a ``.double()`` copy
    poses_f32 / poses_f64        ``gcae.decode(tokens)`` of each, [64, 2, T, V]
    mse_f32 / mse_f64            the scalar ``F.mse_loss(reconstruction, windows)`` of each
    factors, frames              the decoder's upsample factors as the reference computed them, and the frames its layers emit

Only arrays are stored; nothing of the reference is copied.  Arrays above 64 KiB go one per file,
shopformer_decoder_fixture.<key>.npz, so that no committed file exceeds 1 MiB.

    python tests/golden/make_shopformer_decoder_fixture.py
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "shopformer_decoder_fixture.npz")


def main():
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "shopformer"))
    from models import Shopformer as RefShopformer                        # the reference's own classes, imported where they lie
    from shopformer_2.models.shopformer import build_shopformer
    from cvsd_amd.shopformer import resolve_config
    from tools import synth_shopformer_decoder as SD
    store = {}
    for i, (name, (variant, _)) in enumerate(SD.CONFIGS.items()):
        cfg, sd, x = SD.fixture_model(name, i)
        if variant == 1:
            c = resolve_config(cfg)
            model = RefShopformer(in_channels=2, hidden_channels=c["hidden_channels"], latent_channels=c["latent_channels"],
                                  num_keypoints=c["num_keypoints"], seq_len=c["seq_len"], num_tokens=c["num_tokens"],
                                  transformer_heads=c["transformer_heads"], transformer_layers=c["transformer_layers"], dropout=0.1)
        else:
            model = build_shopformer(copy.deepcopy(cfg))
        full = model.state_dict()
        missing = [k for k in full if k not in sd]
        assert not missing and all(k in full for k in sd), (missing, [k for k in sd if k not in full])
        # the score-path fixtures keep only the first rows of the positional-encoding table: the model keeps its own (the GCAE reads none)
        sd = {k: v for k, v in sd.items() if not k.endswith("pos_encoder.pe")}
        for k, v in sd.items():
            assert tuple(full[k].shape) == tuple(np.asarray(v).shape), (k, full[k].shape, np.asarray(v).shape)
        full.update({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
        model.load_state_dict(full)
        model.eval()
        m64 = copy.deepcopy(model).double()
        with torch.no_grad():
            for sfx, m, xs in (("f32", model, torch.from_numpy(x)), ("f64", m64, torch.from_numpy(x).double())):
                tokens = m.gcae.encode(xs)
                poses = m.gcae.decode(tokens)
                store[f"{name}.tokens_{sfx}"], store[f"{name}.poses_{sfx}"] = tokens.numpy(), poses.numpy()
                store[f"{name}.mse_{sfx}"] = np.asarray(F.mse_loss(poses, xs).item(), np.float64)
        dec = model.gcae.decoder
        convs = [m for m in dec.layers if isinstance(m, (torch.nn.ConvTranspose2d, torch.nn.Conv2d))]
        store[f"{name}.factors"] = np.asarray([m.kernel_size[0] for m in convs], np.int64)
        with torch.no_grad():
            h = dec.initial_proj(torch.from_numpy(store[f"{name}.tokens_f32"]))
            h = h.view(len(x), -1, h.shape[-1] // dec.num_keypoints, dec.num_keypoints).permute(0, 2, 1, 3).contiguous()
            store[f"{name}.frames"] = np.asarray(dec.layers(h).shape[2], np.int64)
        store[f"{name}.seeds"] = np.asarray([SD.SEED_DEC + i, SD.SEED_X + i, SD.N_WINDOWS], np.int64)
        p64 = store[f"{name}.poses_f64"]
        print(f"{name}: tokens {store[f'{name}.tokens_f32'].shape}, poses {p64.shape}, factors {store[f'{name}.factors'].tolist()}, "
              f"frames {int(store[f'{name}.frames'])}, |poses| mean {np.abs(p64).mean():.3f}, mse {float(store[f'{name}.mse_f64']):.4f}, "
              f"fp32 mean err {np.abs(store[f'{name}.poses_f32'] - p64).mean():.2e}")
    big = {k: v for k, v in store.items() if v.nbytes > 65536}
    np.savez_compressed(OUT, **{k: v for k, v in store.items() if k not in big})
    for k, v in big.items():
        part = OUT[:-4] + "." + k + ".npz"
        np.savez_compressed(part, **{k: v})
        assert os.path.getsize(part) < (1 << 20), (part, os.path.getsize(part))
    print(f"wrote {OUT} and {len(big)} part files")


if __name__ == "__main__":
    main()
