"""TEST/BENCH INFRASTRUCTURE -- a seeded synthetic Shopformer checkpoint and seeded pose windows.

``synthetic_state_dict(config, adj, pe, seed)``: a state dict with the reference's key names and shapes for the score path of the
given config (the GCAE decoder, which the score does not depend on, is left out), drawn from ``numpy.random.default_rng(seed)``:
weights ~ N(0, 1/fan_in), non-zero biases, BatchNorm running mean / variance away from 0 / 1, BatchNorm and LayerNorm gains away
from 1.  The two buffers a checkpoint carries -- the normalised skeleton adjacency and the positional-encoding table -- are
ARGUMENTS: they are data of the reference (stored in tests/golden/shopformer_fixture.npz), not something this generator restates.
"""
from __future__ import annotations

import glob
import os
from typing import Dict

import numpy as np

from cvsd_amd.shopformer import FF_DIM, KT, N_BLOCKS, block_strides, resolve_config


def synthetic_state_dict(config, adj: np.ndarray, pe: np.ndarray, seed: int = 0) -> Dict[str, np.ndarray]:
    cfg = resolve_config(config)
    rng = np.random.default_rng(seed)
    f32 = np.float32
    V, H, L = cfg["num_keypoints"], cfg["hidden_channels"], cfg["latent_channels"]
    D = L * V
    sd: Dict[str, np.ndarray] = {}

    def bn(p, c):
        sd[p + ".weight"] = rng.uniform(0.7, 1.3, c).astype(f32)
        sd[p + ".bias"] = (rng.standard_normal(c) * 0.2).astype(f32)
        sd[p + ".running_mean"] = (rng.standard_normal(c) * 0.2).astype(f32)
        sd[p + ".running_var"] = rng.uniform(0.6, 1.6, c).astype(f32)
        sd[p + ".num_batches_tracked"] = np.asarray(100, np.int64)

    def w(shape, fan_in):
        return (rng.standard_normal(shape) / np.sqrt(fan_in)).astype(f32)

    def b(c):
        return (rng.standard_normal(c) * 0.1).astype(f32)

    enc = "gcae.encoder."
    bn(enc + "bn_input", 2 * V)
    chans = [2, H, H, H, L]
    strides = block_strides(cfg["seq_len"], cfg["num_tokens"])
    for i in range(N_BLOCKS):
        p, ci, co = f"{enc}layers.{i}.", chans[i], chans[i + 1]
        sd[p + "gcn.weight"], sd[p + "gcn.bias"] = w((ci, co), ci) * f32(1.5), b(co)
        sd[p + "gcn.adj"] = np.asarray(adj, f32).copy()
        sd[p + "tcn.conv.weight"], sd[p + "tcn.conv.bias"] = w((co, co, KT, 1), co * 3), b(co)
        bn(p + "tcn.bn", co)
        if ci != co or strides[i] != 1:
            sd[p + "residual.0.weight"], sd[p + "residual.0.bias"] = w((co, ci, 1, 1), ci), b(co)
            bn(p + "residual.1", co)

    def attn(p):
        sd[p + "in_proj_weight"], sd[p + "in_proj_bias"] = w((3 * D, D), D), b(3 * D)
        sd[p + "out_proj.weight"], sd[p + "out_proj.bias"] = w((D, D), D), b(D)

    def ln(p):
        sd[p + "weight"], sd[p + "bias"] = rng.uniform(0.7, 1.3, D).astype(f32), b(D)

    def ffn(p):
        sd[p + "linear1.weight"], sd[p + "linear1.bias"] = w((FF_DIM, D), D), b(FF_DIM)
        sd[p + "linear2.weight"], sd[p + "linear2.bias"] = w((D, FF_DIM), FF_DIM), b(D)

    sd["transformer.pos_encoder.pe"] = np.asarray(pe, f32).copy()
    for e in range(cfg["transformer_layers"]):
        p = f"transformer.encoder_layers.{e}."
        attn(p + "self_attn.")
        ffn(p)
        ln(p + "norm1.")
        ln(p + "norm2.")
    for e in range(cfg["transformer_layers"]):
        p = f"transformer.decoder_layers.{e}."
        attn(p + "self_attn.")
        attn(p + "multihead_attn.")
        ffn(p)
        ln(p + "norm1.")
        ln(p + "norm2.")
        ln(p + "norm3.")
    sd["transformer.output_proj.weight"], sd["transformer.output_proj.bias"] = w((D, D), D), b(D)
    sd["pos_encoder.pe"] = np.asarray(pe, f32).copy()
    return sd


def synthetic_windows(n: int, config=None, seed: int = 0) -> np.ndarray:
    """[n, 2, T, V] float32 in [-1, 1]: a per-window random pose plus a smooth drift over time and a little per-frame jitter"""
    cfg = resolve_config(config)
    rng = np.random.default_rng(seed)
    T, V = cfg["seq_len"], cfg["num_keypoints"]
    base = rng.uniform(-0.7, 0.7, (n, 2, 1, V))
    drift = rng.uniform(-0.2, 0.2, (n, 2, 1, 1)) * np.linspace(-1, 1, T).reshape(1, 1, T, 1)
    x = base + drift + rng.standard_normal((n, 2, T, V)) * 0.05
    return np.clip(x, -1, 1).astype(np.float32)


GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def load_fixture() -> Dict[str, np.ndarray]:
    """tests/golden/shopformer_fixture.npz plus its part files (one large array each) as one dict"""
    out = dict(np.load(os.path.join(GOLDEN, "shopformer_fixture.npz")))
    for p in sorted(glob.glob(os.path.join(GOLDEN, "shopformer_fixture.*.npz"))):
        out.update(np.load(p))
    return out


def fixture_model(fix, name: str):
    """(config dict, synthetic state dict, windows) of one fixture config, regenerated from its seeds"""
    cfg = dict(zip([str(k) for k in fix["config_keys"]], (int(v) for v in fix[name + ".config"])))
    seed_w, seed_x, n = (int(v) for v in fix[name + ".seeds"])
    sd = synthetic_state_dict(cfg, fix[name + ".adj"], fix[name + ".pe"], seed=seed_w)
    return cfg, sd, synthetic_windows(n, cfg, seed=seed_x)
