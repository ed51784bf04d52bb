"""TEST/BENCH INFRASTRUCTURE -- a seeded synthetic ``shopformer_2`` checkpoint (the paper-aligned variant).

``synthetic_state_dict(config, adj, pe, seed)``: a state dict with the reference's key names and shapes for the score path of the
given nested config (the GCAE decoder, which the score does not depend on, is left out), drawn like tools/synth_shopformer.py draws
the older variant's: weights ~ N(0, 1/fan_in), non-zero biases, BatchNorm statistics away from 0 / 1, gains away from 1, so that
tokens, reconstruction and scores are of order 1.  The adjacency and the positional-encoding table are ARGUMENTS (data of the
reference, stored in tests/golden/shopformer2_fixture.npz).  Nothing is committed: the fixture stores seeds.
"""
from __future__ import annotations

import glob
import os
from typing import Dict

import numpy as np

from cvsd_amd.shopformer import KT, N_BLOCKS, compute_strides_2, resolve_config_2
from tools.synth_shopformer import synthetic_windows as _windows

# the three configs of the fixture: the ``model`` section of the reference's paper_config.yaml, its get_default_config(), and the
# paper config with 24 frames (plain settings; dropout does not act in eval mode and is left out)
CONFIGS = {
    "paper": {"model": {"in_channels": 2, "num_keypoints": 18, "seq_len": 12, "num_tokens": 2,
                        "gcae": {"hidden_channels": 64, "latent_channels": 8, "num_layers": 4},
                        "transformer": {"input_dim": 144, "d_model": 144, "num_heads": 2, "num_layers": 2, "dim_feedforward": 64}}},
    "default24": {"model": {"in_channels": 2, "num_keypoints": 17, "seq_len": 24, "num_tokens": 2,
                            "gcae": {"hidden_channels": 64, "latent_channels": 8, "num_layers": 4},
                            "transformer": {"input_dim": 136, "d_model": 144, "num_heads": 12, "num_layers": 4, "dim_feedforward": 512}}},
    "paper_t24": {"model": {"in_channels": 2, "num_keypoints": 18, "seq_len": 24, "num_tokens": 2,
                            "gcae": {"hidden_channels": 64, "latent_channels": 8, "num_layers": 4},
                            "transformer": {"input_dim": 144, "d_model": 144, "num_heads": 2, "num_layers": 2, "dim_feedforward": 64}}},
}
CONFIG_KEYS = ("in_channels", "num_keypoints", "seq_len", "num_tokens", "gcae.hidden_channels", "gcae.latent_channels", "gcae.num_layers",
               "transformer.input_dim", "transformer.d_model", "transformer.num_heads", "transformer.num_layers",
               "transformer.dim_feedforward")


def nested_config(flat: Dict[str, int]) -> dict:
    """{'seq_len': 12, 'gcae.hidden_channels': 64, ...} -> the nested dict the loader takes"""
    m: dict = {"gcae": {}, "transformer": {}}
    for k, v in flat.items():
        if "." in k:
            a, b = k.split(".")
            m[a][b] = int(v)
        else:
            m[k] = int(v)
    return {"model": m}


def synthetic_state_dict(config: dict, adj: np.ndarray, pe: np.ndarray, seed: int = 0) -> Dict[str, np.ndarray]:
    cfg = resolve_config_2(config)
    rng = np.random.default_rng(seed)
    f32 = np.float32
    V, H, L = cfg["num_keypoints"], cfg["gcae.hidden_channels"], cfg["gcae.latent_channels"]
    Din, D, ff, layers = (cfg["transformer." + k] for k in ("input_dim", "d_model", "dim_feedforward", "num_layers"))
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
    strides = compute_strides_2(cfg["seq_len"], cfg["num_tokens"], N_BLOCKS)[0]
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
        sd[p + "linear1.weight"], sd[p + "linear1.bias"] = w((ff, D), D), b(ff)
        sd[p + "linear2.weight"], sd[p + "linear2.bias"] = w((D, ff), ff), b(D)

    t = "transformer."
    sd[t + "pos_encoder.pe"] = np.asarray(pe, f32).copy()
    if Din != D:
        sd[t + "input_projection.weight"], sd[t + "input_projection.bias"] = w((D, Din), Din), b(D)
        sd[t + "output_projection.weight"], sd[t + "output_projection.bias"] = w((Din, D), D), b(Din)
    for e in range(layers):
        p = f"{t}encoder.layers.{e}."
        attn(p + "self_attn.")
        ffn(p)
        ln(p + "norm1.")
        ln(p + "norm2.")
    ln(t + "encoder.norm.")
    for e in range(layers):
        p = f"{t}decoder.layers.{e}."
        attn(p + "self_attn.")
        attn(p + "multihead_attn.")
        ffn(p)
        ln(p + "norm1.")
        ln(p + "norm2.")
        ln(p + "norm3.")
    ln(t + "decoder.norm.")
    return sd


def synthetic_windows(n: int, config: dict, seed: int = 0) -> np.ndarray:
    cfg = resolve_config_2(config)
    return _windows(n, {"seq_len": cfg["seq_len"], "num_keypoints": cfg["num_keypoints"]}, seed=seed)


GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def load_fixture() -> Dict[str, np.ndarray]:
    """tests/golden/shopformer2_fixture.npz plus its part files (one large array each) as one dict"""
    out = dict(np.load(os.path.join(GOLDEN, "shopformer2_fixture.npz")))
    for p in sorted(glob.glob(os.path.join(GOLDEN, "shopformer2_fixture.*.npz"))):
        out.update(np.load(p))
    return out


def fixture_model(fix, name: str):
    """(nested config, synthetic state dict, windows) of one fixture config, regenerated from its seeds"""
    cfg = nested_config(dict(zip([str(k) for k in fix["config_keys"]], (int(v) for v in fix[name + ".config"]))))
    seed_w, seed_x, n = (int(v) for v in fix[name + ".seeds"])
    sd = synthetic_state_dict(cfg, fix[name + ".adj"], fix[name + ".pe"], seed=seed_w)
    return cfg, sd, synthetic_windows(n, cfg, seed=seed_x)
