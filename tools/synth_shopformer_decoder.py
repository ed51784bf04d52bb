"""TEST/BENCH INFRASTRUCTURE -- seeded synthetic ``gcae.decoder.*`` tensors for a Shopformer config of either variant.

``synthetic_decoder_state_dict(config, seed)``: the reference's key names and shapes for the GCAE decoder (``initial_proj``, four
layers of ``nn.Sequential`` at indices 0, 4, 8, 12 with BatchNorms at 1, 5, 9), drawn like tools/synth_shopformer.py draws the score
path: weights ~ N(0, 1/fan_in), non-zero biases, BatchNorm running mean / variance away from 0 / 1 and gains away from 1, so that
folding is exercised and the reconstruction is of order 1.  tools/synth_shopformer.py and tools/synth_shopformer2.py and what they
emit stay as they are: a full checkpoint is their state dict updated with this one.  Nothing is committed: the fixture stores seeds.
"""
from __future__ import annotations

import glob
import os
from typing import Dict

import numpy as np

from cvsd_amd.shopformer import N_DEC_LAYERS, decoder_factors, is_variant_2, resolve_config, resolve_config_2

# the five configs of tests/golden/shopformer_decoder_fixture*.npz: (fixture the score-path weights come from, its config name)
CONFIGS = {"default": (1, "default"), "kp18_t24": (1, "kp18_t24"), "h32_l4": (1, "h32_l4"), "paper": (2, "paper"), "default24": (2, "default24")}
SEED_DEC, SEED_X, N_WINDOWS = 53, 61, 64


def decoder_dims(config) -> Dict[str, int]:
    if is_variant_2(config):
        c = resolve_config_2(config)
        return {"V": c["num_keypoints"], "T": c["seq_len"], "H": c["gcae.hidden_channels"], "L": c["gcae.latent_channels"], "num_tokens": c["num_tokens"]}
    c = resolve_config(config)
    return {"V": c["num_keypoints"], "T": c["seq_len"], "H": c["hidden_channels"], "L": c["latent_channels"], "num_tokens": c["num_tokens"]}


def synthetic_decoder_state_dict(config, seed: int = 0) -> Dict[str, np.ndarray]:
    d = decoder_dims(config)
    V, H, L = d["V"], d["H"], d["L"]
    rng = np.random.default_rng(seed)
    f32 = np.float32
    sd: Dict[str, np.ndarray] = {}
    p = "gcae.decoder."
    sd[p + "initial_proj.weight"] = (rng.standard_normal((H * V, L * V)) / np.sqrt(L * V)).astype(f32)
    sd[p + "initial_proj.bias"] = (rng.standard_normal(H * V) * 0.1).astype(f32)
    factors = decoder_factors(d["num_tokens"], d["T"])
    for i in range(N_DEC_LAYERS):
        co, q = (H if i < N_DEC_LAYERS - 1 else 2), f"{p}layers.{4 * i}."
        shape = (H, co, factors[i], 1) if factors[i] > 1 else (co, H, 1, 1)
        sd[q + "weight"] = (rng.standard_normal(shape) * np.sqrt(2.0 / H)).astype(f32)
        sd[q + "bias"] = (rng.standard_normal(co) * 0.1).astype(f32)
        if i < N_DEC_LAYERS - 1:
            q = f"{p}layers.{4 * i + 1}."
            sd[q + "weight"] = rng.uniform(0.7, 1.3, co).astype(f32)
            sd[q + "bias"] = (rng.standard_normal(co) * 0.2).astype(f32)
            sd[q + "running_mean"] = (rng.standard_normal(co) * 0.2).astype(f32)
            sd[q + "running_var"] = rng.uniform(0.6, 1.6, co).astype(f32)
            sd[q + "num_batches_tracked"] = np.asarray(100, np.int64)
    return sd


GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def load_fixture() -> Dict[str, np.ndarray]:
    """tests/golden/shopformer_decoder_fixture.npz plus its part files (one large array each) as one dict"""
    out = dict(np.load(os.path.join(GOLDEN, "shopformer_decoder_fixture.npz")))
    for p in sorted(glob.glob(os.path.join(GOLDEN, "shopformer_decoder_fixture.*.npz"))):
        out.update(np.load(p))
    return out


def fixture_model(name: str, i: int = None):
    """(config, full synthetic state dict = the score-path fixture's weights + the decoder's, the fixture's 64 windows) of one of the
    five configs, regenerated from seeds"""
    from tools import synth_shopformer as S1
    from tools import synth_shopformer2 as S2
    variant, src = CONFIGS[name]
    S = S1 if variant == 1 else S2
    cfg, sd, _ = S.fixture_model(S.load_fixture(), src)
    i = list(CONFIGS).index(name) if i is None else i
    sd = dict(sd)
    sd.update(synthetic_decoder_state_dict(cfg, seed=SEED_DEC + i))
    return cfg, sd, S.synthetic_windows(N_WINDOWS, cfg, seed=SEED_X + i)
