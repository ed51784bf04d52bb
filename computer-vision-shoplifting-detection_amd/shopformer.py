"""Shopformer inference: pose windows -> anomaly score, the network of the reference's ``shopformer/`` in ``eval()`` mode as ONE
fused HIP launch (csrc/shopformer_kernels.hip).

Only what ``normality_score`` depends on is evaluated: ``bn_input`` -> 4 ST-GCN blocks -> tokens ``[N, 3, latent*V]`` -> positional
encoding -> post-norm transformer encoder / decoder (no causal mask) -> ``output_proj`` -> mean squared error against
``tokens + PE``.  The GCAE decoder is not part of the score; it is loaded only when asked for (``decoder=True``, below).

A second variant, the reference's ``shopformer_2/`` network (pre-norm ``nn.Transformer`` layers, erf GELU, two real tokens, optional
input / output projection, per-token scores), is loaded by the same functions: a nested config dict with a ``model``
key, or ``variant=2``, selects it.  It runs as two launches: the tokenizer, then the transformer over row groups of 16 windows.

With ``decoder=True`` the loader also folds ``gcae.decoder.*`` (``initial_proj``, four (transposed) convolutions with their
BatchNorms, linear interpolation along time when the layers emit fewer frames than ``seq_len``) into a version-3 image, and the
model gains the reference's fourth output: ``forward(x, poses=True)`` adds ``gcae_reconstructed`` (``reconstructed_poses`` under
``shopformer_2``'s name) and ``pose_error``, ``decode(tokens)`` runs the decoder alone; one more HIP launch.

This module holds (a) the loader: reference-named state dict -> folded tensors -> a small self-describing weight image whose
matrices are already in the kernel's MFMA fragment order, (b) ``Shopformer``, the ctypes front of ``mi355_shopformer_*``, and (c) the
host side between the tracker and the network: ``windows_from_poselift``, ``score_poselift``, ``StreamScorer``, and their forms that
build the windows on the device (csrc/pose_windows.hip): ``Shopformer.score_poses``, ``score_poselift(on_device=True)``,
``score_poselift_many``, ``MultiStreamScorer``.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import struct
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib

MAGIC = b"MI355SF1"
IMAGE_VERSION = 1
BN_EPS = 1e-5
KT = 9                      # temporal kernel of every ST-GCN block (pad 4)
N_BLOCKS = 4
FF_DIM = 64                 # inference.py builds the model with the default transformer_ff_dim
DEFAULT_CONFIG = {"seq_len": 12, "num_keypoints": 17, "num_tokens": 2, "hidden_channels": 64, "latent_channels": 8,
                  "transformer_heads": 2, "transformer_layers": 2}
SUPPORTED = {"num_keypoints": (17, 18), "seq_len": (12, 24), "hidden_channels": (32, 64), "latent_channels": (4, 8),
             "transformer_heads": (1, 2, 4), "transformer_layers": (1, 2, 3, 4), "num_tokens": (2,)}
CFG_FIELDS = ("V", "T", "H", "L", "heads", "layers", "ff", "D", "ntok", "nnz", "s0", "s1", "s2", "s3", "T1", "T2", "T3", "T4")
# version-2 images (the shopformer_2 variant) carry six more ints; D is d_model, Din = latent_channels * num_keypoints the token width
IMAGE_VERSION_2 = 2
CFG_FIELDS_V2 = CFG_FIELDS + ("variant", "Din", "in_proj", "out_proj", "norm_kind", "act_kind")
NORM_POST, NORM_PRE = 0, 1
ACT_RELU, ACT_GELU_ERF = 0, 1
# TransformerConfig's defaults in the reference, used for keys the ``model.transformer`` section leaves out
DEFAULT_TRANSFORMER_2 = {"input_dim": 144, "d_model": 144, "num_heads": 12, "num_layers": 4, "dim_feedforward": 64}
SUPPORTED_2 = {"num_keypoints": (17, 18), "seq_len": (12, 24), "gcae.hidden_channels": (32, 64), "gcae.latent_channels": (4, 8),
               "num_tokens": (2,), "in_channels": (2,), "gcae.num_layers": (4,), "transformer.num_layers": (1, 2, 3, 4)}
MAX_FF_2, MAX_D_MODEL_2 = 512, 144
KIND_PLAIN, KIND_PACKED = 0, 1
# version-3 images: either variant plus its GCAE decoder; all of a version-2 header's ints (variant 1: variant = 1, Din = D, no
# projections, post-norm, ReLU) and six more: the decoder's four upsample factors, the frames its layers emit, the interpolation flag
IMAGE_VERSION_3 = 3
CFG_FIELDS_V3 = CFG_FIELDS_V2 + ("u0", "u1", "u2", "u3", "Tdec", "interp")
N_DEC_LAYERS = 4


def decoder_factors(num_tokens: int, seq_len: int, num_layers: int = N_DEC_LAYERS) -> List[int]:
    """the decoder's upsample rule: from the CONFIG's ``num_tokens`` (not the token count the encoder really emits), double per layer
    while the doubled length still fits ``seq_len``.  2 -> 12: [2, 2, 1, 1]; 2 -> 24: [2, 2, 2, 1]"""
    f, cur = [1] * num_layers, num_tokens
    for i in range(num_layers):
        if cur >= seq_len:
            break
        if cur * 2 <= seq_len:
            f[i], cur = 2, cur * 2
    return f


def _fold_decoder(sd, need, t: Dict[str, np.ndarray], geo: dict, num_tokens: int) -> None:
    """``gcae.decoder.*`` into ``t`` and the six decoder ints into ``geo``.  ``dec.ip``: initial_proj with its output features
    reordered from (channel, joint) to (joint, channel), so that a (window, token) row of its output is V rows of H channels;
    ``dec.l{i}.w``: [out, parity, in], the BatchNorm behind the layer folded in (float64); the last layer has 2 outputs and no norm."""
    V, T, H, L, ntok = geo["V"], geo["T"], geo["H"], geo["L"], geo["ntok"]
    f = decoder_factors(num_tokens, T)
    frames = ntok * int(np.prod(f))
    if f[-1] != 1 or frames > T:
        raise ValueError(f"Shopformer decoder: upsample factors {f} on {ntok} tokens give {frames} frames for seq_len = {T}; a last layer "
                         f"that upsamples and more frames than seq_len are not supported")
    dec = "gcae.decoder."
    w = need(dec + "initial_proj.weight", (H * V, L * V)).reshape(H, V, L * V).transpose(1, 0, 2)
    t["dec.ip.w"] = w.reshape(V * H, 1, L * V)
    t["dec.ip.b"] = need(dec + "initial_proj.bias", (H * V,)).reshape(H, V).T.reshape(-1)
    for i in range(N_DEC_LAYERS):
        co, p = (H if i < N_DEC_LAYERS - 1 else 2), f"{dec}layers.{4 * i}."
        if f[i] > 1:
            w = need(p + "weight", (H, co, f[i], 1))[..., 0].transpose(1, 2, 0)              # ConvTranspose2d [in, out, k, 1] -> [out, k, in]
        else:
            w = need(p + "weight", (co, H, 1, 1))[:, :, 0, 0].reshape(co, 1, H)
        b = need(p + "bias", (co,))
        if i < N_DEC_LAYERS - 1:
            need(f"{dec}layers.{4 * i + 1}.weight", (co,))
            for k in ("bias", "running_mean", "running_var"):
                need(f"{dec}layers.{4 * i + 1}.{k}", (co,))
            g, sh = _bn(sd, f"{dec}layers.{4 * i + 1}")
            w, b = w * g[:, None, None], b * g + sh
        t[f"dec.l{i}.w"], t[f"dec.l{i}.b"] = w, b
    geo.update({"u0": f[0], "u1": f[1], "u2": f[2], "u3": f[3], "Tdec": frames, "interp": int(frames != T)})
    if "variant" not in geo:
        geo.update({"variant": 1, "Din": geo["D"], "in_proj": 0, "out_proj": 0, "norm_kind": NORM_POST, "act_kind": ACT_RELU})


def resolve_config(config: Optional[dict]) -> dict:
    """config.json as inference.py reads it (missing keys take its defaults); anything the kernel does not cover is refused by name"""
    cfg = dict(DEFAULT_CONFIG)
    for k, v in (config or {}).items():
        if k in cfg:
            cfg[k] = int(v)
    for field, allowed in SUPPORTED.items():
        if cfg[field] not in allowed:
            raise ValueError(f"Shopformer config field '{field}' = {cfg[field]} is not supported (supported: {list(allowed)})")
    d = cfg["latent_channels"] * cfg["num_keypoints"]
    if d % cfg["transformer_heads"]:
        raise ValueError(f"Shopformer config field 'transformer_heads' = {cfg['transformer_heads']} does not divide "
                         f"latent_channels * num_keypoints = {d}")
    return cfg


def block_strides(seq_len: int, num_tokens: int, n_blocks: int = N_BLOCKS) -> List[int]:
    """temporal stride of each ST-GCN block: halve while the halved length still holds ``num_tokens`` frames.  12 -> 6 -> 3 stops at 3
    (3 // 2 < 2), so the default model emits THREE tokens per window although the parameter says two."""
    s, t = [], seq_len
    for _ in range(n_blocks):
        if t > num_tokens and t // 2 >= num_tokens:
            s.append(2)
            t //= 2
        else:
            s.append(1)
    return s


def compute_strides_2(seq_len: int, num_tokens: int, num_layers: int = N_BLOCKS) -> Tuple[List[int], int, bool]:
    """the shopformer_2 tokenizer's stride rule -> (strides, final length, needs the adaptive pool).  ``seq_len // num_tokens`` is
    divided by 2, 3, 4, 5, 6 in turn as often as each goes; what is left above 1 is one more factor.  The smallest ``num_layers``
    factors become strides, largest first.  12 / 2 -> [3, 2, 1, 1], 24 / 2 -> [3, 2, 2, 1].  The final length is the floor
    division chain; the pool is needed when it misses ``num_tokens``."""
    strides = [1] * num_layers
    remaining, factors = seq_len // num_tokens, []
    for p in (2, 3, 4, 5, 6):
        while remaining % p == 0 and remaining > 1:
            factors.append(p)
            remaining //= p
    if remaining > 1:
        factors.append(remaining)
    for i, f in enumerate(sorted(factors)[:num_layers]):
        strides[i] = f
    strides.sort(reverse=True)
    final = seq_len
    for s in strides:
        final //= s
    return strides, final, final != num_tokens


def is_variant_2(config) -> bool:
    return isinstance(config, dict) and isinstance(config.get("model"), dict)


def resolve_config_2(config: dict) -> dict:
    """the nested ``shopformer_2`` config (``model``, ``model.gcae``, ``model.transformer``) -> a flat dict of ints with dotted keys;
    whatever the kernel does not cover is refused with the field named, before any image is built"""
    if not is_variant_2(config):
        raise ValueError("a shopformer_2 config is a nested dict with a 'model' section")
    m = config["model"]
    g, tr = m.get("gcae") or {}, m.get("transformer") or {}
    cfg = {}
    for k in ("in_channels", "num_keypoints", "seq_len", "num_tokens"):
        if k not in m:
            raise ValueError(f"shopformer_2 config has no field 'model.{k}'")
        cfg[k] = int(m[k])
    for k in ("hidden_channels", "latent_channels"):
        if k not in g:
            raise ValueError(f"shopformer_2 config has no field 'model.gcae.{k}'")
        cfg["gcae." + k] = int(g[k])
    cfg["gcae.num_layers"] = int(g.get("num_layers", N_BLOCKS))
    for k, d in DEFAULT_TRANSFORMER_2.items():
        cfg["transformer." + k] = int(tr.get(k, d))
    for field, allowed in SUPPORTED_2.items():
        if cfg[field] not in allowed:
            raise ValueError(f"shopformer_2 config field '{field}' = {cfg[field]} is not supported (supported: {list(allowed)})")
    strides, final, pool = compute_strides_2(cfg["seq_len"], cfg["num_tokens"], cfg["gcae.num_layers"])
    t = cfg["seq_len"]
    for s in strides:
        t = (t - 1) // s + 1                       # what the 9-tap convolutions (pad 4) really emit
    if pool or t != cfg["num_tokens"] or max(strides) > 3:
        raise ValueError(f"shopformer_2 config fields 'seq_len' = {cfg['seq_len']} / 'num_tokens' = {cfg['num_tokens']}: strides {strides} end at "
                         f"{t} frames; the adaptive average pool and strides above 3 are not supported")
    din, d, heads, ff = (cfg["transformer." + k] for k in ("input_dim", "d_model", "num_heads", "dim_feedforward"))
    if din != cfg["gcae.latent_channels"] * cfg["num_keypoints"]:
        raise ValueError(f"shopformer_2 config field 'transformer.input_dim' = {din} is not latent_channels * num_keypoints = "
                         f"{cfg['gcae.latent_channels'] * cfg['num_keypoints']}")
    if d < 4 or d % 4 or d > MAX_D_MODEL_2:
        raise ValueError(f"shopformer_2 config field 'transformer.d_model' = {d} is not supported (a multiple of 4, at most {MAX_D_MODEL_2})")
    if heads < 1 or d % heads:
        raise ValueError(f"shopformer_2 config field 'transformer.num_heads' = {heads} does not divide d_model = {d}")
    if ff < 4 or ff % 4 or ff > MAX_FF_2:
        raise ValueError(f"shopformer_2 config field 'transformer.dim_feedforward' = {ff} is not supported (a multiple of 4, at most {MAX_FF_2})")
    return cfg


def _bn(sd, p):
    g = np.asarray(sd[p + ".weight"], np.float64) / np.sqrt(np.asarray(sd[p + ".running_var"], np.float64) + BN_EPS)
    return g, np.asarray(sd[p + ".bias"], np.float64) - np.asarray(sd[p + ".running_mean"], np.float64) * g


def _np_state(sd) -> Dict[str, np.ndarray]:
    return {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in sd.items()}


def _needer(sd, cfg):
    def need(key, shape):
        if key not in sd:
            raise ValueError(f"Shopformer checkpoint has no tensor '{key}' (config {cfg})")
        if tuple(sd[key].shape) != tuple(shape):
            raise ValueError(f"Shopformer checkpoint tensor '{key}' has shape {tuple(sd[key].shape)}, the config asks for {tuple(shape)}")
        return np.asarray(sd[key], np.float64)
    return need


def _fold_tokenizer(sd, need, t: Dict[str, np.ndarray], V: int, H: int, L: int, strides: List[int]) -> int:
    """bn_input and the four ST-GCN blocks (the same modules in both variants) into ``t``; -> the adjacency's longest row"""
    chans = [2, H, H, H, L]
    enc = "gcae.encoder."
    need(enc + "bn_input.weight", (2 * V,))
    g, b = _bn(sd, enc + "bn_input")
    t["in_scale"], t["in_shift"] = g, b
    adj = need(enc + "layers.0.gcn.adj", (V, V))
    nnz = max(1, int((adj != 0).sum(1).max()))
    col, val = np.zeros((V, nnz), np.float64), np.zeros((V, nnz), np.float64)
    for v in range(V):
        nz = np.nonzero(adj[v])[0]
        col[v, :len(nz)], val[v, :len(nz)] = nz, adj[v, nz]
    t["adj_col"], t["adj_val"] = col, val
    for i in range(N_BLOCKS):
        p, ci, co = f"{enc}layers.{i}.", chans[i], chans[i + 1]
        if not np.array_equal(need(p + "gcn.adj", (V, V)), adj):
            raise ValueError(f"Shopformer checkpoint: '{p}gcn.adj' differs from block 0's adjacency")
        t[f"b{i}.gw"] = need(p + "gcn.weight", (ci, co)).T.reshape(co, 1, ci)
        t[f"b{i}.gb"] = need(p + "gcn.bias", (co,))
        g, b = _bn(sd, p + "tcn.bn")
        w = need(p + "tcn.conv.weight", (co, co, KT, 1))[..., 0]                    # [o, i, k]
        t[f"b{i}.tw"] = (w * g[:, None, None]).transpose(0, 2, 1)                    # [o, k, i]
        t[f"b{i}.tb"] = need(p + "tcn.conv.bias", (co,)) * g + b
        if ci != co or strides[i] != 1:
            g, b = _bn(sd, p + "residual.1")
            t[f"b{i}.rw"] = (need(p + "residual.0.weight", (co, ci, 1, 1))[:, :, 0, 0] * g[:, None]).reshape(co, 1, ci)
            t[f"b{i}.rb"] = need(p + "residual.0.bias", (co,)) * g + b
    return nnz


def fold_state_dict(sd: Dict[str, np.ndarray], config: Optional[dict] = None, dtype=np.float32, variant: Optional[int] = None,
                    decoder: bool = False) -> Tuple[dict, Dict[str, np.ndarray]]:
    """reference state dict -> (geometry, logical folded tensors, float32; ``dtype=np.float64`` keeps the unrounded fold, for tests).  Every BatchNorm disappears into the scale/shift of the
    input or into the weights and bias of the conv in front of it (folded in float64, rounded once).  Matrices are [out, taps, in].
    ``variant``: 1 = ``shopformer/``, 2 = ``shopformer_2/``, None = 2 when the config is the nested dict with a ``model`` key.
    ``decoder``: also fold ``gcae.decoder.*`` (the geometry then has the version-3 fields)."""
    if variant not in (None, 1, 2):
        raise ValueError(f"Shopformer variant must be 1 or 2, got {variant}")
    if variant == 2 or (variant is None and is_variant_2(config)):
        return fold_state_dict_2(sd, config, dtype, decoder)
    cfg = resolve_config(config)
    sd = _np_state(sd)
    V, T, H, L = cfg["num_keypoints"], cfg["seq_len"], cfg["hidden_channels"], cfg["latent_channels"]
    D = L * V
    strides = block_strides(T, cfg["num_tokens"])
    tn = [T]
    for s in strides:
        tn.append((tn[-1] - 1) // s + 1)
    need = _needer(sd, cfg)
    t: Dict[str, np.ndarray] = {}
    nnz = _fold_tokenizer(sd, need, t, V, H, L, strides)
    ntok = tn[-1]
    shape = lambda k: sd[k].shape if k in sd else ()
    t["pe_in"] = need("transformer.pos_encoder.pe", shape("transformer.pos_encoder.pe"))[0, :ntok, :D]
    t["pe_score"] = need("pos_encoder.pe", shape("pos_encoder.pe"))[0, :ntok, :D]
    if t["pe_in"].shape != (ntok, D) or t["pe_score"].shape != (ntok, D):
        raise ValueError(f"Shopformer checkpoint: positional encodings do not cover {ntok} tokens of {D} features")

    def lin(dst, src, o, i):
        t[dst + ".w"], t[dst + ".b"] = need(src + "weight", (o, i)).reshape(o, 1, i), need(src + "bias", (o,))

    def attn(dst, src):
        # q and (k, v) as two matrices: cross-attention feeds them different inputs, and D need not be a multiple of the 16-row tile
        w, b = need(src + "in_proj_weight", (3 * D, D)), need(src + "in_proj_bias", (3 * D,))
        t[dst + ".q.w"], t[dst + ".q.b"] = w[:D].reshape(D, 1, D), b[:D]
        t[dst + ".kv.w"], t[dst + ".kv.b"] = w[D:].reshape(2 * D, 1, D), b[D:]
        lin(dst + ".out", src + "out_proj.", D, D)

    def norm(dst, src):
        t[dst + ".g"], t[dst + ".b"] = need(src + "weight", (D,)), need(src + "bias", (D,))

    for e in range(cfg["transformer_layers"]):
        p = f"transformer.encoder_layers.{e}."
        attn(f"e{e}.sa", p + "self_attn.")
        norm(f"e{e}.n1", p + "norm1.")
        lin(f"e{e}.f1", p + "linear1.", FF_DIM, D)
        lin(f"e{e}.f2", p + "linear2.", D, FF_DIM)
        norm(f"e{e}.n2", p + "norm2.")
        p = f"transformer.decoder_layers.{e}."
        attn(f"d{e}.sa", p + "self_attn.")
        norm(f"d{e}.n1", p + "norm1.")
        attn(f"d{e}.ca", p + "multihead_attn.")
        norm(f"d{e}.n2", p + "norm2.")
        lin(f"d{e}.f1", p + "linear1.", FF_DIM, D)
        lin(f"d{e}.f2", p + "linear2.", D, FF_DIM)
        norm(f"d{e}.n3", p + "norm3.")
    lin("proj", "transformer.output_proj.", D, D)
    geo = {"V": V, "T": T, "H": H, "L": L, "heads": cfg["transformer_heads"], "layers": cfg["transformer_layers"], "ff": FF_DIM, "D": D,
           "ntok": ntok, "nnz": nnz, "s0": strides[0], "s1": strides[1], "s2": strides[2], "s3": strides[3],
           "T1": tn[1], "T2": tn[2], "T3": tn[3], "T4": tn[4]}
    if decoder:
        _fold_decoder(sd, need, t, geo, cfg["num_tokens"])
    return geo, {k: np.ascontiguousarray(v, dtype) for k, v in t.items()}


def fold_state_dict_2(sd, config: dict, dtype=np.float32, decoder: bool = False) -> Tuple[dict, Dict[str, np.ndarray]]:
    """the ``shopformer_2`` state dict (``gcae.*``, ``transformer.encoder.layers.N.*``, ``transformer.encoder.norm.*``, the decoder
    alike, ``transformer.input_projection.*`` / ``output_projection.*`` when input_dim != d_model) -> (geometry, folded tensors).
    Layer names in the image: e{N} / d{N} as in variant 1, ``en`` / ``dn`` the two final norms, ``inp`` / ``outp`` the projections."""
    cfg = resolve_config_2(config)
    sd = _np_state(sd)
    V, T, H, L = cfg["num_keypoints"], cfg["seq_len"], cfg["gcae.hidden_channels"], cfg["gcae.latent_channels"]
    Din, D, ff = cfg["transformer.input_dim"], cfg["transformer.d_model"], cfg["transformer.dim_feedforward"]
    layers, ntok = cfg["transformer.num_layers"], cfg["num_tokens"]
    strides, _, _ = compute_strides_2(T, ntok, N_BLOCKS)
    tn = [T]
    for s in strides:
        tn.append((tn[-1] - 1) // s + 1)
    need = _needer(sd, cfg)
    t: Dict[str, np.ndarray] = {}
    nnz = _fold_tokenizer(sd, need, t, V, H, L, strides)
    if "transformer.pos_encoder.pe" not in sd:
        raise ValueError(f"Shopformer checkpoint has no tensor 'transformer.pos_encoder.pe' (config {cfg})")
    t["pe_in"] = np.asarray(sd["transformer.pos_encoder.pe"], np.float64)[0, :ntok, :D]
    if t["pe_in"].shape != (ntok, D):
        raise ValueError(f"Shopformer checkpoint: the positional encoding does not cover {ntok} tokens of {D} features")

    def lin(dst, src, o, i):
        t[dst + ".w"], t[dst + ".b"] = need(src + "weight", (o, i)).reshape(o, 1, i), need(src + "bias", (o,))

    def attn(dst, src):
        w, b = need(src + "in_proj_weight", (3 * D, D)), need(src + "in_proj_bias", (3 * D,))
        t[dst + ".q.w"], t[dst + ".q.b"] = w[:D].reshape(D, 1, D), b[:D]
        t[dst + ".kv.w"], t[dst + ".kv.b"] = w[D:].reshape(2 * D, 1, D), b[D:]
        lin(dst + ".out", src + "out_proj.", D, D)

    def norm(dst, src):
        t[dst + ".g"], t[dst + ".b"] = need(src + "weight", (D,)), need(src + "bias", (D,))

    proj = Din != D
    if proj:
        lin("inp", "transformer.input_projection.", D, Din)
    for e in range(layers):
        p = f"transformer.encoder.layers.{e}."
        attn(f"e{e}.sa", p + "self_attn.")
        norm(f"e{e}.n1", p + "norm1.")
        lin(f"e{e}.f1", p + "linear1.", ff, D)
        lin(f"e{e}.f2", p + "linear2.", D, ff)
        norm(f"e{e}.n2", p + "norm2.")
    norm("en", "transformer.encoder.norm.")
    for e in range(layers):
        p = f"transformer.decoder.layers.{e}."
        attn(f"d{e}.sa", p + "self_attn.")
        norm(f"d{e}.n1", p + "norm1.")
        attn(f"d{e}.ca", p + "multihead_attn.")
        norm(f"d{e}.n2", p + "norm2.")
        lin(f"d{e}.f1", p + "linear1.", ff, D)
        lin(f"d{e}.f2", p + "linear2.", D, ff)
        norm(f"d{e}.n3", p + "norm3.")
    norm("dn", "transformer.decoder.norm.")
    if proj:
        lin("outp", "transformer.output_projection.", Din, D)
    geo = {"V": V, "T": T, "H": H, "L": L, "heads": cfg["transformer.num_heads"], "layers": layers, "ff": ff, "D": D,
           "ntok": ntok, "nnz": nnz, "s0": strides[0], "s1": strides[1], "s2": strides[2], "s3": strides[3],
           "T1": tn[1], "T2": tn[2], "T3": tn[3], "T4": tn[4],
           "variant": 2, "Din": Din, "in_proj": int(proj), "out_proj": int(proj), "norm_kind": NORM_PRE, "act_kind": ACT_GELU_ERF}
    if decoder:
        _fold_decoder(sd, need, t, geo, cfg["num_tokens"])
    return geo, {k: np.ascontiguousarray(v, dtype) for k, v in t.items()}


# ---------------------------------------------------------------------------------------------- kernel layout
def pack_mfma(w: np.ndarray) -> np.ndarray:
    """[out, taps, in] -> the A-operand fragment order of v_mfma_f32_16x16x4_f32, [out tile 16][tap][in block 16][lane 64][4]:
    lane l holds out = 16*tile + l % 16, in = 16*block + 4*(l // 16) + s for s = 0..3; zeros beyond either extent."""
    co, taps, ci = w.shape
    nct, cib = (co + 15) // 16, (ci + 15) // 16
    pad = np.zeros((nct * 16, taps, cib * 16), np.float32)
    pad[:co, :, :ci] = w
    p = pad.reshape(nct, 16, taps, cib, 4, 4)                    # ct, i, tap, cb, q, s
    return np.ascontiguousarray(p.transpose(0, 2, 3, 4, 1, 5)).reshape(-1)     # ct, tap, cb, q, i, s  (lane = 16 q + i)


def unpack_mfma(flat: np.ndarray, co: int, taps: int, ci: int) -> np.ndarray:
    nct, cib = (co + 15) // 16, (ci + 15) // 16
    p = np.asarray(flat).reshape(nct, taps, cib, 4, 16, 4).transpose(0, 4, 1, 2, 3, 5)
    return np.ascontiguousarray(p.reshape(nct * 16, taps, cib * 16)[:co, :, :ci])


def _is_matrix(name: str) -> bool:
    return name.endswith((".w", ".gw", ".tw", ".rw")) and not name.startswith("b0.g") and name != "b0.rw"


def build_image(geo: dict, tensors: Dict[str, np.ndarray]) -> bytes:
    """header | config ints | tensor table (name, kind, logical dims, offset, count) | float32 data, 16-byte aligned.
    Matrices are stored packed (``pack_mfma``); block 0's two-input-channel matrices, biases, gains and tables stay plain
    (biases padded with zeros to a multiple of 16 floats, which is what a 16-wide output tile reads)."""
    entries, data, off = [], [], 0
    for name, a in tensors.items():
        a = np.asarray(a, np.float32)
        if _is_matrix(name):
            kind, dims, flat = KIND_PACKED, a.shape, pack_mfma(a)
        else:
            kind, dims = KIND_PLAIN, (a.shape + (1, 1, 1))[:3]
            flat = a.reshape(-1)
            flat = np.concatenate([flat, np.zeros((-len(flat)) % 16, np.float32)])
        entries.append((name.encode(), kind, dims, off, len(flat)))
        data.append(flat)
        off += len(flat)
    ver, fields = (IMAGE_VERSION_2, CFG_FIELDS_V2) if geo.get("variant", 1) == 2 else (IMAGE_VERSION, CFG_FIELDS)
    if "Tdec" in geo:
        ver, fields = IMAGE_VERSION_3, CFG_FIELDS_V3
    head = MAGIC + struct.pack("<II", ver, len(fields)) + struct.pack(f"<{len(fields)}i", *(geo[f] for f in fields))
    head += struct.pack("<I", len(entries))
    for name, kind, dims, o, n in entries:
        head += struct.pack("<32sI3IQQ", name, kind, *dims, o, n)
    head += b"\0" * ((-len(head)) % 16)
    return head + np.concatenate(data).tobytes()


def parse_image(blob: bytes) -> Tuple[dict, Dict[str, np.ndarray]]:
    """the inverse of ``build_image``: geometry and the LOGICAL tensors (matrices unpacked from the fragment order)"""
    if blob[:8] != MAGIC:
        raise ValueError("not a Shopformer weight image (bad magic)")
    ver, ncfg = struct.unpack_from("<II", blob, 8)
    fields = {IMAGE_VERSION: CFG_FIELDS, IMAGE_VERSION_2: CFG_FIELDS_V2, IMAGE_VERSION_3: CFG_FIELDS_V3}.get(ver)
    if fields is None or ncfg != len(fields):
        raise ValueError(f"unsupported Shopformer weight image version {ver}")
    pos = 16
    geo = dict(zip(fields, struct.unpack_from(f"<{ncfg}i", blob, pos)))
    pos += 4 * ncfg
    (n,) = struct.unpack_from("<I", blob, pos)
    pos += 4
    rec = struct.Struct("<32sI3IQQ")
    table = [rec.unpack_from(blob, pos + i * rec.size) for i in range(n)]
    pos += n * rec.size
    pos += (-pos) % 16
    data = np.frombuffer(blob, np.float32, offset=pos)
    out = {}
    for name, kind, d0, d1, d2, o, cnt in table:
        name = name.rstrip(b"\0").decode()
        flat = data[o:o + cnt]
        out[name] = unpack_mfma(flat, d0, d1, d2) if kind == KIND_PACKED else flat[:d0 * d1 * d2].reshape([d for d in (d0, d1, d2)]).squeeze()
        if kind == KIND_PLAIN and out[name].ndim == 0:
            out[name] = out[name].reshape(1)
    for k in [k for k in ("adj_col", "adj_val", "pe_in", "pe_score") if k in out]:
        out[k] = out[k].reshape(geo["V"] if k.startswith("adj") else geo["ntok"], -1)
    for k in ("b0.gw", "b0.rw"):
        out[k] = out[k].reshape(geo["H"], 1, 2)
    return geo, out


def image_from_state_dict(sd, config: Optional[dict] = None, variant: Optional[int] = None, decoder: bool = False) -> bytes:
    """``decoder=False``: the version-1 / version-2 image of the score path; ``decoder=True``: a version-3 image with the GCAE decoder too"""
    return build_image(*fold_state_dict(sd, config, variant=variant, decoder=decoder))


def load_config_file(path) -> Optional[dict]:
    """a config path -> dict: ``.yaml`` / ``.yml`` through PyYAML (imported here, only when asked for), anything else as JSON"""
    if not os.path.exists(path):
        return None
    with open(path) as f:
        if str(path).lower().endswith((".yaml", ".yml")):
            import yaml
            return yaml.safe_load(f)
        return json.load(f)


def state_dict_from_checkpoint(ck: dict) -> dict:
    """``model_state_dict``, the split ``gcae_state_dict`` + ``transformer_state_dict`` pair, or the bare state dict itself"""
    if "model_state_dict" in ck:
        return ck["model_state_dict"]
    if "gcae_state_dict" in ck or "transformer_state_dict" in ck:
        if not ("gcae_state_dict" in ck and "transformer_state_dict" in ck):
            raise ValueError("Shopformer checkpoint: the split form needs both 'gcae_state_dict' and 'transformer_state_dict'")
        sd = {"gcae." + k: v for k, v in ck["gcae_state_dict"].items()}
        sd.update({"transformer." + k: v for k, v in ck["transformer_state_dict"].items()})
        return sd
    return ck


def image_from_checkpoint(path: str, config=None, variant: Optional[int] = None, decoder: bool = False) -> bytes:
    import torch
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if config is None and isinstance(ck, dict) and is_variant_2(ck.get("config")):
        config = ck["config"]
    if config is None:
        config = os.path.join(os.path.dirname(os.path.abspath(path)), "config.json")
    if isinstance(config, (str, os.PathLike)):
        config = load_config_file(config)
    return image_from_state_dict(state_dict_from_checkpoint(ck), config, variant=variant, decoder=decoder)


# ---------------------------------------------------------------------------------------------- the model
class ShopformerInfo(C.Structure):
    _fields_ = [("num_keypoints", C.c_int), ("seq_len", C.c_int), ("hidden_channels", C.c_int), ("latent_channels", C.c_int),
                ("heads", C.c_int), ("layers", C.c_int), ("n_tokens", C.c_int), ("d_model", C.c_int), ("group", C.c_int),
                ("lds_bytes", C.c_int), ("variant", C.c_int), ("group_transformer", C.c_int), ("n_params", C.c_longlong),
                ("macs_per_window", C.c_longlong), ("launches", C.c_longlong)]


class ShopformerOutputs(C.Structure):
    """mi355_shopformer_outputs_t: optional output pointers of the *_ex entry points (host or device, as the call takes them)"""
    _fields_ = [("struct_size", C.c_int), ("reserved", C.c_int), ("scores", C.c_void_p), ("token_scores", C.c_void_p),
                ("tokens", C.c_void_p), ("recon", C.c_void_p), ("poses", C.c_void_p), ("pose_error", C.c_void_p)]


class ShopformerDecoderInfo(C.Structure):
    _fields_ = [("factors", C.c_int * 4), ("frames", C.c_int), ("interpolate", C.c_int), ("group", C.c_int), ("lds_bytes", C.c_int),
                ("macs_per_window", C.c_longlong)]


NO_DECODER = "this Shopformer model was loaded without the decoder (load it with decoder=True)"


def _outputs(scores=None, token_scores=None, tokens=None, recon=None, poses=None, pose_error=None) -> ShopformerOutputs:
    return ShopformerOutputs(C.sizeof(ShopformerOutputs), 0, scores or None, token_scores or None, tokens or None, recon or None,
                             poses or None, pose_error or None)


class Shopformer:
    """``model.score(windows)``: windows ``[N, 2, T, V]`` float32 (normalised as the reference's loader does) -> ``[N]`` anomaly
    scores (higher = less like the training data), computed on an MI355X.  There is no CPU path."""

    def __init__(self, image: bytes, device: int = 0):
        self._h = C.c_void_p()
        self._blob = bytes(image)
        self.device = int(device)
        self.geometry, _ = parse_image(self._blob)
        _lib.check(_lib.lib().mi355_shopformer_create(self._blob, len(self._blob), self.device, C.byref(self._h)))
        self.info = self._info()
        self.seq_len, self.num_keypoints = self.info.seq_len, self.info.num_keypoints
        self.n_tokens, self.d_model = self.info.n_tokens, self.info.d_model
        self.variant = int(self.geometry.get("variant", 1))
        self.token_dim = int(self.geometry.get("Din", self.d_model))        # width of tokens / reconstructed_tokens
        self.neck = self.variant == 2 and self.num_keypoints == 18           # the shopformer_2 loader synthesises joint 17
        self.decoder_info = None
        if self.has_decoder:
            self.decoder_info = ShopformerDecoderInfo()
            _lib.check(_lib.lib().mi355_shopformer_decoder_info(self._h, C.byref(self.decoder_info)))

    def _info(self) -> ShopformerInfo:
        info = ShopformerInfo()
        _lib.check(_lib.lib().mi355_shopformer_info(self._h, C.byref(info)))
        return info

    @property
    def launches(self) -> int:
        """kernel launches this model has enqueued so far (the engine's own counter, incremented beside the launch)"""
        return int(self._info().launches)

    @property
    def has_decoder(self) -> bool:
        """the image holds the GCAE decoder (it was built with ``decoder=True``): ``forward(poses=True)`` and ``decode`` work"""
        return "Tdec" in self.geometry

    @classmethod
    def from_state_dict(cls, sd, config: Optional[dict] = None, device: int = 0, variant: Optional[int] = None,
                        decoder: bool = False) -> "Shopformer":
        return cls(image_from_state_dict(sd, config, variant=variant, decoder=decoder), device=device)

    @classmethod
    def from_checkpoint(cls, path: str, config=None, device: int = 0, variant: Optional[int] = None, decoder: bool = False) -> "Shopformer":
        """``torch.save({'model_state_dict': ...})`` as the reference's train.py writes it; ``config``: a dict, a path, or None for the
        ``config.json`` beside the checkpoint (absent: the reference's defaults), as its inference.py resolves it.  A ``shopformer_2``
        checkpoint carries its nested config under ``config`` (used when none is given); ``config`` may also be a YAML path; the split
        ``gcae_state_dict`` / ``transformer_state_dict`` form is accepted as its evaluate.py accepts it."""
        return cls(image_from_checkpoint(path, config, variant, decoder), device=device)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.lib().mi355_shopformer_destroy(h)
            except Exception:
                pass
            self._h = C.c_void_p()

    def _check(self, windows) -> np.ndarray:
        w = np.ascontiguousarray(windows, np.float32)
        if w.ndim != 4 or w.shape[1:] != (2, self.seq_len, self.num_keypoints):
            raise ValueError(f"windows must be [N, 2, {self.seq_len}, {self.num_keypoints}], got {tuple(w.shape)}")
        return w

    def _run(self, want, n: int, call) -> Dict[str, np.ndarray]:
        """allocates the host outputs ``want`` names (fields of ``ShopformerOutputs``) for ``n`` windows, builds the struct and, for
        n > 0, hands it to ``call``: the window form or the poses form of the ``_ex`` entry points -> {field: array}"""
        tok, win = (self.n_tokens, self.token_dim), (self.seq_len, self.num_keypoints)
        shapes = {"scores": (), "token_scores": tok[:1], "tokens": tok, "recon": tok, "poses": (2,) + win, "pose_error": win}
        out = {k: np.empty((n,) + shapes[k], np.float32) for k in want}
        if n:
            _lib.check(call(C.byref(_outputs(**{k: a.ctypes.data for k, a in out.items()}))))
        return out

    def forward(self, windows, outputs: bool = True, poses: bool = False) -> Dict[str, np.ndarray]:
        """-> ``normality_score`` [N]; with ``outputs`` also ``tokens`` and ``reconstructed_tokens`` [N, n_tokens, token_dim] and, for
        the shopformer_2 variant, ``token_scores`` [N, n_tokens]; with ``poses`` (a model loaded with ``decoder=True``) also
        ``gcae_reconstructed`` [N, 2, T, V] = the decoder on ``tokens`` (the same array as ``reconstructed_poses``, shopformer_2's name)
        and ``pose_error`` [N, T, V], the mean over the 2 channels of (reconstruction - window)^2"""
        w = self._check(windows)
        if poses and not self.has_decoder:
            raise ValueError(NO_DECODER)
        want = ["scores"] + (["tokens", "recon"] + ["token_scores"] * (self.variant == 2) if outputs else []) + (["poses", "pose_error"] if poses else [])
        a = self._run(want, len(w), lambda o: _lib.lib().mi355_shopformer_score_ex(self._h, w.ctypes.data, len(w), o))
        out = {"normality_score": a["scores"]}
        if outputs:
            out["tokens"], out["reconstructed_tokens"] = a["tokens"], a["recon"]
        if "token_scores" in a:
            out["token_scores"] = a["token_scores"]
        if poses:
            out["gcae_reconstructed"] = out["reconstructed_poses"] = a["poses"]
            out["pose_error"] = a["pose_error"]
        return out

    def decode(self, tokens) -> np.ndarray:
        """tokens ``[N, n_tokens, token_dim]`` -> the decoder's poses ``[N, 2, T, V]``; ``decode(forward(x)["reconstructed_tokens"])`` is
        the pose the transformer expected.  One launch; a pose's bits do not depend on N or on its position."""
        if not self.has_decoder:
            raise ValueError(NO_DECODER)
        t = np.ascontiguousarray(tokens, np.float32)
        if t.ndim != 3 or t.shape[1:] != (self.n_tokens, self.token_dim):
            raise ValueError(f"tokens must be [N, {self.n_tokens}, {self.token_dim}], got {tuple(t.shape)}")
        pose = np.empty((len(t), 2, self.seq_len, self.num_keypoints), np.float32)
        if len(t):
            _lib.check(_lib.lib().mi355_shopformer_decode(self._h, t.ctypes.data, len(t), pose.ctypes.data))
        return pose

    def decode_device_async(self, tokens_dev: int, n: int, poses_dev: int, stream: int = 0) -> None:
        """``decode`` on device pointers, enqueued on the caller's stream; returns without waiting"""
        if not self.has_decoder:
            raise ValueError(NO_DECODER)
        _lib.check(_lib.lib().mi355_shopformer_decode_device_async(self._h, tokens_dev, int(n), poses_dev, stream or None))

    def score(self, windows, reduction: str = "mean") -> np.ndarray:
        """``reduction='mean'`` -> [N]; ``'none'`` -> [N, n_tokens] (the shopformer_2 variant's per-token scores)"""
        if reduction == "mean":
            return self.forward(windows, outputs=False)["normality_score"]
        if reduction != "none":
            raise ValueError(f"Unknown reduction: {reduction}")
        if self.variant != 2:
            raise ValueError("reduction='none' exists only for the shopformer_2 variant: the shopformer/ network has no per-token score")
        w = self._check(windows)
        return self._run(["token_scores"], len(w), lambda o: _lib.lib().mi355_shopformer_score_ex(self._h, w.ctypes.data, len(w), o))["token_scores"]

    def predict(self, windows, threshold: float = 0.5) -> np.ndarray:
        return (self.score(windows) > threshold).astype(np.int64)

    def score_poses(self, poses, starts, reduction: str = "mean") -> np.ndarray:
        """``score`` on windows the device builds itself: ``poses`` [P, V_src, 2] float32 or float64 (the x, y of
        every retained pose), window i = the ``seq_len`` consecutive poses from ``starts[i]``.  One upload, the window launch, the
        score launch(es): the same bits as ``score(_window_tensor(...))`` of those poses.  The neck joint follows ``self.neck``."""
        from . import ops
        if reduction not in ("mean", "none"):
            raise ValueError(f"Unknown reduction: {reduction}")
        if reduction == "none" and self.variant != 2:
            raise ValueError("reduction='none' exists only for the shopformer_2 variant: the shopformer/ network has no per-token score")
        p, code = ops.pose_array(poses)
        st = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1)
        field = "scores" if reduction == "mean" else "token_scores"
        return self._run([field], len(st), lambda o: _lib.lib().mi355_shopformer_score_poses(
            self._h, p.ctypes.data, code, p.shape[0], p.shape[1], st.ctypes.data, len(st), int(self.neck), o))[field]

    def score_device_async(self, windows_dev: int, n: int, scores_dev: int, stream: int = 0, tokens_dev: int = 0, recon_dev: int = 0,
                           token_scores_dev: int = 0, poses_dev: int = 0, pose_error_dev: int = 0) -> None:
        """device pointers in, device pointers out, enqueued on the caller's stream (0 = the null stream); returns without waiting.
        ``token_scores_dev`` ([n, n_tokens]) is an output of the shopformer_2 variant only; ``poses_dev`` ([n, 2, T, V]) and
        ``pose_error_dev`` ([n, T, V], beside ``poses_dev``) need a model loaded with ``decoder=True``."""
        if (poses_dev or pose_error_dev) and not self.has_decoder:
            raise ValueError(NO_DECODER)
        if token_scores_dev and self.variant != 2:
            raise ValueError("token_scores exist only for the shopformer_2 variant")
        o = _outputs(scores_dev, token_scores_dev, tokens_dev, recon_dev, poses_dev, pose_error_dev)
        _lib.check(_lib.lib().mi355_shopformer_score_ex_device_async(self._h, windows_dev, int(n), C.byref(o), stream or None))


# ---------------------------------------------------------------------------------------------- tracks -> windows -> scores
def _normalise(seq: np.ndarray) -> np.ndarray:
    """[T, V, 2] pixels -> centred on the mean of the non-zero joints, divided by the largest |offset| (+1e-6): inside [-1, 1]"""
    xy = seq[:, :, :2].copy()
    valid = np.any(xy != 0, axis=-1)
    if valid.sum() > 0:
        centre = xy[valid].mean(axis=0)
        scale = np.abs((xy - centre)[valid]).max() + 1e-6
    else:
        centre, scale = np.array([0.0, 0.0]), 1.0
    seq[:, :, :2] = np.nan_to_num((xy - centre) / scale, nan=0.0, posinf=0.0, neginf=0.0)
    return seq


def _with_neck(k: np.ndarray) -> np.ndarray:
    """(>= 0, 3) keypoints -> (18, 3): the 17 COCO joints (zero rows if fewer came) and joint 17, the midpoint of the shoulders
    (joints 5 and 6); a shoulder whose x and y are both ~0 is missing: the neck is then the other shoulder, or zero without both"""
    if k.shape[0] < 17:
        k = np.vstack([k, np.zeros((17 - k.shape[0], k.shape[1]))])
    ls, rs = k[5], k[6]
    neck = (ls + rs) / 2.0
    l0, r0 = np.allclose(ls[:2], 0), np.allclose(rs[:2], 0)
    if l0 and r0:
        neck = np.zeros_like(ls)
    elif l0:
        neck = rs.copy()
    elif r0:
        neck = ls.copy()
    return np.vstack([k[:17], neck.reshape(1, -1)])


def _window_tensor(poses: List[np.ndarray], num_keypoints: int, neck: bool = False) -> np.ndarray:
    if neck:
        poses = [_with_neck(np.asarray(k).reshape(-1, 3)) for k in poses]
    seq = np.array([np.asarray(k).reshape(-1, 3)[:num_keypoints, :2] for k in poses])       # (V, 3) or the flat (3 V,) form
    if seq.shape[1] < num_keypoints:
        seq = np.concatenate([seq, np.zeros((seq.shape[0], num_keypoints - seq.shape[1], 2), seq.dtype)], axis=1)
    return np.transpose(_normalise(seq).astype(np.float32), (2, 0, 1))


def windows_from_poselift(data: dict, seq_len: int = 12, stride: int = 6, max_gap: int = 5, num_keypoints: int = 17, neck: bool = False):
    """PoseLift dict ``{frame: {person: [bbox, kpts(V, 3)]}}`` -> (windows ``[n, 2, seq_len, V]`` float32, index) with
    ``index[i] = (person_id, first_frame, last_frame)``, in the order the reference's loader emits its samples: persons in order of
    first appearance, each person's frames sorted, a window every ``stride`` of that person's frames, dropped when two consecutive
    frames of it lie more than ``max_gap`` apart; poses with NaN / inf are left out before windowing.  ``neck=True`` (with
    ``num_keypoints=18``): joint 17 is the neck the ``shopformer_2`` loader synthesises from the shoulders, added before normalisation;
    without it joints beyond those delivered are zero."""
    if neck and num_keypoints != 18:
        raise ValueError("neck=True needs num_keypoints=18 (17 COCO joints + the neck)")
    per = _people(data)
    xs, index = [], []
    for pid, fr in per.items():
        idx = sorted(fr)
        for s in range(0, len(idx) - seq_len + 1, stride):
            win = idx[s:s + seq_len]
            if any(b - a > max_gap for a, b in zip(win, win[1:])):
                continue
            xs.append(_window_tensor([fr[f] for f in win], num_keypoints, neck))
            index.append((int(pid), int(win[0]), int(win[-1])))
    x = np.stack(xs) if xs else np.zeros((0, 2, seq_len, num_keypoints), np.float32)
    return x, index


def _people(data: dict) -> Dict[int, Dict[int, np.ndarray]]:
    """person -> {frame: keypoints} in order of first appearance; records without keypoints and poses with NaN / inf are left out"""
    per: Dict[int, Dict[int, np.ndarray]] = {}
    for fnum, people in data.items():
        if not people or not isinstance(people, dict):
            continue
        for pid, rec in people.items():
            if not isinstance(rec, (list, tuple)) or len(rec) < 2:
                continue
            k = np.array(rec[1])
            if np.isnan(k).any() or np.isinf(k).any():
                continue
            per.setdefault(pid, {})[int(fnum)] = k
    return per


def pack_poselift(data: dict, seq_len: int = 12, stride: int = 6, max_gap: int = 5):
    """The offline loader's window cut without building a window: -> (poses, starts, index).  ``poses`` [P, rows, 2] holds the x, y
    of every retained pose, persons in order of first appearance, each person's frames sorted; window i is the ``seq_len`` poses from
    ``starts[i]`` (int32); ``index`` is what ``windows_from_poselift`` returns.  The cut comes from each person's sorted frame numbers
    alone: starts 0, stride, ..., a start dropped when one of its ``seq_len - 1`` frame gaps exceeds ``max_gap``.
    ``poses`` is None when the dict is not one the device path covers: its poses must share ONE float dtype (float32 or float64) and
    ONE row count; mixed dtypes, integer poses and ragged row counts are left to the host path (where numpy promotes or refuses)."""
    per = _people(data)
    chunks, starts, index, off = [], [], [], 0
    sig = {(k.dtype, k.size // 3 if k.size % 3 == 0 else -1) for fr in per.values() for k in fr.values()}
    ok = len(sig) == 1 and next(iter(sig))[0] in (np.dtype(np.float32), np.dtype(np.float64)) and next(iter(sig))[1] > 0
    for pid, fr in per.items():
        idx = np.array(sorted(fr), np.int64)
        if ok:
            chunks.append(np.asarray([fr[int(f)] for f in idx]).reshape(len(idx), -1, 3)[:, :, :2])     # (V, 3) or the flat (3 V,) form
        s = np.arange(0, len(idx) - seq_len + 1, stride)
        if len(s):
            broken = np.concatenate([[0], np.cumsum(np.diff(idx) > max_gap)])         # gaps above max_gap before each position
            s = s[broken[s + seq_len - 1] == broken[s]]
            starts.append(off + s)
            index += [(int(pid), int(a), int(b)) for a, b in zip(idx[s], idx[s + seq_len - 1])]
        off += len(idx)
    st = np.concatenate(starts).astype(np.int32) if starts else np.zeros(0, np.int32)
    return (np.concatenate(chunks) if ok else None), st, index


def _device_poses(model, poses) -> bool:
    """the rule of ``score_poselift(on_device=True)``: the model scores poses itself, the dict packed to one float array, and a neck
    model got at least the 17 COCO rows (with fewer, the host path pads with float64 zeros and numpy promotes the window)"""
    return hasattr(model, "score_poses") and poses is not None and not (bool(getattr(model, "neck", False)) and poses.shape[1] < 17)


def score_poselift(model, data: dict, stride: int = 6, max_gap: int = 5, on_device: bool = False):
    """-> (scores [n], index) for every window of every person of one video's PoseLift dict.
    ``on_device=True``: the windows are built on the GPU (``model.score_poses``: one upload of the poses, one window launch, the score
    launches) instead of one by one on the host; same scores, same index, bit for bit.  That path covers dicts whose poses all share
    one float dtype (float32 or float64) and one row count, at least 17 rows when the model has a neck joint; any other dict (mixed
    dtypes, integer poses, ragged row counts, a neck model fed fewer than 17 rows), and a model without ``score_poses``, takes the host
    path for that call."""
    if on_device:
        poses, starts, index = pack_poselift(data, model.seq_len, stride, max_gap)
        if _device_poses(model, poses):
            return model.score_poses(poses, starts), index
    x, index = windows_from_poselift(data, seq_len=model.seq_len, stride=stride, max_gap=max_gap, num_keypoints=model.num_keypoints,
                                     neck=bool(getattr(model, "neck", False)))
    return model.score(x), index


def score_poselift_many(model, datas, stride: int = 6, max_gap: int = 5, on_device: bool = True):
    """``score_poselift`` for every dict of ``datas`` (a tree of videos) -> ``[(scores, index), ...]``.  With ``on_device`` the whole
    tree is ONE ``model.score_poses`` call: the videos' pose arrays concatenated, each video's offset added to its starts.  That needs
    every dict that holds poses to pass ``score_poselift``'s device rule with the same dtype and row count; otherwise each dict is
    scored by ``score_poselift`` on the host path."""
    datas = list(datas)
    packed = [pack_poselift(d, model.seq_len, stride, max_gap) for d in datas] if on_device else []
    full = [p for p in packed if p[0] is not None or p[2]]                            # dicts without a retained pose contribute nothing
    if not on_device or not full or not all(_device_poses(model, p[0]) for p in full) or len({(p[0].dtype, p[0].shape[1]) for p in full}) != 1:
        return [score_poselift(model, d, stride, max_gap) for d in datas]
    offs = np.cumsum([0] + [len(p[0]) if p[0] is not None else 0 for p in packed])
    scores = model.score_poses(np.concatenate([p[0] for p in full]), np.concatenate([p[1] + o for p, o in zip(packed, offs)]).astype(np.int32))
    cuts = np.cumsum([0] + [len(p[2]) for p in packed])
    return [(scores[a:b], p[2]) for p, a, b in zip(packed, cuts, cuts[1:])]


class StreamScorer:
    """The same windows, live: feed each frame's tracker rows and keypoints as ``model.track`` yields them; ``update`` returns
    ``[(person_id, first_frame, last_frame, score)]`` for every window the new frame completes.  Per track id it keeps the last
    ``seq_len`` poses and the count of poses seen, so a window closes at that person's poses number seq_len, seq_len + stride, ...
    exactly where the offline loader cuts them.  Frames must arrive in increasing order.  A track not seen for more than ``max_gap``
    frames gives its poses back (any window that still held them would straddle the gap and be dropped); only its pose count, one
    integer per id ever seen, stays, because the offline cut positions depend on it."""

    def __init__(self, model, stride: int = 6, max_gap: int = 5):
        self.model, self.stride, self.max_gap = model, int(stride), int(max_gap)
        self.seq_len, self.num_keypoints = model.seq_len, model.num_keypoints
        self.neck = bool(getattr(model, "neck", False))
        self._ring: Dict[int, list] = {}
        self._seen: Dict[int, int] = {}

    def cut(self, frame_num: int, track_rows, keypoints) -> list:
        """take one frame in -> ``[(person_id, first_frame, last_frame, poses)]``, the windows it completes, ``poses`` the window's
        ``seq_len`` keypoint arrays (float32, (rows, 3)); the half of ``update`` that ``MultiStreamScorer`` shares"""
        done = []
        for pid in [p for p, ring in self._ring.items() if frame_num - ring[-1][0] > self.max_gap]:
            del self._ring[pid]
        for row, kp in zip(np.asarray(track_rows), np.asarray(keypoints)):
            k = np.asarray(kp, np.float32).reshape(-1, 3)
            if np.isnan(k).any() or np.isinf(k).any():
                continue
            pid = int(row[4])
            ring = self._ring.setdefault(pid, [])
            ring.append((int(frame_num), k))
            del ring[:-self.seq_len]
            seen = self._seen[pid] = self._seen.get(pid, 0) + 1
            if len(ring) == self.seq_len and (seen - self.seq_len) % self.stride == 0:
                fr = [f for f, _ in ring]
                if any(b - a > self.max_gap for a, b in zip(fr, fr[1:])):
                    continue
                done.append((pid, fr[0], fr[-1], [p for _, p in ring]))
        return done

    def update(self, frame_num: int, track_rows, keypoints):
        done = self.cut(frame_num, track_rows, keypoints)
        if not done:
            return []
        scores = self.model.score(np.stack([_window_tensor(poses, self.num_keypoints, self.neck) for _, _, _, poses in done]))
        return [(pid, a, b, float(s)) for (pid, a, b, _), s in zip(done, scores)]


class MultiStreamScorer:
    """``StreamScorer`` for the N cameras of one store: ``update(frame_num, cams)`` takes one tick, ``cams[i]`` = ``(track_rows,
    keypoints)`` of camera i or None for a camera without a frame (it is not stepped); ``frame_num`` is one int or one per camera.
    It returns, per camera, the list that camera's own ``StreamScorer.update`` would return, the same floats: every camera cuts its
    windows with ``StreamScorer.cut`` on state of its own, and the tick's completed windows of ALL cameras go through ONE
    ``model.score_poses`` call (poses stacked, ``starts = arange(n) * seq_len``): one upload and one window launch per tick instead of
    N window builders, N uploads and N score calls.  A tick whose poses do not share one row count (at least 17 with a neck model),
    and a model without ``score_poses``, builds the windows on the host and calls ``model.score`` once."""

    def __init__(self, model, n_cameras: int, stride: int = 6, max_gap: int = 5):
        self.model, self.seq_len = model, model.seq_len
        self.cameras = [StreamScorer(model, stride, max_gap) for _ in range(int(n_cameras))]

    def update(self, frame_num, cams):
        cams = list(cams)
        if len(cams) != len(self.cameras):
            raise ValueError(f"one entry per camera: expected {len(self.cameras)}, got {len(cams)}")
        frames = [int(frame_num)] * len(cams) if np.ndim(frame_num) == 0 else [int(f) for f in frame_num]
        if len(frames) != len(cams):
            raise ValueError("frame_num is one int or one per camera")
        done = [cam.cut(f, *c) if c is not None else [] for cam, f, c in zip(self.cameras, frames, cams)]
        wins = [w for d in done for w in d]
        if not wins:
            return [[] for _ in cams]
        rows = {k.shape[0] for w in wins for k in w[3]}
        first = self.cameras[0]
        if hasattr(self.model, "score_poses") and len(rows) == 1 and not (first.neck and min(rows) < 17):
            poses = np.stack([k[:, :2] for w in wins for k in w[3]])
            scores = self.model.score_poses(poses, np.arange(len(wins), dtype=np.int32) * self.seq_len)
        else:
            scores = self.model.score(np.stack([_window_tensor(w[3], first.num_keypoints, first.neck) for w in wins]))
        out, at = [], 0
        for d in done:
            out.append([(pid, a, b, float(s)) for (pid, a, b, _), s in zip(d, scores[at:at + len(d)])])
            at += len(d)
        return out
