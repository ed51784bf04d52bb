"""Shopformer inference: pose windows -> anomaly score, the network of the reference's ``shopformer/`` in ``eval()`` mode as ONE
fused HIP launch (csrc/shopformer_kernels.hip).

Only what ``normality_score`` depends on is evaluated: ``bn_input`` -> 4 ST-GCN blocks -> tokens ``[N, 3, latent*V]`` -> positional
encoding -> post-norm transformer encoder / decoder (no causal mask) -> ``output_proj`` -> mean squared error against
``tokens + PE``.  The GCAE decoder is not part of the score and is not loaded.

This module holds (a) the loader: reference-named state dict -> folded tensors -> a small self-describing weight image whose
matrices are already in the kernel's MFMA fragment order, (b) ``Shopformer``, the ctypes front of ``mi355_shopformer_*``, and (c) the
host side between the tracker and the network: ``windows_from_poselift``, ``score_poselift``, ``StreamScorer``.
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
KIND_PLAIN, KIND_PACKED = 0, 1


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


def _bn(sd, p):
    g = np.asarray(sd[p + ".weight"], np.float64) / np.sqrt(np.asarray(sd[p + ".running_var"], np.float64) + BN_EPS)
    return g, np.asarray(sd[p + ".bias"], np.float64) - np.asarray(sd[p + ".running_mean"], np.float64) * g


def fold_state_dict(sd: Dict[str, np.ndarray], config: Optional[dict] = None, dtype=np.float32) -> Tuple[dict, Dict[str, np.ndarray]]:
    """reference state dict -> (geometry, logical folded tensors, float32; ``dtype=np.float64`` keeps the unrounded fold, for tests).  Every BatchNorm disappears into the scale/shift of the
    input or into the weights and bias of the conv in front of it (folded in float64, rounded once).  Matrices are [out, taps, in]."""
    cfg = resolve_config(config)
    sd = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in sd.items()}
    V, T, H, L = cfg["num_keypoints"], cfg["seq_len"], cfg["hidden_channels"], cfg["latent_channels"]
    D = L * V
    strides = block_strides(T, cfg["num_tokens"])
    tn = [T]
    for s in strides:
        tn.append((tn[-1] - 1) // s + 1)
    chans = [2, H, H, H, L]
    enc = "gcae.encoder."

    def need(key, shape):
        if key not in sd:
            raise ValueError(f"Shopformer checkpoint has no tensor '{key}' (config {cfg})")
        if tuple(sd[key].shape) != tuple(shape):
            raise ValueError(f"Shopformer checkpoint tensor '{key}' has shape {tuple(sd[key].shape)}, the config asks for {tuple(shape)}")
        return np.asarray(sd[key], np.float64)

    t: Dict[str, np.ndarray] = {}
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
    ntok = tn[-1]
    t["pe_in"] = need("transformer.pos_encoder.pe", sd["transformer.pos_encoder.pe"].shape)[0, :ntok, :D]
    t["pe_score"] = need("pos_encoder.pe", sd["pos_encoder.pe"].shape)[0, :ntok, :D]
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
    head = MAGIC + struct.pack("<II", IMAGE_VERSION, len(CFG_FIELDS)) + struct.pack(f"<{len(CFG_FIELDS)}i", *(geo[f] for f in CFG_FIELDS))
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
    if ver != IMAGE_VERSION or ncfg != len(CFG_FIELDS):
        raise ValueError(f"unsupported Shopformer weight image version {ver}")
    pos = 16
    geo = dict(zip(CFG_FIELDS, struct.unpack_from(f"<{ncfg}i", blob, pos)))
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
    for k in ("adj_col", "adj_val", "pe_in", "pe_score"):
        out[k] = out[k].reshape(geo["V"] if k.startswith("adj") else geo["ntok"], -1)
    for k in ("b0.gw", "b0.rw"):
        out[k] = out[k].reshape(geo["H"], 1, 2)
    return geo, out


def image_from_state_dict(sd, config: Optional[dict] = None) -> bytes:
    return build_image(*fold_state_dict(sd, config))


# ---------------------------------------------------------------------------------------------- the model
class ShopformerInfo(C.Structure):
    _fields_ = [("num_keypoints", C.c_int), ("seq_len", C.c_int), ("hidden_channels", C.c_int), ("latent_channels", C.c_int),
                ("heads", C.c_int), ("layers", C.c_int), ("n_tokens", C.c_int), ("d_model", C.c_int), ("group", C.c_int),
                ("lds_bytes", C.c_int), ("reserved", C.c_int * 2), ("n_params", C.c_longlong),
                ("macs_per_window", C.c_longlong), ("launches", C.c_longlong)]


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

    def _info(self) -> ShopformerInfo:
        info = ShopformerInfo()
        _lib.check(_lib.lib().mi355_shopformer_info(self._h, C.byref(info)))
        return info

    @property
    def launches(self) -> int:
        """kernel launches this model has enqueued so far (the engine's own counter, incremented beside the launch)"""
        return int(self._info().launches)

    @classmethod
    def from_state_dict(cls, sd, config: Optional[dict] = None, device: int = 0) -> "Shopformer":
        return cls(image_from_state_dict(sd, config), device=device)

    @classmethod
    def from_checkpoint(cls, path: str, config=None, device: int = 0) -> "Shopformer":
        """``torch.save({'model_state_dict': ...})`` as the reference's train.py writes it; ``config``: a dict, a path, or None for the
        ``config.json`` beside the checkpoint (absent: the reference's defaults), as its inference.py resolves it"""
        import torch
        if config is None:
            config = os.path.join(os.path.dirname(os.path.abspath(path)), "config.json")
        if isinstance(config, (str, os.PathLike)):
            if os.path.exists(config):
                with open(config) as f:
                    config = json.load(f)
            else:
                config = None
        ck = torch.load(path, map_location="cpu", weights_only=True)
        return cls.from_state_dict(ck["model_state_dict"] if "model_state_dict" in ck else ck, config, device=device)

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

    def forward(self, windows, outputs: bool = True) -> Dict[str, np.ndarray]:
        w = self._check(windows)
        n = len(w)
        score = np.empty(n, np.float32)
        tok = np.empty((n, self.n_tokens, self.d_model), np.float32) if outputs else None
        rec = np.empty((n, self.n_tokens, self.d_model), np.float32) if outputs else None
        if n:
            _lib.check(_lib.lib().mi355_shopformer_score(self._h, w.ctypes.data, n, score.ctypes.data,
                                                         tok.ctypes.data if outputs else None, rec.ctypes.data if outputs else None))
        out = {"normality_score": score}
        if outputs:
            out["tokens"], out["reconstructed_tokens"] = tok, rec
        return out

    def score(self, windows) -> np.ndarray:
        return self.forward(windows, outputs=False)["normality_score"]

    def predict(self, windows, threshold: float = 0.5) -> np.ndarray:
        return (self.score(windows) > threshold).astype(np.int64)

    def score_device_async(self, windows_dev: int, n: int, scores_dev: int, stream: int = 0, tokens_dev: int = 0, recon_dev: int = 0) -> None:
        """device pointers in, device pointers out, one launch on the caller's stream (0 = the null stream); returns without waiting"""
        _lib.check(_lib.lib().mi355_shopformer_score_device_async(self._h, windows_dev, int(n), scores_dev, tokens_dev or None,
                                                                  recon_dev or None, stream or None))


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


def _window_tensor(poses: List[np.ndarray], num_keypoints: int) -> np.ndarray:
    seq = np.array([np.asarray(k).reshape(-1, 3)[:num_keypoints, :2] for k in poses])       # (V, 3) or the flat (3 V,) form
    if seq.shape[1] < num_keypoints:
        seq = np.concatenate([seq, np.zeros((seq.shape[0], num_keypoints - seq.shape[1], 2), seq.dtype)], axis=1)
    return np.transpose(_normalise(seq).astype(np.float32), (2, 0, 1))


def windows_from_poselift(data: dict, seq_len: int = 12, stride: int = 6, max_gap: int = 5, num_keypoints: int = 17):
    """PoseLift dict ``{frame: {person: [bbox, kpts(V, 3)]}}`` -> (windows ``[n, 2, seq_len, V]`` float32, index) with
    ``index[i] = (person_id, first_frame, last_frame)``, in the order the reference's loader emits its samples: persons in order of
    first appearance, each person's frames sorted, a window every ``stride`` of that person's frames, dropped when two consecutive
    frames of it lie more than ``max_gap`` apart; poses with NaN / inf are left out before windowing."""
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
    xs, index = [], []
    for pid, fr in per.items():
        idx = sorted(fr)
        for s in range(0, len(idx) - seq_len + 1, stride):
            win = idx[s:s + seq_len]
            if any(b - a > max_gap for a, b in zip(win, win[1:])):
                continue
            xs.append(_window_tensor([fr[f] for f in win], num_keypoints))
            index.append((int(pid), int(win[0]), int(win[-1])))
    x = np.stack(xs) if xs else np.zeros((0, 2, seq_len, num_keypoints), np.float32)
    return x, index


def score_poselift(model, data: dict, stride: int = 6, max_gap: int = 5):
    """-> (scores [n], index) for every window of every person of one video's PoseLift dict"""
    x, index = windows_from_poselift(data, seq_len=model.seq_len, stride=stride, max_gap=max_gap, num_keypoints=model.num_keypoints)
    return model.score(x), index


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
        self._ring: Dict[int, list] = {}
        self._seen: Dict[int, int] = {}

    def update(self, frame_num: int, track_rows, keypoints):
        done, xs = [], []
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
                xs.append(_window_tensor([p for _, p in ring], self.num_keypoints))
                done.append((pid, fr[0], fr[-1]))
        if not done:
            return []
        scores = self.model.score(np.stack(xs))
        return [(pid, a, b, float(s)) for (pid, a, b), s in zip(done, scores)]
