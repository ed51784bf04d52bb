"""TEST INFRASTRUCTURE: the ``shopformer_2`` score path evaluated in numpy (float64 by default) from the FOLDED version-2 weight image
(cvsd_amd.shopformer.parse_image).  Reproducing the reference's float64 outputs from it proves, without a GPU, the BatchNorm folding,
the packing, the restated stride rule, the pre-norm layer order with its two final norms, the erf GELU, the optional projections,
the decoder fed from the encoder's own input, and the score without positional encoding."""
import math

import numpy as np

from _shopformer_numpy import _lin, _ln, _mha

_erf = np.vectorize(math.erf, otypes=[np.float64])


def _gelu(x):
    return (0.5 * x * (1.0 + _erf(np.asarray(x, np.float64) / math.sqrt(2.0)))).astype(x.dtype)


def tokenizer(geo, t, windows, dtype):
    V, H, L = geo["V"], geo["H"], geo["L"]
    x = np.asarray(windows, dtype)                                              # [N, 2, T, V]
    n = len(x)
    x = x * t["in_scale"][:2 * V].reshape(1, 2, 1, V) + t["in_shift"][:2 * V].reshape(1, 2, 1, V)
    adj = np.zeros((V, V), dtype)
    for v in range(V):
        for c, a in zip(t["adj_col"][v].astype(int), t["adj_val"][v]):
            adj[v, c] += a
    chans = [2, H, H, H, L]
    for i in range(4):
        s, co = geo[f"s{i}"], chans[i + 1]
        if f"b{i}.rw" in t:
            res = np.einsum("nctv,oc->notv", x[:, :, ::s], t[f"b{i}.rw"][:, 0, :]) + t[f"b{i}.rb"][:co].reshape(1, -1, 1, 1)
        else:
            res = x
        h = np.einsum("vu,nctu->nctv", adj, x)
        h = np.einsum("nctv,oc->notv", h, t[f"b{i}.gw"][:, 0, :]) + t[f"b{i}.gb"][:co].reshape(1, -1, 1, 1)
        h = np.maximum(h, 0)
        tout = (h.shape[2] - 1) // s + 1
        assert tout == geo[f"T{i + 1}"]
        hp = np.pad(h, ((0, 0), (0, 0), (4, 4), (0, 0)))
        y = np.zeros((n, co, tout, V), dtype)
        for k in range(9):
            y += np.einsum("nctv,oc->notv", hp[:, :, k:k + s * (tout - 1) + 1:s], t[f"b{i}.tw"][:, k, :])
        x = np.maximum(y + t[f"b{i}.tb"][:co].reshape(1, -1, 1, 1) + res, 0)
    assert x.shape == (n, L, geo["ntok"], V)
    return x.transpose(0, 2, 1, 3).reshape(n, geo["ntok"], L * V)


def forward(geo, tensors, windows, dtype=np.float64):
    assert geo.get("variant") == 2 and geo["norm_kind"] == 1 and geo["act_kind"] == 1
    t = {k: np.asarray(v, dtype) for k, v in tensors.items()}
    D, heads = geo["D"], geo["heads"]
    tokens = tokenizer(geo, t, windows, dtype)
    assert tokens.shape[-1] == geo["Din"]
    n = lambda x, name: _ln(x, t[name + ".g"][:D], t[name + ".b"][:D])
    x0 = (_lin(tokens, t, "inp") if geo["in_proj"] else tokens) + t["pe_in"]
    src = x0
    for e in range(geo["layers"]):
        y = n(src, f"e{e}.n1")
        src = src + _mha(y, y, t, f"e{e}.sa", heads)
        src = src + _lin(_gelu(_lin(n(src, f"e{e}.n2"), t, f"e{e}.f1")), t, f"e{e}.f2")
    mem = n(src, "en")
    tgt = x0
    for e in range(geo["layers"]):
        y = n(tgt, f"d{e}.n1")
        tgt = tgt + _mha(y, y, t, f"d{e}.sa", heads)
        tgt = tgt + _mha(n(tgt, f"d{e}.n2"), mem, t, f"d{e}.ca", heads)
        tgt = tgt + _lin(_gelu(_lin(n(tgt, f"d{e}.n3"), t, f"d{e}.f1")), t, f"d{e}.f2")
    rec = n(tgt, "dn")
    if geo["out_proj"]:
        rec = _lin(rec, t, "outp")
    ts = ((tokens - rec) ** 2).mean(axis=2)
    return {"normality_score": ((tokens - rec) ** 2).mean(axis=(1, 2)), "token_scores": ts, "tokens": tokens, "reconstructed_tokens": rec}


from tools.synth_shopformer2 import fixture_model, load_fixture  # noqa: E402,F401  (the fixture's readers live beside its generator)
