"""TEST INFRASTRUCTURE: the Shopformer score path evaluated in numpy (float64 by default) from the FOLDED weight image that the
kernel reads (cvsd_amd.shopformer.parse_image: geometry + logical tensors, matrices unpacked from the MFMA fragment order).
Reproducing the reference's float64 outputs from it proves the BatchNorm folding, the packing, the three-token stride rule, the
unmasked decoder and the PE-shifted target without a GPU."""
import numpy as np


def _ln(x, g, b):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + 1e-5) * g + b


def _lin(x, t, name):
    return x @ t[name + ".w"][:, 0, :].T + t[name + ".b"][:t[name + ".w"].shape[0]]


def _mha(q_in, kv_in, t, name, heads):
    d = q_in.shape[-1]
    q = _lin(q_in, t, name + ".q")
    kv = _lin(kv_in, t, name + ".kv")
    k, v = kv[..., :d], kv[..., d:]
    n, s, hd = q.shape[0], q.shape[1], d // heads
    sp = lambda a: a.reshape(n, -1, heads, hd).transpose(0, 2, 1, 3)
    q, k, v = sp(q), sp(k), sp(v)
    a = q @ k.transpose(0, 1, 3, 2) / q.dtype.type(np.sqrt(hd))             # a scalar of the evaluation's own type: float32 stays float32
    a = np.exp(a - a.max(-1, keepdims=True))
    a = a / a.sum(-1, keepdims=True)
    o = (a @ v).transpose(0, 2, 1, 3).reshape(n, s, d)
    return _lin(o, t, name + ".out")


def forward(geo, tensors, windows, dtype=np.float64):
    t = {k: np.asarray(v, dtype) for k, v in tensors.items()}
    V, H, L, D, ntok = geo["V"], geo["H"], geo["L"], geo["D"], geo["ntok"]
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
        tin = h.shape[2]
        tout = (tin - 1) // s + 1
        hp = np.pad(h, ((0, 0), (0, 0), (4, 4), (0, 0)))
        y = np.zeros((n, co, tout, V), dtype)
        for k in range(9):
            y += np.einsum("nctv,oc->notv", hp[:, :, k:k + s * (tout - 1) + 1:s], t[f"b{i}.tw"][:, k, :])
        x = np.maximum(y + t[f"b{i}.tb"][:co].reshape(1, -1, 1, 1) + res, 0)
    assert x.shape == (n, L, ntok, V)
    tokens = x.transpose(0, 2, 1, 3).reshape(n, ntok, D)
    heads = geo["heads"]
    src = tokens + t["pe_in"]
    for e in range(geo["layers"]):
        src = _ln(src + _mha(src, src, t, f"e{e}.sa", heads), t[f"e{e}.n1.g"][:D], t[f"e{e}.n1.b"][:D])
        ff = _lin(np.maximum(_lin(src, t, f"e{e}.f1"), 0), t, f"e{e}.f2")
        src = _ln(src + ff, t[f"e{e}.n2.g"][:D], t[f"e{e}.n2.b"][:D])
    tgt = np.concatenate([np.zeros((n, 1, D), dtype), tokens[:, :-1]], 1) + t["pe_in"]
    for e in range(geo["layers"]):
        tgt = _ln(tgt + _mha(tgt, tgt, t, f"d{e}.sa", heads), t[f"d{e}.n1.g"][:D], t[f"d{e}.n1.b"][:D])
        tgt = _ln(tgt + _mha(tgt, src, t, f"d{e}.ca", heads), t[f"d{e}.n2.g"][:D], t[f"d{e}.n2.b"][:D])
        ff = _lin(np.maximum(_lin(tgt, t, f"d{e}.f1"), 0), t, f"d{e}.f2")
        tgt = _ln(tgt + ff, t[f"d{e}.n3.g"][:D], t[f"d{e}.n3.b"][:D])
    rec = _lin(tgt, t, "proj")
    score = ((rec - (tokens + t["pe_score"])) ** 2).mean(axis=(1, 2))
    return {"normality_score": score, "tokens": tokens, "reconstructed_tokens": rec}


from tools.synth_shopformer import fixture_model, load_fixture  # noqa: E402,F401  (the fixture's readers live beside its generator)
