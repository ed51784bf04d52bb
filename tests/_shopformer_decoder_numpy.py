"""TEST INFRASTRUCTURE: the GCAE decoder evaluated in numpy (float64 by default) from a parsed version-3 weight image
(cvsd_amd.shopformer.parse_image).  Reproducing the reference's float64 poses from it proves, without a GPU, the BatchNorm fold of
the decoder's layers, the (joint, channel) reordering of initial_proj, the parity matrices of the transposed convolutions, the
factor rule and the interpolation formula.

The interpolation is restated here exactly as the kernel fixes it (align_corners=False along time; the joint axis maps V -> V with
zero fractional weight): in float32, ``scale = Td / T``, ``src = max(scale * (t + 0.5) - 0.5, 0)``, ``i0 = min(int(src), Td - 1)``,
``i1 = min(i0 + 1, Td - 1)``, ``w = src - i0``; then ``(1 - w) * a + w * b`` with each operation rounded on its own."""
import numpy as np

from tools.synth_shopformer_decoder import fixture_model, load_fixture  # noqa: F401  (the fixture's readers live beside its generator)


def interp_table(Td: int, T: int):
    """-> (i0 [T] int, i1 [T] int, w [T] float32), the kernel's float32 arithmetic"""
    f32 = np.float32
    scale = f32(Td) / f32(T)
    t = np.arange(T, dtype=f32)
    src = np.maximum(scale * (t + f32(0.5)) - f32(0.5), f32(0))
    assert src.dtype == np.float32
    i0 = np.minimum(src.astype(np.int64), Td - 1)
    i1 = np.minimum(i0 + 1, Td - 1)
    return i0, i1, (src - i0.astype(f32)).astype(f32)


def layers(geo, tensors, tokens, dtype=np.float64):
    """tokens [N, ntok, L*V] -> what the four layers emit, [N, 2, Tdec, V] (before the interpolation)"""
    t = {k: np.asarray(v, dtype) for k, v in tensors.items() if k.startswith("dec.")}
    V, H, ntok = geo["V"], geo["H"], geo["ntok"]
    x = np.asarray(tokens, dtype)
    n = len(x)
    assert x.shape[1:] == (ntok, geo["L"] * V)
    x = x @ t["dec.ip.w"][:, 0, :].T + t["dec.ip.b"][:V * H]                 # [N, ntok, V * H], features in (joint, channel) order
    x = x.reshape(n, ntok, V, H)                                              # [N, frames, V, channels]
    for i in range(4):
        w, f = t[f"dec.l{i}.w"], geo[f"u{i}"]
        co = w.shape[0]
        assert w.shape[1] == f
        y = np.einsum("nfvc,opc->nfpvo", x, w) + t[f"dec.l{i}.b"][:co]       # frame f * factor + parity
        x = y.reshape(n, x.shape[1] * f, V, co)
        if i < 3:
            x = np.maximum(x, 0)
    assert x.shape == (n, geo["Tdec"], V, 2)
    return x.transpose(0, 3, 1, 2)


def interpolate(geo, y, dtype=np.float64):
    """[N, 2, Tdec, V] -> [N, 2, T, V] by the formula of the module docstring (``dtype=np.float32``: the kernel's own rounding)"""
    if not geo["interp"]:
        assert geo["Tdec"] == geo["T"]
        return np.asarray(y, dtype)
    i0, i1, w = interp_table(geo["Tdec"], geo["T"])
    y = np.asarray(y, dtype)
    w1 = w.astype(dtype).reshape(1, 1, -1, 1)
    w0 = (np.float32(1) - w).astype(dtype).reshape(1, 1, -1, 1)
    return w0 * y[:, :, i0] + w1 * y[:, :, i1]


def decode(geo, tensors, tokens, dtype=np.float64):
    return interpolate(geo, layers(geo, tensors, tokens, dtype), dtype)


def pose_error_f32(poses, windows):
    """the kernel's stated order in float32: d = pose - window per channel; 0.5 * (d0 * d0 + d1 * d1), every operation rounded"""
    p, x = np.asarray(poses, np.float32), np.asarray(windows, np.float32)
    d0, d1 = p[:, 0] - x[:, 0], p[:, 1] - x[:, 1]
    return np.float32(0.5) * (d0 * d0 + d1 * d1)
