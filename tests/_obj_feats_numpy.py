"""Reference of the object-feature gather (csrc/post_kernels.hip:obj_feats_kernel): Ultralytics' DetectionPredictor.get_obj_feats
(8.3.225, restated) in the canonical arithmetic the kernel is pinned to.

``s = min(C_l)``; per level ``x.permute(0, 2, 3, 1).reshape(B, -1, s, C_l // s).mean(-1)``, levels concatenated along the anchor axis
(P3 row-major, then P4, then P5), rows taken at the kept anchors.  The mean over a group of g consecutive channels is the SEQUENTIAL
float32 sum ``acc = x[0]; acc += x[r]`` for ascending r, then ``acc / float32(g)`` (IEEE division); g = 1 copies the bits.  fp16 maps are
widened to float32 first.  numpy's ``+`` and ``/`` on float32 arrays are single correctly rounded operations, so stating the order
elementwise over the group axis gives the same bits on any machine.
"""
import numpy as np


def group_mean(x: np.ndarray, s: int) -> np.ndarray:
    """x [..., C] float32 or float16 -> [..., s] float32, C = s * g"""
    c = x.shape[-1]
    assert c % s == 0
    g = c // s
    v = x.astype(np.float32).reshape(*x.shape[:-1], s, g)
    if g == 1:
        return v[..., 0].copy()
    acc = v[..., 0].copy()
    for r in range(1, g):
        acc = (acc + v[..., r]).astype(np.float32)
    return (acc / np.float32(g)).astype(np.float32)


def obj_feats(levels, anchor_idx: np.ndarray, counts: np.ndarray, fill: np.ndarray) -> np.ndarray:
    """levels: [(buf [n, h, w, cs], c_off, C)], NHWC; anchor_idx [n, cap]; counts [n]; fill: what rows at or beyond the count hold.
    -> [n, cap, s] float32"""
    s = min(c for _, _, c in levels)
    n, cap = anchor_idx.shape
    per_level = [group_mean(buf[..., off:off + c].reshape(n, -1, c), s) for buf, off, c in levels]
    table = np.concatenate(per_level, axis=1)                  # [n, A, s]
    out = np.empty((n, cap, s), np.float32)
    out.view(np.uint32)[:] = np.asarray(fill).view(np.uint32)
    for i in range(n):
        k = int(counts[i])
        out[i, :k] = table[i, anchor_idx[i, :k]]
    return out
