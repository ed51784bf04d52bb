"""numpy wrappers over the single-operator C-ABI entry points (``mi355_op_*``).

They exist so the parity tests can isolate one HIP kernel at a time; each call goes to the GPU
(there is no CPU implementation behind them).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .sources import DeviceFrame, Ragged, bgr_view, one_or_many, wait_for_torch  # noqa: F401  (DeviceFrame: part of this module's surface)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def conv2d(x_nhwc: np.ndarray, w_oihw: np.ndarray, bias: np.ndarray, stride: int = 1, silu: bool = True,
           residual: Optional[np.ndarray] = None, device: int = 0, plan: int = 0, return_n_plans: bool = False,
           half: bool = False, out_f32: bool = False):
    """Fused conv + bias (+SiLU) (+residual): x [N,H,W,Cin] fp32 -> [N,H/s,W/s,Cout].
    ``plan`` picks one of the engine's candidate launch plans (all must give identical bits).
    ``half``: the half=True kernels -- x, w, residual rounded to fp16, fp32 accumulate, y rounded to fp16 once
    (``out_f32``: y kept in fp32, as for the head's final convs); values are returned as fp32 either way."""
    x, w, b = _f32(x_nhwc), _f32(w_oihw), _f32(bias)
    n, h, wd, cin = x.shape
    cout, cin2, k, k2 = w.shape
    if cin2 != cin or k != k2 or b.shape != (cout,):
        raise ValueError("shape mismatch between x, w and bias")
    y = np.empty((n, h // stride, wd // stride, cout), dtype=np.float32)
    npl = C.c_int(0)
    r = None
    if residual is not None:
        r = _f32(residual)
        if r.shape != y.shape:
            raise ValueError("residual must have the output's shape")
    if half:
        _lib.check(_lib.lib().mi355_op_conv2d_f16(device, x.ctypes.data, n, h, wd, cin, w.ctypes.data, b.ctypes.data, cout,
                                                  k, stride, int(silu), r.ctypes.data if r is not None else None,
                                                  y.ctypes.data, int(out_f32), int(plan), C.byref(npl)))
        return (y, npl.value) if return_n_plans else y
    _lib.check(_lib.lib().mi355_op_conv2d(device, x.ctypes.data, n, h, wd, cin, w.ctypes.data, b.ctypes.data, cout, k,
                                          stride, int(silu), r.ctypes.data if r is not None else None, y.ctypes.data,
                                          int(plan), C.byref(npl)))
    return (y, npl.value) if return_n_plans else y


def conv2d_subrange(x_nhwc: np.ndarray, w_oihw: np.ndarray, bias: np.ndarray, t0: int, y_in: np.ndarray, silu: bool = True,
                    device: int = 0, plan: int = 0):
    """The 3x3 / stride 1 conv launched over its cout tiles [t0, last] alone (tiles of 16 couts), as the engine launches the class
    couts of a merged head conv in a sparse pass: -> (y, n_plans, tile).  ``y_in`` [N,H,W,Cout] is what the output buffer holds before
    the launch (couts below 16 * t0 must come back untouched); ``tile`` is the launch's geometry as in :func:`plan_tiles`."""
    x, w, b = _f32(x_nhwc), _f32(w_oihw), _f32(bias)
    n, h, wd, cin = x.shape
    cout = w.shape[0]
    if w.shape != (cout, cin, 3, 3) or b.shape != (cout,) or y_in.shape != (n, h, wd, cout):
        raise ValueError("shape mismatch between x, w, bias and y_in")
    y = np.array(y_in, dtype=np.float32, order="C", copy=True)
    npl, tile = C.c_int(0), (C.c_int * len(PLAN_TILE_FIELDS))()
    _lib.check(_lib.lib().mi355_op_conv2d_subrange(device, x.ctypes.data, n, h, wd, cin, w.ctypes.data, b.ctypes.data, cout, int(silu),
                                                   int(t0), y.ctypes.data, int(plan), C.byref(npl), tile))
    p = dict(zip(PLAN_TILE_FIELDS, tile))
    p["P"] = p["WP"] * p["PT"] * 16
    p["tiles_x"], p["tiles_y"] = -(-wd // p["TW"]), -(-h // p["TH"])
    return y, npl.value, p


def conv1x1_upcat(x_half: np.ndarray, x_skip: np.ndarray, w_oihw: np.ndarray, bias: np.ndarray, silu: bool = True, device: int = 0,
                  plan: int = 0, return_n_plans: bool = False, half: bool = False):
    """Pointwise conv over cat(upsample2x(x_half), x_skip) with the upsample fused into the read side (fp32):
    x_half [N,H/2,W/2,Cu], x_skip [N,H,W,Cs], w [Cout,Cu+Cs,1,1] -> [N,H,W,Cout].  ``half``: the half=True kernels."""
    xh, xs, w, b = _f32(x_half), _f32(x_skip), _f32(w_oihw), _f32(bias)
    n, h, wd, cs = xs.shape
    cu, cout = xh.shape[3], w.shape[0]
    if xh.shape != (n, h // 2, wd // 2, cu) or w.shape != (cout, cu + cs, 1, 1) or b.shape != (cout,):
        raise ValueError("shape mismatch")
    y = np.empty((n, h, wd, cout), dtype=np.float32)
    npl = C.c_int(0)
    fn = _lib.lib().mi355_op_conv1x1_upcat_f16 if half else _lib.lib().mi355_op_conv1x1_upcat
    _lib.check(fn(device, xh.ctypes.data, xs.ctypes.data, n, h, wd, cu, cs, w.ctypes.data, b.ctypes.data,
                                                 cout, int(silu), y.ctypes.data, int(plan), C.byref(npl)))
    return (y, npl.value) if return_n_plans else y


def dwconv2d(x_nhwc: np.ndarray, w_c1kk: np.ndarray, bias: np.ndarray, silu: bool = True, residual: Optional[np.ndarray] = None,
             x_off: int = 0, c: Optional[int] = None, res_off: int = 0, y: Optional[np.ndarray] = None, y_off: int = 0,
             device: int = 0) -> np.ndarray:
    """Depthwise k x k conv (stride 1, pad k/2) + bias (+SiLU) (+residual) on channel views (YOLO11 DWConv / Attention.pe):
    reads channels x_off .. x_off+c-1 of x [N,H,W,Cx] (and res_off .. of residual [N,H,W,Cr]), writes channels y_off .. of
    y [N,H,W,Cy] (a copy of ``y`` if given, else zeros [N,H,W,c]); the other channels of y come back unchanged."""
    x, w, b = _f32(x_nhwc), _f32(w_c1kk), _f32(bias)
    n, h, wd, cx = x.shape
    c = w.shape[0] if c is None else c
    k = w.shape[2]
    if w.shape != (c, 1, k, k) or b.shape != (c,):
        raise ValueError("shape mismatch between w, bias and the channel count")
    out = np.zeros((n, h, wd, c), np.float32) if y is None else np.array(y, dtype=np.float32, order="C", copy=True)
    r = _f32(residual) if residual is not None else None
    _lib.check(_lib.lib().mi355_op_dwconv2d(device, x.ctypes.data, n, h, wd, cx, x_off, c, w.ctypes.data, b.ctypes.data, k, int(silu),
                                            r.ctypes.data if r is not None else None, r.shape[3] if r is not None else 0, res_off,
                                            out.ctypes.data, out.shape[3], y_off))
    return out


# What decode / sppf_pools / upsample2x put into outputs before the launch: a quiet NaN with a payload no kernel produces, so a
# word the kernel did not write is told apart from any value it could have written (compare the bits, NaN != NaN).
SENTINEL_BITS = np.uint32(0x7FC5A5A5)
SENTINEL = SENTINEL_BITS.view(np.float32)
DECODE_MODES = {"full": 0, "nms": 1, "split": 2}


def _sentinel(shape) -> np.ndarray:
    return np.full(shape, SENTINEL_BITS, dtype=np.uint32).view(np.float32)


def decode(levels, nc: int, nkpt: int = 0, kdim: int = 0, mode: str = "full", gate: Optional[int] = None, device: int = 0):
    """The head decode kernel alone (DFL + dist2bbox, class scores -> best score / first argmax, keypoints), fp32.
    ``levels``: up to 4 tuples ``(buf [n,h,w,cs] fp32, box_off, cls_off, kpt_off, stride)``: 64 box logits, nc class logits and
    nkpt*kdim keypoint values of each pixel sit at those channel offsets of ``buf``.
    ``mode``: "full" = the raw-head form (every class score stored); "nms" = the form predict() runs (box, keypoints, best);
    "split" = the sparse box branch's pair: score stage, then the box stage behind a device gate word set to ``gate``.
    -> (pred [n, A, 4+nc+nkpt*kdim], best [n, A, 2]) and, for "split", the box stage's fallback counter.  Both arrays are filled
    with SENTINEL before the launch."""
    if mode not in DECODE_MODES:
        raise ValueError(f"mode must be one of {sorted(DECODE_MODES)}")
    if (mode == "split") != (gate is not None):
        raise ValueError("gate is the split mode's argument (and it needs one)")
    levels = list(levels)
    if not 1 <= len(levels) <= 4:
        raise ValueError("decode takes 1 to 4 levels")
    if nc <= 0 or nkpt < 0 or (kdim not in (2, 3) if nkpt else kdim != 0):
        raise ValueError("nc must be positive; kdim 2 or 3 with keypoints, 0 without")
    nk = nkpt * kdim
    no = 4 + nc + nk
    bufs, geom, anchors, n = [], [], 0, None
    for buf, box_off, cls_off, kpt_off, stride in levels:
        b = _f32(buf)
        if b.ndim != 4 or (n is not None and b.shape[0] != n):
            raise ValueError("every level is [n, h, w, cs] with the same n")
        n, h, w, cs = b.shape
        if min(n, h, w) <= 0 or stride <= 0:
            raise ValueError("empty level or non-positive stride")
        if box_off < 0 or box_off + 64 > cs or cls_off < 0 or cls_off + nc > cs or (nk and (kpt_off < 0 or kpt_off + nk > cs)):
            raise ValueError("a level's box / class / keypoint slice lies outside its cs channels")
        bufs.append(b)
        geom += [cs, box_off, cls_off, kpt_off, h, w, stride]
        anchors += h * w
    pred = _sentinel((n, anchors, no))
    best = _sentinel((n, anchors, 2))
    ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
    g = (C.c_int * len(geom))(*[int(v) for v in geom])
    count = C.c_int(-1)
    _lib.check(_lib.lib().mi355_op_decode(device, ptrs, g, len(bufs), n, nc, nkpt, kdim, DECODE_MODES[mode], int(gate or 0),
                                          pred.ctypes.data, best.ctypes.data, C.byref(count)))
    return (pred, best, count.value) if mode == "split" else (pred, best)


def obj_feats(levels, anchor_idx, counts, half: bool = False, device: int = 0) -> np.ndarray:
    """The object-feature gather alone (csrc/post_kernels.hip).  ``levels``: 1 to 4 tuples ``(buf [n,h,w,cs], c_off, C)``,
    the level's channels at ``c_off .. c_off + C - 1`` of ``buf``; fp32 arrays, or with ``half`` float16 arrays (all levels alike).
    ``anchor_idx`` int32 [n, cap] (P3 row-major first), ``counts`` [n].  -> float32 [n, cap, s], s = min(C): row r of frame i =
    the group means of its anchor's channels for r < counts[i]; the rest keeps SENTINEL, which fills the output before the launch."""
    levels = list(levels)
    if not 1 <= len(levels) <= 4:
        raise ValueError("obj_feats takes 1 to 4 levels")
    want = np.float16 if half else np.float32
    bufs, geom, n = [], [], None
    for buf, c_off, c in levels:
        b = np.ascontiguousarray(buf)
        if b.dtype != want or b.ndim != 4 or (n is not None and b.shape[0] != n):
            raise ValueError(f"every level is a {np.dtype(want).name} array [n, h, w, cs] with the same n")
        n = b.shape[0]
        bufs.append(b)
        geom += [b.shape[3], int(c_off), int(c), b.shape[1], b.shape[2]]
    idx = np.ascontiguousarray(anchor_idx, dtype=np.int32)
    cnt = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if idx.ndim != 2 or idx.shape[0] != n or len(cnt) != n:
        raise ValueError("anchor_idx is [n, cap] and counts [n]")
    dim = min(int(c) for _, _, c in levels)
    out = _sentinel((n, idx.shape[1], dim))
    ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
    g = (C.c_int * len(geom))(*[int(v) for v in geom])
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    _lib.check(_lib.lib().mi355_op_obj_feats(device, ptrs, g, len(bufs), n, int(bool(half)), i32(idx), i32(cnt), idx.shape[1], dim,
                                             out.ctypes.data))
    return out


def pose_array(poses):
    """-> (poses as a C-contiguous [P, V_src, 2] array, its MI355_POSE_* code); anything but float32 / float64 is refused, because the
    window arithmetic runs in the poses' own type"""
    p = np.asarray(poses)
    if p.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"poses must be float32 or float64, got {p.dtype}")
    if p.ndim != 3 or p.shape[2] != 2:
        raise ValueError(f"poses must be [P, V_src, 2] (x, y), got {tuple(p.shape)}")
    return np.ascontiguousarray(p), (_lib.POSE_F64 if p.dtype == np.float64 else _lib.POSE_F32)


def pose_windows(poses: np.ndarray, starts, seq_len: int, num_keypoints: int, neck: bool = False, device: int = 0) -> np.ndarray:
    """The pose-window kernel alone (csrc/pose_windows.hip): ``poses`` [P, V_src, 2] float32 or float64, window i = the ``seq_len``
    consecutive poses from ``starts[i]`` -> [n, 2, seq_len, num_keypoints] float32, the bits ``shopformer._window_tensor`` gives for
    those poses.  ``device=-1`` runs the kernel's per-window routine compiled for the host (no GPU is touched).  Starts that leave
    the array, ``neck`` without 18 keypoints or without both shoulders are refused before any launch (ValueError).  The output is
    filled with SENTINEL before the launch."""
    p, code = pose_array(poses)
    st = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1)
    out = _sentinel((len(st), 2, int(seq_len), int(num_keypoints)))
    _lib.check(_lib.lib().mi355_pose_windows(int(device), p.ctypes.data, code, p.shape[0], p.shape[1], st.ctypes.data, len(st), int(seq_len),
                                             int(num_keypoints), int(bool(neck)), out.ctypes.data))
    return out


def tile_overlap_px(tile, overlap: float):
    """``tile`` (int or (tile_h, tile_w)) and the fractional ``overlap`` of ``predict(tile=...)`` -> (tile_h, tile_w, overlap_y_px,
    overlap_x_px): the overlap is turned into pixels once, here, as ``int(overlap * tile)`` per axis; the C ABI takes pixels.  Refuses
    (TypeError / ValueError naming the argument) a tile that is no int or pair of ints or is below 32, and an overlap outside [0, 1)."""
    if isinstance(tile, (bool, float)) or (not isinstance(tile, (int, np.integer)) and not (
            isinstance(tile, (tuple, list)) and len(tile) == 2 and all(isinstance(t, (int, np.integer)) and not isinstance(t, bool) for t in tile))):
        raise TypeError(f"tile must be an int or (tile_h, tile_w), got {tile!r}")
    th, tw = (int(tile), int(tile)) if isinstance(tile, (int, np.integer)) else (int(tile[0]), int(tile[1]))
    if th < 32 or tw < 32:
        raise ValueError(f"tile must be >= 32, got {tile!r}")
    if isinstance(overlap, bool) or not isinstance(overlap, (int, float, np.integer, np.floating)):
        raise TypeError(f"overlap must be a number in [0, 1), got {overlap!r}")
    if not 0 <= float(overlap) < 1:
        raise ValueError(f"overlap must be in [0, 1), got {overlap!r}")
    return th, tw, int(float(overlap) * th), int(float(overlap) * tw)


def tile_grid(height: int, width: int, tile, overlap: float = 0.2) -> np.ndarray:
    """The tile grid of ``predict(tile=..., overlap=...)`` for a ``height`` x ``width`` frame (``mi355_tile_grid``, host arithmetic
    only): int32 [T, 4] rows x, y, w, h, row-major (y outer, x inner)."""
    th, tw, oy, ox = tile_overlap_px(tile, overlap)
    cnt = C.c_int()
    _lib.check(_lib.lib().mi355_tile_grid(int(height), int(width), th, tw, oy, ox, None, 0, C.byref(cnt)))
    out = np.zeros((cnt.value, 4), np.int32)
    _lib.check(_lib.lib().mi355_tile_grid(int(height), int(width), th, tw, oy, ox, out.ctypes.data, cnt.value, C.byref(cnt)))
    return out


TILE_METRICS = {"ios": _lib.TILE_IOS, "iou": _lib.TILE_IOU}


def tile_merge(rows: np.ndarray, counts, origins, kdim: int = 0, metric: str = "ios", thr: float = 0.5, device: int = 0):
    """The merge kernel of a tiled predict alone (csrc/post_kernels.hip: one block per source frame): ``rows`` float32
    [F, E, max_det, 58] (the words of ``mi355_det``; cls and anchor_idx are int32 bits), ``counts`` [F, E], ``origins`` [F, E, 2] = x, y
    of every entry -> (merged rows [F, max_det, 58], counts [F], tile_idx int32 [F, max_det]).  Slots at or beyond a frame's count come
    back as SENTINEL_BITS (tile_idx: -1).  ``device=-1`` runs the same per-frame routine on the host (no GPU is touched)."""
    r = np.ascontiguousarray(rows, dtype=np.float32)
    if r.ndim != 4 or r.shape[3] != _lib.DET_WORDS:
        raise ValueError(f"rows must be [F, E, max_det, {_lib.DET_WORDS}], got {tuple(r.shape)}")
    F, E, md = r.shape[:3]
    cnt = np.ascontiguousarray(counts, dtype=np.int32).reshape(F, E)
    org = np.ascontiguousarray(origins, dtype=np.int32).reshape(F, E, 2)
    if metric not in TILE_METRICS:
        raise ValueError(f"tile_metric must be 'ios' or 'iou', got {metric!r}")
    out = _sentinel((F, md, _lib.DET_WORDS))
    oc = np.zeros(F, np.int32)
    idx = np.full((F, md), -1, np.int32)
    _lib.check(_lib.lib().mi355_op_tile_merge(int(device), r.ctypes.data, cnt.ctypes.data, org.ctypes.data, F, E, md, int(kdim),
                                              TILE_METRICS[metric], float(thr), out.ctypes.data, oc.ctypes.data, idx.ctypes.data))
    return out, oc, idx


class SparseBoxResult:
    """What :func:`sparse_box` hands back: ``pred`` [n, A, no]; per level ``mid`` [n, h, w, mid_cs], ``dil`` / ``cand`` (the first
    min(count, cap) list entries, int32, in the kernel's order), ``n_dil`` / ``n_cand`` (the counts the device holds, also beyond
    the caps); ``overflow`` (the device's overflow word)."""

    def __init__(self, pred, mid, dil, cand, n_dil, n_cand, overflow):
        self.pred, self.mid, self.dil, self.cand = pred, mid, dil, cand
        self.n_dil, self.n_cand, self.overflow = n_dil, n_cand, overflow


def sparse_box(levels, best: np.ndarray, conf: float, nc: int, no: Optional[int] = None, classes: Optional[Sequence[int]] = None,
               act: int = 1, device: int = 0) -> SparseBoxResult:
    """The sparse box branch alone (the lists kernel and the two gathered convs of csrc/conv_f32_sparse.hip), enqueued as a pass
    enqueues its sparse tail minus the dense launches.  ``levels``: 1 to 3 dicts with
    ``src`` [n,h,w,cs] fp32 (the neck map at channels ``src_off`` .. ``src_off + cin``, cin a multiple of 16; default: all of src),
    ``wA, bA`` (cv2.i.0, OIHW [>= 64, cin, 3, 3]: the first 64 couts are used, a merged cv3.i.0 may follow), ``wB, bB``
    ([64, 64, 3, 3]), ``wC, bC`` ([64, 64, 1, 1]), ``stride``, ``mid_cs`` / ``mid_off`` (default 64 / 0) and ``cap_dil`` /
    ``cap_cand`` (default: every position).  ``best`` [n, A, 2] (score, class) is the caller's; ``conf`` and ``classes`` filter as
    NMS does.  ``pred`` [n, A, no] (``no`` defaults to 4 + nc) and every ``mid`` are filled with SENTINEL before the launch."""
    levels = list(levels)
    if not 1 <= len(levels) <= 3:
        raise ValueError("sparse_box takes 1 to 3 levels")
    no = 4 + nc if no is None else no
    if nc <= 0 or no < 4 + nc:
        raise ValueError("nc must be positive and no at least 4 + nc")
    if act not in (0, 1, 2):
        raise ValueError("act must be 0 (none), 1 (SiLU) or 2 (fast SiLU)")
    keep, ptrs, geom, mids, dils, cands, anchors, n = [], [], [], [], [], [], 0, None
    for lv in levels:
        src = _f32(lv["src"])
        if src.ndim != 4 or (n is not None and src.shape[0] != n):
            raise ValueError("every level's src is [n, h, w, cs] with the same n")
        n, h, w, cs = src.shape
        stride, src_off, cin = int(lv["stride"]), int(lv.get("src_off", 0)), int(lv.get("cin", cs))
        mid_cs, mid_off = int(lv.get("mid_cs", 64)), int(lv.get("mid_off", 0))
        if min(n, h, w) <= 0 or stride <= 0:
            raise ValueError("empty level or non-positive stride")
        if cin <= 0 or cin % 16:
            raise ValueError("cin must be a positive multiple of 16")
        _check_view("src", cs, src_off, cin, 4)
        _check_view("mid", mid_cs, mid_off, 64, 4)
        wA, bA, wB, bB, wC, bC = (_f32(lv[k]) for k in ("wA", "bA", "wB", "bB", "wC", "bC"))
        cout_a = wA.shape[0]
        if wA.shape != (cout_a, cin, 3, 3) or cout_a < 64 or bA.shape != (cout_a,):
            raise ValueError("wA must be [>= 64, cin, 3, 3] with a bias per cout")
        if wB.shape != (64, 64, 3, 3) or bB.shape != (64,) or wC.shape != (64, 64, 1, 1) or bC.shape != (64,):
            raise ValueError("wB must be [64, 64, 3, 3], wC [64, 64, 1, 1], each with 64 biases")
        pos = n * h * w
        cap_dil = pos if lv.get("cap_dil") is None else int(lv["cap_dil"])
        cap_cand = pos if lv.get("cap_cand") is None else int(lv["cap_cand"])
        if not (1 <= cap_dil <= pos and 1 <= cap_cand <= pos):
            raise ValueError("list capacities must lie in 1 .. n*h*w")
        mid, dil, cand = _sentinel((n, h, w, mid_cs)), np.full(cap_dil, -1, np.int32), np.full(cap_cand, -1, np.int32)
        arrs = [src, wA, bA, wB, bB, wC, bC, mid, dil, cand]
        keep.append(arrs)
        ptrs += [a.ctypes.data for a in arrs]
        geom += [h, w, cs, src_off, cin, cout_a, stride, mid_cs, mid_off, cap_dil, cap_cand]
        mids.append(mid); dils.append(dil); cands.append(cand)
        anchors += h * w
    bst = _f32(best)
    if bst.shape != (n, anchors, 2):
        raise ValueError("best must be [n, A, 2] with A the levels' positions per frame")
    cls_arr, ncls = None, 0
    if classes is not None:
        cls_arr = (C.c_int * len(classes))(*[int(c) for c in classes])
        ncls = len(classes)
        if ncls and not ((bst[..., 1] >= 0) & (bst[..., 1] < nc)).all():
            raise ValueError("with a class list every class of best[] must lie in 0 .. nc-1")
    pred = _sentinel((n, anchors, no))
    state = (C.c_int * 12)()
    p = (C.c_void_p * len(ptrs))(*ptrs)
    g = (C.c_int * len(geom))(*[int(v) for v in geom])
    _lib.check(_lib.lib().mi355_op_sparse_box(device, p, g, len(levels), n, bst.ctypes.data, float(conf), cls_arr, ncls, nc, no, int(act),
                                              pred.ctypes.data, state))
    nl = len(levels)
    n_dil, n_cand = [state[l] for l in range(nl)], [state[4 + l] for l in range(nl)]
    dils = [d[:max(0, min(c, len(d)))].copy() for d, c in zip(dils, n_dil)]
    cands = [d[:max(0, min(c, len(d)))].copy() for d, c in zip(cands, n_cand)]
    return SparseBoxResult(pred, mids, dils, cands, n_dil, n_cand, state[8])


def _check_view(name: str, cs: int, off: int, c: int, al: int):
    if off < 0 or cs % al or off % al or off + c > cs:
        raise ValueError(f"{name}: stride {cs} / offset {off} must be multiples of {al} and channels {off} .. {off + c} inside the tensor")


def sppf_pools(x_nhwc: np.ndarray, c: int, x_off: int = 0, y: Optional[np.ndarray] = None, y_off: int = 0, half: bool = False,
               device: int = 0) -> np.ndarray:
    """SPPF's three chained MaxPool2d(5, 1, 2) on channel views: pools channels x_off .. x_off+c of x [N,H,W,Cx] and writes
    x1|x2|x3 into channels y_off .. y_off+3c of a copy of ``y`` [N,H,W,Cy] (default: SENTINEL-filled [N,H,W,3c]); the other
    channels of y come back unchanged.  ``half``: x and y are rounded to fp16 on the host and the fp16 kernels run (c, strides and
    offsets are then multiples of 8 instead of 4: 16-byte vectors); values are returned as fp32 either way."""
    x = _f32(x_nhwc)
    if x.ndim != 4:
        raise ValueError("x must be [N, H, W, Cx]")
    n, h, wd, cx = x.shape
    al = 8 if half else 4
    if c <= 0 or c % al:
        raise ValueError(f"c must be a positive multiple of {al}")
    out = _sentinel((n, h, wd, 3 * c)) if y is None else np.array(y, dtype=np.float32, order="C", copy=True)
    if out.shape[:3] != (n, h, wd):
        raise ValueError("y must be [N, H, W, Cy] with x's N, H, W")
    _check_view("x", cx, x_off, c, al)
    _check_view("y", out.shape[3], y_off, 3 * c, al)
    if half:
        x, out = x.astype(np.float16), out.astype(np.float16)
    _lib.check(_lib.lib().mi355_op_sppf_pools(device, x.ctypes.data, n, h, wd, cx, x_off, c, out.ctypes.data, out.shape[3], y_off,
                                              int(half)))
    return out.astype(np.float32) if half else out


def upsample2x(x_nhwc: np.ndarray, c: int, x_off: int = 0, y: Optional[np.ndarray] = None, y_off: int = 0, device: int = 0) -> np.ndarray:
    """Nearest 2x upsample of 32-bit words on channel views (the engine also moves fp16 pairs with it, so any bit pattern must
    survive): x [N,H,W,Cx] uint32 (or fp32, taken as its bits) channels x_off .. x_off+c -> channels y_off .. y_off+c of a copy of
    ``y`` [N,2H,2W,Cy] (default: SENTINEL_BITS-filled [N,2H,2W,c]); returned as uint32, the other channels of y unchanged."""
    def words(a):
        a = np.asarray(a)
        if a.dtype not in (np.dtype(np.uint32), np.dtype(np.float32)):
            raise ValueError("32-bit words: uint32 or float32 arrays")
        return np.ascontiguousarray(a).view(np.uint32)
    x = words(x_nhwc)
    if x.ndim != 4:
        raise ValueError("x must be [N, H, W, Cx]")
    n, h, wd, cx = x.shape
    if c <= 0:
        raise ValueError("c must be positive")
    out = np.full((n, 2 * h, 2 * wd, c), SENTINEL_BITS, np.uint32) if y is None else words(y).copy()
    if out.shape[:3] != (n, 2 * h, 2 * wd):
        raise ValueError("y must be [N, 2H, 2W, Cy]")
    _check_view("x", cx, x_off, c, 4)
    _check_view("y", out.shape[3], y_off, c, 4)
    _lib.check(_lib.lib().mi355_op_upsample2x(device, x.ctypes.data, n, h, wd, cx, x_off, c, out.ctypes.data, out.shape[3], y_off))
    return out


def psa_attention(qkv: np.ndarray, heads: int, key_dim: int = 32, head_dim: int = 64, device: int = 0) -> np.ndarray:
    """PSA attention (YOLO11 Attention between qkv and pe): qkv [N, HW, heads*(2*key_dim+head_dim)] laid out
    [q of every head | k of every head | v of every head] -> [N, HW, heads*head_dim]."""
    x = _f32(qkv)
    n, hw, cin = x.shape
    if cin != heads * (2 * key_dim + head_dim):
        raise ValueError("qkv channel count does not match heads / key_dim / head_dim")
    y = np.empty((n, hw, heads * head_dim), np.float32)
    _lib.check(_lib.lib().mi355_op_psa_attention(device, x.ctypes.data, n, hw, heads, key_dim, head_dim, y.ctypes.data))
    return y


def conv2d_fused(x_nhwc: np.ndarray, w1: np.ndarray, b1: np.ndarray, w2: np.ndarray, b2: np.ndarray, stride: int = 1, silu2: bool = False,
                 device: int = 0, plan: int = 0, return_n_plans: bool = False, half: bool = False, out_f32: bool = False):
    """Conv3x3 + bias + SiLU -> Conv1x1 + bias (+SiLU) as one fused launch: x [N,H,W,Cin] -> [N,H/s,W/s,C2].
    ``half``: the half=True kernels (see conv2d); ``out_f32``: the pointwise stage writes fp32 (head finals)."""
    x, w1, b1, w2, b2 = _f32(x_nhwc), _f32(w1), _f32(b1), _f32(w2), _f32(b2)
    n, h, wd, cin = x.shape
    c1, c2 = w1.shape[0], w2.shape[0]
    if w1.shape != (c1, cin, 3, 3) or w2.shape != (c2, c1, 1, 1) or b1.shape != (c1,) or b2.shape != (c2,):
        raise ValueError("shape mismatch")
    y = np.empty((n, h // stride, wd // stride, c2), dtype=np.float32)
    npl = C.c_int(0)
    if half:
        _lib.check(_lib.lib().mi355_op_conv2d_fused_f16(device, x.ctypes.data, n, h, wd, cin, w1.ctypes.data, b1.ctypes.data, c1, stride,
                                                        w2.ctypes.data, b2.ctypes.data, c2, int(silu2), y.ctypes.data, int(out_f32),
                                                        int(plan), C.byref(npl)))
        return (y, npl.value) if return_n_plans else y
    _lib.check(_lib.lib().mi355_op_conv2d_fused(device, x.ctypes.data, n, h, wd, cin, w1.ctypes.data, b1.ctypes.data, c1, stride,
                                                w2.ctypes.data, b2.ctypes.data, c2, int(silu2), y.ctypes.data, int(plan), C.byref(npl)))
    return (y, npl.value) if return_n_plans else y


def stem(bgr_u8: np.ndarray, w_oihw: np.ndarray, bias: np.ndarray, stride: int = 2, device: int = 0, half: bool = False,
         variant: int = 0) -> np.ndarray:
    """uint8 BGR frames [N,H,W,3] -> /255, RGB -> conv kxk + bias + SiLU -> [N,H/s,W/s,Cout].
    half=True: the half predictor's arithmetic (input, weights and output rounded to fp16, fp32 accumulation), float16 result;
    variant 0 = the kernel the engine launches, 1 = the general kernel, 2 = the k 3 / stride 2 kernel."""
    img = np.ascontiguousarray(bgr_u8, dtype=np.uint8)
    w, b = _f32(w_oihw), _f32(bias)
    n, h, wd, _ = img.shape
    cout, _, k, _ = w.shape
    if half:
        yh = np.empty((n, h // stride, wd // stride, cout), dtype=np.float16)
        _lib.check(_lib.lib().mi355_op_stem_f16(device, img.ctypes.data, n, h, wd, w.ctypes.data, b.ctypes.data, cout, k,
                                                stride, int(variant), yh.ctypes.data))
        return yh
    y = np.empty((n, h // stride, wd // stride, cout), dtype=np.float32)
    _lib.check(_lib.lib().mi355_op_stem(device, img.ctypes.data, n, h, wd, w.ctypes.data, b.ctypes.data, cout, k,
                                        stride, y.ctypes.data))
    return y


def letterbox_shape(h: int, w: int, imgsz: int = 640):
    oh, ow = C.c_int(), C.c_int()
    _lib.check(_lib.lib().mi355_letterbox_shape(h, w, imgsz, C.byref(oh), C.byref(ow)))
    return oh.value, ow.value


def letterbox(bgr_u8: np.ndarray, imgsz: int = 640, device: int = 0) -> np.ndarray:
    img = np.ascontiguousarray(bgr_u8, dtype=np.uint8)
    if img.ndim == 3:
        img = img[None]
    n, h, w, _ = img.shape
    oh, ow = letterbox_shape(h, w, imgsz)
    out = np.empty((n, oh, ow, 3), dtype=np.uint8)
    _lib.check(_lib.lib().mi355_op_letterbox(device, img.ctypes.data, n, h, w, imgsz, out.ctypes.data))
    return out


def letterbox_multi(frames: Sequence[np.ndarray], imgsz: int = 640, device: int = 0) -> np.ndarray:
    """Frames of any (h, w) (row strides honoured) -> the square [n, imgsz, imgsz, 3] canvas of a mixed batch (LetterBox auto=False)."""
    ptrs, hs, ws, rs, _, n = Ragged(frames, False).args()
    out = np.empty((n, imgsz, imgsz, 3), dtype=np.uint8)
    _lib.check(_lib.lib().mi355_op_letterbox_multi(device, ptrs, hs, ws, rs, n, imgsz, out.ctypes.data))
    return out


def yuv_to_bgr(frames, device: int = 0, out: Optional[Sequence[np.ndarray]] = None):
    """NV12 / I420 frames (``cvsd_amd.YUVFrame``, any sizes and row strides, formats may be mixed) -> a list of BGR arrays [H, W, 3]: the
    conversion the engine runs at ingest, alone.  ``device=-1`` runs the kernel's host twin and touches no GPU.  ``out``: C-contiguous
    uint8 arrays [H, W, 3] to write into (a test passes views of guarded buffers).  Planes on the GPU are brought to the host first:
    the hook takes host memory."""
    from .yuv import as_frames, struct_array
    fr = as_frames(frames)
    if fr is None:
        raise ValueError("frames: pass a YUVFrame or a list of them")
    fr = [f.host() for f in fr]
    if out is None:
        out = [np.empty((max(f.shape[0], 0), max(f.shape[1], 0), 3), np.uint8) for f in fr]
    out = list(out)
    if len(out) != len(fr):
        raise ValueError("out: one array per frame")
    for f, o in zip(fr, out):
        if not isinstance(o, np.ndarray) or o.dtype != np.uint8 or o.shape != (f.shape[0], f.shape[1], 3) or not o.flags.c_contiguous:
            raise ValueError("out: C-contiguous uint8 arrays of shape [H, W, 3]")
    ptrs = (C.c_void_p * len(out))(*[o.ctypes.data or 1 for o in out])     # (an empty array has no address; the frame is refused before any write)
    _lib.check(_lib.lib().mi355_op_yuv_to_bgr(int(device), struct_array(fr), len(fr), ptrs))
    return out


def motion_grid(frames, block: int = 16, device: int = 0):
    """The block-luma sums of a motion gate alone (csrc/motion_kernels.hip): ``frames`` -- BGR arrays [H, W, 3] of any row pitch or
    ``cvsd_amd.YUVFrame``s (their Y plane), up to 64, any sizes -> a list of uint32 [ceil(H / block), ceil(W / block)] grids.  One launch
    for all frames; ``device=-1`` runs the same routine on the host and touches no GPU.  Frames on a GPU are brought to the host first:
    the hook takes host memory and uploads it with the caller's pitch and base alignment."""
    import torch
    from .motion import _descriptor
    from .yuv import YUVFrame
    if isinstance(frames, (np.ndarray, YUVFrame, torch.Tensor)):
        frames = [frames]
    keep, descs = [], []
    for f in frames:
        f = f.host() if isinstance(f, YUVFrame) else (f.cpu() if isinstance(f, torch.Tensor) else f)
        descs.append(_descriptor(f, keep)[0])
    b = int(block)
    out = [np.zeros((-(-d.height // b), -(-d.width // b)) if b > 0 else (0, 0), np.uint32) for d in descs]
    ptrs = (C.c_void_p * len(out))(*[o.ctypes.data or 1 for o in out])
    _lib.check(_lib.lib().mi355_op_motion_grid(int(device), (_lib.MotionFrame * len(descs))(*descs), len(descs), b, ptrs))
    return out


def _frame_descriptors(frames, device: int, handle):
    """The ``mi355_render_frame`` records of a render or JPEG call -> (records, what they point into, ``frames`` or None): a list of
    arrays, CUDA tensors, ``YUVFrame`` and ``DeviceFrame``; or None with a handle -- the frames of the handle's last call."""
    from .yuv import YUVFrame
    lib = _lib.lib()
    keep, fd = [], []
    if frames is None:
        if handle is None:
            raise ValueError("frames=None needs an engine handle")
        cnt = C.c_int()
        _lib.check(lib.mi355_yolo_last_frames(handle, None, 0, C.byref(cnt)))
        last = (_lib.RenderFrame * max(cnt.value, 1))()
        _lib.check(lib.mi355_yolo_last_frames(handle, last, cnt.value, C.byref(cnt)))
        fd = [last[i] for i in range(cnt.value)]
        if not fd or any(not f.data for f in fd):
            raise LookupError("a frame of the handle's last call is no longer on the GPU")
        frames = None
    else:
        frames = list(frames)
        if not frames:
            raise ValueError("empty list of frames")
        for f in frames:
            if isinstance(f, YUVFrame):
                f = yuv_to_bgr([f], device=-1)[0] if device < 0 else f.to_bgr(device)
            v = bgr_view(f, empty_ok=True)
            if isinstance(f, DeviceFrame):
                if device < 0:
                    raise ValueError("a frame on a GPU cannot be rendered by the host twin")
                fd.append(_lib.RenderFrame(v.ptr, *v.hw, v.pitch, 1))      # a raw pointer: passed on as it was given
                continue
            if v.on_device:
                if device < 0 or v.keep.device.index != device:
                    raise ValueError("a CUDA frame must live on the GPU the call runs on")
                wait_for_torch(v.keep.device)
            keep.append(v.keep)
            # an empty array has no address and may report any pitch: the entries take a non-null pointer and a pitch of at least one
            # row, and refuse the frame by its size
            fd.append(_lib.RenderFrame(v.ptr or 1, *v.hw, int(max(v.pitch, 3 * v.hw[1])), int(v.on_device)))
    return fd, keep, frames


def _call_on_frames(handle, device: int, by_handle, by_device, fd, frames, args, timing: Optional[list]) -> None:
    """One render / encode call over the records ``fd``: with an engine ``handle`` on its stream with its scratch (``frames`` None:
    the frames of the handle's last call), else on ``device`` with the call's own; ``timing`` receives the launches' ms."""
    n = len(fd)
    ms = C.c_float(0.0)
    msp = C.byref(ms) if timing is not None else None
    if handle is not None:
        _lib.check(by_handle(handle, None if frames is None else (_lib.RenderFrame * n)(*fd), n, *args, msp))
    else:
        _lib.check(by_device(device, (_lib.RenderFrame * n)(*fd), n, *args, None, msp))
    if timing is not None:
        timing.append(float(ms.value))


def render(frames, prims, device: int = 0, out: str = "numpy", timing: Optional[list] = None, handle=None):
    """Draw primitive lists into COPIES of frames (csrc/render_kernels.hip): ``frames`` -- a BGR array [H, W, 3] (any row
    pitch), a uint8 CUDA tensor [H, W, 3] on ``device`` (any row pitch, read in place and left unchanged), a ``cvsd_amd.YUVFrame``
    (rendered from the BGR the ingest conversion makes of it), or a list of them of any sizes; ``prims`` -- int32 [P, 8] records
    (``cvsd_amd.render.primitives`` builds them), one array per frame.  One call, two launches, whatever the number of frames.
    ``out="numpy"``: uint8 arrays; ``"cuda"``: tensors on ``device``, nothing comes back to the host.  A single frame gives a single
    picture, a list a list.  ``device=-1`` runs the host twin and touches no GPU.  ``timing``: a list that receives the launches' ms.
    ``handle``: an engine handle -- the call runs on its stream with its scratch (``mi355_yolo_render``), and ``frames=None`` then means
    the frames of that handle's last call, read from where the call left them on the GPU."""
    import torch
    if out not in ("numpy", "cuda"):
        raise ValueError(f"out must be 'numpy' or 'cuda', got {out!r}")
    device = int(device)
    if out == "cuda" and device < 0:
        raise ValueError("out='cuda' needs a GPU: the host twin (device=-1) returns numpy arrays")
    lib = _lib.lib()
    frames, single = one_or_many(frames)
    prims = [prims] if single else list(prims)
    fd, keep, frames = _frame_descriptors(frames, device, handle)
    if len(fd) != len(prims):
        raise ValueError("prims: one int32 [P, 8] array per frame")
    od, outs, pp = [], [], []
    for f in fd:
        h, w = max(f.height, 0), max(f.width, 0)
        if out == "cuda":
            o = torch.empty((h, w, 3), dtype=torch.uint8, device=torch.device("cuda", device))
            od.append(_lib.RenderOut(o.data_ptr() or 1, 3 * w, 1))
        else:
            o = np.empty((h, w, 3), np.uint8)
            od.append(_lib.RenderOut(o.ctypes.data or 1, 3 * w, 0))
        outs.append(o)
    for p in prims:
        p = np.ascontiguousarray(np.zeros((0, _lib.RENDER_WORDS), np.int32) if p is None else p)
        if p.dtype != np.int32 or p.ndim != 2 or p.shape[1] != _lib.RENDER_WORDS:
            raise ValueError(f"prims must be int32 arrays of shape [P, {_lib.RENDER_WORDS}]")
        pp.append(p)
    n = len(fd)
    ptrs = (C.c_void_p * n)(*[p.ctypes.data if len(p) else None for p in pp])
    counts = (C.c_int * n)(*[len(p) for p in pp])
    _call_on_frames(handle, device, lib.mi355_yolo_render, lib.mi355_render, fd, frames, (ptrs, counts, (_lib.RenderOut * n)(*od)), timing)
    return outs[0] if single else outs


def crop_resize(frames, rects, size=None, fit: str = "stretch", fill: int = 114, device: int = 0, out: str = "numpy", handle=None,
                timing: Optional[list] = None):
    """Cut rectangles out of frames and copy or resample them (csrc/crop_kernels.hip).  ``frames``: what :func:`render`
    takes -- arrays of any pitch, uint8 CUDA tensors on ``device`` read in place, ``cvsd_amd.YUVFrame``, :class:`DeviceFrame`, or a list
    of them of any sizes; ``rects``: int32 [M, 4] (x1, y1, x2, y2) per frame (``cvsd_amd.crops.crop_rects`` makes them of boxes), M may
    be 0 and x2 <= x1 or y2 <= y1 is an empty rectangle.  ``size=None``: crop k is the copy ``frame[y1:y2, x1:x2]``; ``size=(h, w)``:
    ``fit="stretch"`` is ``cv2.resize(crop, (w, h), INTER_LINEAR)`` bit for bit, ``"pad"`` LetterBox(auto=False) with ``fill``; an empty
    rectangle is all ``fill``.  One call, ONE launch, whatever the number of frames and rectangles.  Returns, per frame, a list of uint8
    arrays (``out="numpy"``) or CUDA tensors (``"cuda"``); with a fixed size and ``"cuda"`` one tensor [M, h, w, 3] per frame, all views
    of a single allocation -- nothing comes back to the host.  A single frame gives a single such value.  ``device=-1`` runs the host
    twin and touches no GPU.  ``handle``: an engine handle -- the call runs on its stream with its scratch (``mi355_yolo_crops``), and
    ``frames=None`` then means the frames of that handle's last call.  ``timing``: a list that receives the launch's ms."""
    import torch
    if out not in ("numpy", "cuda"):
        raise ValueError(f"out must be 'numpy' or 'cuda', got {out!r}")
    if fit not in _lib.CROP_FIT:
        raise ValueError(f"fit must be 'stretch' or 'pad', got {fit!r}")
    device = int(device)
    if out == "cuda" and device < 0:
        raise ValueError("out='cuda' needs a GPU: the host twin (device=-1) returns numpy arrays")
    lib = _lib.lib()
    frames, single = one_or_many(frames)
    rects = [rects] if single else list(rects)
    fd, keep, frames = _frame_descriptors(frames, device, handle)
    if len(fd) != len(rects):
        raise ValueError("rects: one int32 [M, 4] array per frame")
    rr = []
    for r in rects:
        r = np.ascontiguousarray(np.zeros((0, 4), np.int32) if r is None else r)
        if r.dtype != np.int32 or r.ndim != 2 or r.shape[1] != 4:
            raise ValueError("rects must be int32 arrays of shape [M, 4]")
        rr.append(r)
    if size is not None and (int(size[0]), int(size[1])) == (0, 0):
        raise ValueError("size must be None (native) or (h, w) of positive integers, got (0, 0)")
    if size is None:
        spec = _lib.CropSpec(C.sizeof(_lib.CropSpec), 0, 0, _lib.CROP_FIT[fit], int(fill))
    else:
        spec = _lib.CropSpec(C.sizeof(_lib.CropSpec), int(size[0]), int(size[1]), _lib.CROP_FIT[fit], int(fill))
    cuda = out == "cuda"
    dev = torch.device("cuda", device) if cuda else None
    res, od = [], []

    def record(o):
        if cuda:
            return _lib.RenderOut(o.data_ptr() or 1, 3 * o.shape[1], 1)
        return _lib.RenderOut(o.ctypes.data or 1, 3 * o.shape[1], 0)

    if size is None:
        for r in rr:
            per = []
            for x1, y1, x2, y2 in r.tolist():
                h, w = (y2 - y1, x2 - x1) if x2 > x1 and y2 > y1 else (0, 0)
                o = torch.empty((h, w, 3), dtype=torch.uint8, device=dev) if cuda else np.empty((h, w, 3), np.uint8)
                per.append(o)
                od.append(record(o))
            res.append(per)
    else:
        h, w = max(int(size[0]), 0), max(int(size[1]), 0)
        total = sum(len(r) for r in rr)
        block = torch.empty((total, h, w, 3), dtype=torch.uint8, device=dev) if cuda else np.empty((total, h, w, 3), np.uint8)
        at = 0
        for r in rr:
            part = block[at:at + len(r)]
            at += len(r)
            od.extend(record(part[k]) for k in range(len(r)))
            res.append(part if cuda else list(part))
    n = len(fd)
    ptrs = (C.c_void_p * n)(*[r.ctypes.data if len(r) else None for r in rr])
    counts = (C.c_int * n)(*[len(r) for r in rr])
    outs = (_lib.RenderOut * max(len(od), 1))(*od)
    _call_on_frames(handle, device, lib.mi355_yolo_crops, lib.mi355_crops, fd, frames, (ptrs, counts, C.byref(spec), outs), timing)
    return res[0] if single else res


def _jpeg_args(quality, subsampling):
    ss = {"420": _lib.JPEG_420, "444": _lib.JPEG_444, 420: _lib.JPEG_420, 444: _lib.JPEG_444}.get(subsampling)
    if ss is None:
        raise ValueError(f"subsampling must be '420' or '444', got {subsampling!r}")
    return int(quality), ss


def jpeg_encode(frames, quality: int = 85, subsampling: str = "420", device: int = 0, handle=None, timing: Optional[list] = None):
    """Encode BGR frames as baseline JFIF streams (csrc/jpeg_kernels.hip) -> ``bytes`` (a list of ``bytes`` for a list).
    ``frames``: what :func:`render` takes -- arrays of any pitch, uint8 CUDA tensors on ``device`` read in place, ``cvsd_amd.YUVFrame``
    (from the BGR the ingest conversion makes of it), :class:`DeviceFrame`, or a list of them of any sizes.  One call, three launches,
    whatever the number of frames; only the streams' bytes come back from the GPU.  ``quality`` 1 .. 100 (the IJG scaling of the Annex K
    tables), ``subsampling`` "420" or "444".  ``device=-1`` runs the host twin and touches no GPU.  ``handle``: an engine handle -- the
    call runs on its stream with its scratch (``mi355_yolo_encode``), and ``frames=None`` then means the frames of that handle's last
    call, read from where the call left them on the GPU.  ``timing``: a list that receives the launches' ms."""
    device = int(device)
    quality, ss = _jpeg_args(quality, subsampling)
    lib = _lib.lib()
    frames, single = one_or_many(frames)
    fd, keep, frames = _frame_descriptors(frames, device, handle)
    n = len(fd)
    bufs, od = [], []
    for f in fd:
        cap = int(lib.mi355_jpeg_bound(f.height, f.width, ss))
        b = np.empty(max(cap, 1), np.uint8)                 # the worst case of the frame's size; only the stream's pages are ever touched
        bufs.append(b)
        od.append(_lib.JpegOut(b.ctypes.data, cap, 0))
    outs = (_lib.JpegOut * n)(*od)
    _call_on_frames(handle, device, lib.mi355_yolo_encode, lib.mi355_jpeg_encode, fd, frames, (quality, ss, outs), timing)
    res = [bufs[i][:outs[i].length].tobytes() for i in range(n)]
    return res[0] if single else res


def jpeg_coefficients(frames, quality: int = 85, subsampling: str = "420", device: int = 0):
    """The transform stage of :func:`jpeg_encode` alone (``mi355_op_jpeg_coefficients``): per frame int16 [blocks, 64] -- quantised DCT
    coefficients in zigzag order, blocks in scan order (MCU rows, MCUs, then Y0 Y1 Y2 Y3 Cb Cr for "420", Y Cb Cr for "444").
    ``device=-1`` runs the host twin."""
    device = int(device)
    quality, ss = _jpeg_args(quality, subsampling)
    lib = _lib.lib()
    frames, single = one_or_many(frames)
    fd, keep, frames = _frame_descriptors(frames, device, None)
    m, per = (16, 6) if ss == _lib.JPEG_420 else (8, 3)
    outs = [np.zeros((max(-(-f.height // m) * -(-f.width // m) * per, 0), 64), np.int16) for f in fd]
    ptrs = (C.c_void_p * len(fd))(*[o.ctypes.data or 1 for o in outs])
    _lib.check(lib.mi355_op_jpeg_coefficients(device, (_lib.RenderFrame * len(fd))(*fd), len(fd), quality, ss, ptrs))
    return outs[0] if single else outs


def _jpeg_streams(streams):
    """-> (list of JPEGFrame, single?): bytes-like streams are parsed here, so a refused one raises ``ValueError`` naming its index"""
    from .jpeg_decode import JPEGFrame
    single = isinstance(streams, (JPEGFrame, bytes, bytearray, memoryview))
    fr = []
    for i, s in enumerate([streams] if single else list(streams)):
        if not isinstance(s, JPEGFrame):
            try:
                s = JPEGFrame(s)
            except ValueError as e:
                raise ValueError(f"streams[{i}]: {e}") from None
        fr.append(s)
    if not fr:
        raise ValueError("streams: pass a JPEGFrame (or its bytes) or a list of them")
    return fr, single


def jpeg_decode(streams, device: int = 0, entropy: str = "auto", out=None, as_tensor: bool = False, handle=None,
                timing: Optional[list] = None):
    """Decode baseline JPEG streams to BGR frames (csrc/jpeg_decode_kernels.hip) -> uint8 [H, W, 3] (a list for a list).
    ``streams``: ``cvsd_amd.JPEGFrame`` or bytes-like, or a list of them of any sizes and layouts (4:4:4, 4:2:2, 4:2:0, gray; with or
    without restart markers).  One call, three launches, whatever the number of streams; only the compressed bytes go up.
    ``entropy``: "gpu" -- one GPU lane per restart segment (a stream without restart markers is one segment on one lane: slow, correct);
    "host" -- Huffman decoding on the calling thread, coefficients uploaded; "auto" -- "gpu" for a stream with a restart interval,
    "host" for one without; "sync" -- many GPU lanes per restart segment, the self-synchronising parallel Huffman decoder of
    csrc/jpeg_sync.h, meant for streams without restart markers (opt-in: "auto" never chooses it; four more launches).  A
    ``JPEGFrame(data, entropy=...)`` carries its own request, which goes before the call's.  ``as_tensor=True``: CUDA tensors on ``device`` that never visit the host.  ``out``: arrays (or, on a GPU,
    CUDA tensors) [H, W, 3] uint8 to write into, last strides (3, 1), any row pitch.  ``device=-1`` runs the host twin and touches no
    GPU.  ``handle``: an engine handle -- the call runs on its stream with its scratch (``mi355_yolo_decode``).  ``timing``: a list that
    receives ``{"ms": the launches' device time, "entropy": ["gpu" | "host" | "sync" per stream]}``.  A stream whose entropy-coded data is
    corrupt raises ``ValueError`` naming its index; the other streams' frames (in ``out``) are complete."""
    import torch
    device = int(device)
    if entropy not in _lib.JPEG_ENTROPY:
        raise ValueError(f"entropy must be 'auto', 'gpu', 'host' or 'sync', got {entropy!r}")
    if as_tensor and device < 0:
        raise ValueError("as_tensor=True needs a GPU: the host twin (device=-1) returns numpy arrays")
    fr, single = _jpeg_streams(streams)
    n = len(fr)
    if out is None:
        outs = [torch.empty((f.shape[0], f.shape[1], 3), dtype=torch.uint8, device=f"cuda:{device}") if as_tensor
                else np.empty((f.shape[0], f.shape[1], 3), np.uint8) for f in fr]
    else:
        outs = [out] if single and not isinstance(out, (list, tuple)) else list(out)
        if len(outs) != n:
            raise ValueError("out: one array per stream")
    od = []
    for f, o in zip(fr, outs):
        on_dev = isinstance(o, torch.Tensor) and o.is_cuda
        if isinstance(o, torch.Tensor) and not on_dev:
            raise ValueError("out: numpy arrays or CUDA tensors")
        dt_ok = o.dtype == (torch.uint8 if on_dev else np.uint8)
        st = tuple(o.stride()) if on_dev else tuple(o.strides) if isinstance(o, np.ndarray) else None
        if st is None or not dt_ok or tuple(o.shape) != (f.shape[0], f.shape[1], 3) or st[2] != 1 or st[1] != 3 or (f.shape[0] > 1 and st[0] < 3 * f.shape[1]):
            raise ValueError(f"out: uint8 [H, W, 3] of the stream's size {f.shape} with pixel stride 3 and rows of at least 3 W bytes")
        if on_dev and (device < 0 or o.device.index != device):
            raise ValueError("out: a CUDA tensor must live on the call's GPU")
        if not on_dev and not o.flags.writeable:
            raise ValueError("out: a read-only array")
        od.append(_lib.RenderOut(o.data_ptr() if on_dev else o.ctypes.data, int(max(st[0], 3 * f.shape[1])), int(on_dev)))
    if any(d.on_device for d in od):
        wait_for_torch(device)                               # the call runs on its own stream
    sd = (_lib.JpegStream * n)(*[f.struct() for f in fr])
    status = (C.c_int * n)()
    ms = C.c_float(0.0)
    msp = C.byref(ms) if timing is not None else None
    lib = _lib.lib()
    if handle is not None:
        rc = lib.mi355_yolo_decode(handle, sd, n, _lib.JPEG_ENTROPY[entropy], (_lib.RenderOut * n)(*od), status, msp)
    else:
        rc = lib.mi355_jpeg_decode(device, sd, n, _lib.JPEG_ENTROPY[entropy], (_lib.RenderOut * n)(*od), status, None, msp)
    _lib.check(rc)
    if timing is not None:
        timing.append({"ms": float(ms.value), "entropy": [{1: "gpu", 3: "sync"}.get(s.entropy_used, "host") for s in sd]})
    return outs[0] if single else outs


def jpeg_decode_coefficients(streams, device: int = 0, entropy: str = "auto"):
    """The entropy stage of :func:`jpeg_decode` alone (``mi355_op_jpeg_decode_coefficients``): per stream int16 [blocks, 64] -- the
    quantised coefficients in zigzag order, blocks in scan order, DC absolute.  ``device=-1`` runs the host twin."""
    if entropy not in _lib.JPEG_ENTROPY:
        raise ValueError(f"entropy must be 'auto', 'gpu', 'host' or 'sync', got {entropy!r}")
    fr, single = _jpeg_streams(streams)
    n = len(fr)
    outs = [np.zeros((f.blocks, 64), np.int16) for f in fr]
    ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    sd = (_lib.JpegStream * n)(*[f.struct() for f in fr])
    _lib.check(_lib.lib().mi355_op_jpeg_decode_coefficients(int(device), sd, n, _lib.JPEG_ENTROPY[entropy], ptrs, (C.c_int * n)()))
    return outs[0] if single else outs


def jpeg_sync(stream, device: int = 0, sub_bytes: int = 128, seq_subs: int = 256):
    """``entropy="sync"`` on one stream with subsequences of ``sub_bytes`` bytes (a power of two >= 8) and sequences of ``seq_subs``
    subsequences (2 .. 256) -- the test hook ``mi355_op_jpeg_sync`` (csrc/jpeg_sync.h); ``device=-1`` runs the host twin.
    -> ``{"coefficients": int16 [blocks, 64], "status": 0 | 1 .. 4, "states": int64 [nsub, 6] -- per subsequence (segment, byte, bit, j,
    k, B) of its true entry state, "stats": {"nsub", "nseq", "rounds_local", "rounds_global"}}``."""
    fr, single = _jpeg_streams(stream)
    if not single:
        raise ValueError("jpeg_sync takes one stream")
    f = fr[0]
    lib = _lib.lib()
    sd = f.struct()
    stats = _lib.JpegSyncStats()
    _lib.check(lib.mi355_op_jpeg_sync(int(device), C.byref(sd), int(sub_bytes), int(seq_subs), None, None, None, 0, C.byref(stats)))
    nsub = int(stats.nsub)
    coef = np.zeros((f.blocks, 64), np.int16)
    states = (_lib.JpegSyncState * nsub)()
    status = C.c_int(0)
    _lib.check(lib.mi355_op_jpeg_sync(int(device), C.byref(sd), int(sub_bytes), int(seq_subs), coef.ctypes.data, C.byref(status), states, nsub,
                                      C.byref(stats)))
    rows = np.array([(s.segment, s.byte, s.bit, s.j, s.k, s.block) for s in states], np.int64).reshape(nsub, 6)
    return {"coefficients": coef, "status": int(status.value), "states": rows,
            "stats": {k: int(getattr(stats, k)) for k in ("nsub", "nseq", "rounds_local", "rounds_global")}}


def nms(pred: np.ndarray, nc: int, conf: float = 0.25, iou: float = 0.7, classes: Optional[Sequence[int]] = None,
        max_det: int = 300, device: int = 0):
    """non_max_suppression on pred [N, 4+nc+extra, A] -> list of (rows [n,6+extra], anchor_idx [n])."""
    p = _f32(pred)
    n, no, a = p.shape
    extra = no - 4 - nc
    rows = np.zeros((n, max_det, _lib.DET_WORDS), dtype=np.float32)
    counts = np.zeros(n, dtype=np.int32)
    cls_arr, ncls = None, 0
    if classes is not None:
        cls_arr = (C.c_int * len(classes))(*[int(c) for c in classes])
        ncls = len(classes)
    _lib.check(_lib.lib().mi355_op_nms(device, p.ctypes.data, n, nc, extra, a, conf, iou, cls_arr, ncls, max_det,
                                       rows.ctypes.data, max_det, counts.ctypes.data_as(C.POINTER(C.c_int))))
    out = []
    for i in range(n):
        r = rows[i, :counts[i]]
        ints = r[:, 5:7].view(np.int32)
        out.append((np.concatenate([r[:, :5], ints[:, :1].astype(np.float32), r[:, 7:7 + extra]], 1), ints[:, 1].copy()))
    return out


class PostprocessResult:
    """What :func:`postprocess` hands back: ``rows`` [n, max_det, 58] uint32 (every slot, SENTINEL_BITS where nothing was written),
    ``counts`` [n] int32 and, with ``pack``, ``packed`` [n * max_det, 58] uint32, ``offsets`` [n + 1] int32 and ``total``."""

    def __init__(self, rows, counts, packed=None, offsets=None):
        self.rows, self.counts, self.packed, self.offsets = rows, counts, packed, offsets
        self.total = None if offsets is None else int(offsets[-1])


def postprocess(pred: np.ndarray, nc: int, conf: float = 0.25, iou: float = 0.7, classes: Optional[Sequence[int]] = None,
                max_det: int = 300, max_nms: int = 30000, kdim: int = 0, geom=None, best: Optional[np.ndarray] = None,
                pack: bool = False, device: int = 0) -> PostprocessResult:
    """The detector's tail as a pass runs it: candidate filter, sort, greedy suppression, scale-back, rows and (``pack``) row
    compaction, on pred [n, 4+nc+extra, A].  ``best`` [n, A, 2] (score, class) is the caller's, or computed from pred.  ``kdim``
    0, 2 or 3 says how scale-back reads the extra columns.  ``geom``: None = rows stay in letterboxed pixels; 7 floats (gain,
    pad_x, pad_y, kpad_x, kpad_y, orig_w, orig_h) = one geometry for every frame (the kernel's scalars); [n, 7] = one per frame
    (the mixed-batch table).  Which launches run follows from n and A alone: A > 16384 the multi-launch sort, else n <= 16 the fused
    sort + greedy kernel, else the two-launch pair.  Rows, packed rows and offsets are filled with SENTINEL_BITS before the launch."""
    p = _f32(pred)
    if p.ndim != 3:
        raise ValueError("pred must be [n, 4+nc+extra, A]")
    n, no, a = p.shape
    extra = no - 4 - nc
    if n <= 0 or a <= 0 or nc <= 0 or extra < 0:
        raise ValueError("pred must be [n, 4+nc+extra, A] with n, A, nc positive")
    if not 1 <= max_det <= 1024:
        raise ValueError("max_det must lie in 1 .. 1024")
    if max_nms < 1:
        raise ValueError("max_nms must be at least 1")
    if extra > _lib.MAX_KPT_FLOATS:
        raise ValueError("too many extra columns")
    if kdim not in (0, 2, 3) or (kdim and (extra == 0 or extra % kdim)):
        raise ValueError("kdim must be 0, 2 or 3 and, with keypoints, divide the extra columns")
    if not conf >= 0:
        raise ValueError("conf must be >= 0 (the sort key orders positive scores only)")
    g, mode = None, 0
    if geom is not None:
        g = _f32(geom)
        if g.shape == (7,):
            mode = 1
        elif g.shape == (n, 7):
            mode = 2
        else:
            raise ValueError("geom must be 7 floats or [n, 7]")
    cls_arr, ncls = None, 0
    if classes is not None:
        if len(classes) == 0:
            raise ValueError("an empty class list keeps nothing: pass None for every class")
        cls_arr = (C.c_int * len(classes))(*[int(c) for c in classes])
        ncls = len(classes)
    b = None
    if best is not None:
        b = _f32(best)
        if b.shape != (n, a, 2):
            raise ValueError("best must be [n, A, 2]")
        if ncls and not ((b[..., 1] >= 0) & (b[..., 1] < nc)).all():
            raise ValueError("with a class list every class of best[] must lie in 0 .. nc-1")
    rows = np.full((n, max_det, _lib.DET_WORDS), SENTINEL_BITS, np.uint32)
    counts = np.full(n, -1, np.int32)
    packed = offsets = None
    if pack:
        packed = np.full((n * max_det, _lib.DET_WORDS), SENTINEL_BITS, np.uint32)
        offsets = np.full(n + 1, SENTINEL_BITS, np.uint32).view(np.int32)
    _lib.check(_lib.lib().mi355_op_nms_ex(device, p.ctypes.data, b.ctypes.data if b is not None else None, n, nc, extra, a, float(conf),
                                          float(iou), cls_arr, ncls, int(max_det), int(max_nms), int(kdim),
                                          g.ctypes.data if g is not None else None, mode, int(pack), rows.ctypes.data, counts.ctypes.data,
                                          packed.ctypes.data if pack else None, offsets.ctypes.data if pack else None))
    return PostprocessResult(rows, counts, packed, offsets)


def plan_versions(n: int, h: int, w: int, cin: int, cout: int, k: int, stride: int = 1, src_cs: int = 0, dst_cs: int = 0, res_cs: int = 0,
                  f2_cout: int = 0, f2_dst_cs: int = 0, half: bool = False):
    """Kernel versions of the candidate launch plans the planner offers for this conv (host-only query, runs without a GPU):
    1 LDS-staged implicit GEMM, 3 streaming pointwise, 4 pipelined pointwise, 6 split-K; + 100 = with the fused pointwise stage."""
    cap = 4096
    out = (C.c_int * cap)()
    npl = C.c_int(0)
    r4 = lambda c: (c + 3) // 4 * 4
    _lib.check(_lib.lib().mi355_plan_query(n, h, w, cin, cout, k, stride, src_cs or r4(cin), dst_cs or r4(cout), res_cs, f2_cout,
                                           f2_dst_cs or r4(f2_cout), int(half), out, cap, C.byref(npl)))
    return [out[i] for i in range(min(cap, npl.value))]


PLAN_TILE_FIELDS = ("version", "PT", "CT", "WP", "TW", "TH", "G", "grid_x", "grid_y")


def plan_tiles(n: int, h: int, w: int, cin: int, cout: int, k: int, stride: int = 1, src_cs: int = 0, dst_cs: int = 0, res_cs: int = 0,
               f2_cout: int = 0, f2_dst_cs: int = 0, half: bool = False):
    """The candidate launch plans of :func:`plan_versions`, in the same order, each as a dict of its launch geometry (host-only
    query): ``version``, ``PT`` / ``CT`` (pixel / cout tiles of 16 per wave), ``WP`` (waves along pixels), ``TW`` x ``TH`` (output
    tile), ``G`` (cout groups per wave), ``grid_x`` / ``grid_y``; and, worked out here for the LDS-staged kernels, ``P`` (pixels a
    block computes = WP * PT * 16) and ``tiles_x`` / ``tiles_y`` (tiles over the output map): tiles_x * tiles_y * P pixels are
    computed per image for the map's Wout * Hout."""
    cap, nf = 4096, len(PLAN_TILE_FIELDS)
    out = (C.c_int * (cap * nf))()
    npl = C.c_int(0)
    r4 = lambda c: (c + 3) // 4 * 4
    _lib.check(_lib.lib().mi355_plan_query_tiles(n, h, w, cin, cout, k, stride, src_cs or r4(cin), dst_cs or r4(cout), res_cs, f2_cout,
                                                 f2_dst_cs or r4(f2_cout), int(half), out, cap, C.byref(npl)))
    wo, ho = (n * h * w, 1) if k == 1 else (w // stride, h // stride)
    plans = []
    for i in range(min(cap, npl.value)):
        p = dict(zip(PLAN_TILE_FIELDS, out[i * nf:(i + 1) * nf]))
        p["P"] = p["WP"] * p["PT"] * 16
        p["tiles_x"], p["tiles_y"] = -(-wo // p["TW"]), -(-ho // p["TH"])
        plans.append(p)
    return plans


def memory_plan(blob: bytes, n: int, height: int, width: int, imgsz: int = 640, half: bool = False, reuse: bool = True):
    """Where the engine would place the activation buffers of weight image ``blob`` for ``n`` frames per pass (host-only query):
    -> (offsets [n_buffers], sizes [n_buffers], arena_bytes, unshared_bytes)."""
    cap = 4096
    off, sz = (C.c_longlong * cap)(), (C.c_longlong * cap)()
    nb, arena, plain = C.c_int(0), C.c_longlong(0), C.c_longlong(0)
    _lib.check(_lib.lib().mi355_memory_plan(blob, len(blob), n, height, width, imgsz, int(half), int(reuse), off, sz, cap, C.byref(nb),
                                            C.byref(arena), C.byref(plain)))
    k = nb.value
    return np.array(off[:k], dtype=np.int64), np.array(sz[:k], dtype=np.int64), arena.value, plain.value


def memory_plan_ex(blob: bytes, n: int, height: int, width: int, imgsz: int = 640, half: bool = False, reuse: bool = True,
                   obj_feats: bool = False):
    """:func:`memory_plan` for an engine with ``mi355_opts.obj_feats``: -> (offsets, sizes, arena_bytes, unshared_bytes, detect_bufs),
    ``detect_bufs`` = the program buffers that hold the Detect head's input maps, one per level (what the option keeps alive)."""
    cap = 4096
    off, sz = (C.c_longlong * cap)(), (C.c_longlong * cap)()
    nb, arena, plain = C.c_int(0), C.c_longlong(0), C.c_longlong(0)
    det = (C.c_int * 4)(-1, -1, -1, -1)
    _lib.check(_lib.lib().mi355_memory_plan_ex(blob, len(blob), n, height, width, imgsz, int(half), int(reuse), int(obj_feats), off, sz, cap,
                                               C.byref(nb), C.byref(arena), C.byref(plain), det))
    k = nb.value
    return np.array(off[:k], dtype=np.int64), np.array(sz[:k], dtype=np.int64), arena.value, plain.value, [d for d in det if d >= 0]


def conv2d_group(x_nhwc: np.ndarray, wa: np.ndarray, ba: np.ndarray, wb: np.ndarray, bb: np.ndarray, stride_a: int = 1, stride_b: int = 1,
                 plan_a: int = 0, plan_b: int = 0, device: int = 0, w2a: Optional[np.ndarray] = None, b2a: Optional[np.ndarray] = None):
    """Two independent convs of one input as ONE grouped launch (conv_f32_group.hip): -> (ya, yb, n_menu_a, n_menu_b).
    ``w2a`` / ``b2a``: a pointwise conv fused behind conv a (3x3), as in :func:`conv2d_fused`; ya is then its output."""
    x, wa, ba, wb, bb = _f32(x_nhwc), _f32(wa), _f32(ba), _f32(wb), _f32(bb)
    n, h, wd, cin = x.shape
    c2 = 0
    if w2a is not None:
        w2a, b2a = _f32(w2a), _f32(b2a)
        c2 = w2a.shape[0]
    ya = np.empty((n, h // stride_a, wd // stride_a, c2 or wa.shape[0]), dtype=np.float32)
    yb = np.empty((n, h // stride_b, wd // stride_b, wb.shape[0]), dtype=np.float32)
    na, nb = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().mi355_op_conv2d_group(device, x.ctypes.data, n, h, wd, cin, wa.ctypes.data, ba.ctypes.data, wa.shape[0], wa.shape[2],
                                                stride_a, wb.ctypes.data, bb.ctypes.data, wb.shape[0], wb.shape[2], stride_b, ya.ctypes.data,
                                                yb.ctypes.data, int(plan_a), int(plan_b), C.byref(na), C.byref(nb),
                                                w2a.ctypes.data if c2 else None, b2a.ctypes.data if c2 else None, c2))
    return ya, yb, na.value, nb.value


def c2f_tail(x_nhwc: np.ndarray, w1: np.ndarray, b1: np.ndarray, lead: np.ndarray, w2: np.ndarray, b2: np.ndarray,
             residual: Optional[np.ndarray] = None, device: int = 0, plan: int = 0, return_n_plans: bool = False):
    """The tail of a C2f block as one fused launch: SiLU(conv1x1(cat(lead, SiLU(conv3x3(x) + b1) + residual)) + b2).
    x [N,H,W,Cin], lead [N,H,W,L] (L and the 3x3's cout multiples of 16), w2 [C2, L + C1, 1, 1]."""
    x, w1, b1, lead, w2, b2 = _f32(x_nhwc), _f32(w1), _f32(b1), _f32(lead), _f32(w2), _f32(b2)
    n, h, wd, cin = x.shape
    c1, c2, L = w1.shape[0], w2.shape[0], lead.shape[-1]
    if w1.shape != (c1, cin, 3, 3) or w2.shape != (c2, L + c1, 1, 1) or lead.shape[:3] != (n, h, wd):
        raise ValueError("shape mismatch")
    r = None
    if residual is not None:
        r = _f32(residual)
        if r.shape != (n, h, wd, c1):
            raise ValueError("residual must have the 3x3 conv's output shape")
    y = np.empty((n, h, wd, c2), dtype=np.float32)
    npl = C.c_int(0)
    _lib.check(_lib.lib().mi355_op_c2f_tail(device, x.ctypes.data, n, h, wd, cin, w1.ctypes.data, b1.ctypes.data, c1,
                                            r.ctypes.data if r is not None else None, lead.ctypes.data, L, w2.ctypes.data, b2.ctypes.data, c2,
                                            y.ctypes.data, int(plan), C.byref(npl)))
    return (y, npl.value) if return_n_plans else y
