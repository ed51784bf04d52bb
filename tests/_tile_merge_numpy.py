"""Sequential statement of tiled predict's geometry and merge (include/mi355_yolo.h), in float32 numpy scalars, one
operation per line: the tile grid rule, the shift of a row into frame coordinates, the stable order and the greedy pass with both
metrics.  The CPU suite checks the host twin against it, the GPU suite the kernel and the whole tiled call."""
import numpy as np

F32 = np.float32
DET_WORDS = 58
MAX_KPT_FLOATS = 51


def axis_positions(L, t, o):
    """positions of the tiles along an axis of length L, tile t, overlap o pixels (0 <= o < t)"""
    pos = []
    p = 0
    while p + t < L:
        pos.append(p)
        p = p + t - o
    pos.append(max(0, L - t))
    return pos


def tile_grid(height, width, tile_h, tile_w, overlap_y_px, overlap_x_px):
    """-> int32 [T, 4] rows x, y, w, h, row-major (y outer, x inner); every tile's extent on an axis is min(t, L)"""
    ys = axis_positions(height, tile_h, overlap_y_px)
    xs = axis_positions(width, tile_w, overlap_x_px)
    eh, ew = min(tile_h, height), min(tile_w, width)
    return np.array([[x, y, ew, eh] for y in ys for x in xs], np.int32).reshape(-1, 4)


def entries(height, width, tile, overlap, full_frame=True):
    """the entry list of one frame as predict(tile=, overlap=) builds it: overlap -> pixels as int(overlap * tile) per axis"""
    th, tw = (tile, tile) if isinstance(tile, int) else tile
    g = tile_grid(height, width, th, tw, int(overlap * th), int(overlap * tw))
    if full_frame:
        g = np.concatenate([g, np.array([[0, 0, width, height]], np.int32)])
    return g


def _overlap_gt(a, b, metric, thr):
    """a = float32 [K, 5] rows x1, y1, x2, y2, area of the earlier kept rows, b = the candidate's five float32 scalars -> bool [K];
    every line is ONE float32 operation per element"""
    xx1 = np.where(a[:, 0] > b[0], a[:, 0], b[0])
    yy1 = np.where(a[:, 1] > b[1], a[:, 1], b[1])
    xx2 = np.where(a[:, 2] < b[2], a[:, 2], b[2])
    yy2 = np.where(a[:, 3] < b[3], a[:, 3], b[3])
    dw = xx2 - xx1
    dh = yy2 - yy1
    w = np.where(dw > F32(0), dw, F32(0))
    h = np.where(dh > F32(0), dh, F32(0))
    inter = w * h
    if metric == "ios":
        den = np.where(a[:, 4] < b[4], a[:, 4], b[4])
    else:
        s = a[:, 4] + b[4]
        den = s - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        m = inter / den
    assert m.dtype == np.float32
    return m > F32(thr)                 # NaN compares false


def merge_frame(rows, counts, origins, kdim, metric, thr, nk=None):
    """rows float32 [E, max_det, 58] (words; cls / anchor_idx are int32 bits), counts [E], origins [E, 2] = ox, oy of every entry ->
    (merged rows [M, 58], tile_idx int32 [M]) in kept order.  nk = keypoint floats of a row (default: every whole group of kdim)."""
    rows = np.ascontiguousarray(rows, np.float32)
    E, max_det = rows.shape[:2]
    if nk is None:
        nk = (MAX_KPT_FLOATS // kdim) * kdim if kdim else 0
    bits = rows.view(np.uint32)
    cand = []
    for e in range(E):
        for r in range(int(counts[e])):
            slot = e * max_det + r
            key = (((~int(bits[e, r, 4])) & 0xFFFFFFFF) << 32) | slot
            cand.append((key, e, r))
    cand.sort()                                        # keys are unique: descending conf, ties by ascending slot
    kept = np.zeros((max_det, 5), np.float32)          # x1, y1, x2, y2, area of the kept rows
    kcls = np.zeros(max_det, np.int64)
    out, idx = [], []
    for _, e, r in cand:
        if len(out) >= max_det:
            break
        ox = F32(int(origins[e][0]))
        oy = F32(int(origins[e][1]))
        x1 = F32(rows[e, r, 0] + ox)
        y1 = F32(rows[e, r, 1] + oy)
        x2 = F32(rows[e, r, 2] + ox)
        y2 = F32(rows[e, r, 3] + oy)
        bw = F32(x2 - x1)
        bh = F32(y2 - y1)
        area = F32(bw * bh)
        cls = int(bits[e, r, 5])
        me = np.array([x1, y1, x2, y2, area], np.float32)
        k = len(out)
        if np.any((kcls[:k] == cls) & _overlap_gt(kept[:k], me, metric, thr)):
            continue
        kept[k] = me
        kcls[k] = cls
        row = rows[e, r].copy()
        row[0], row[1], row[2], row[3] = x1, y1, x2, y2
        if kdim >= 2:
            for j in range(nk):
                if j % kdim == 0:
                    row[7 + j] = F32(row[7 + j] + ox)
                elif j % kdim == 1:
                    row[7 + j] = F32(row[7 + j] + oy)
        out.append(row)
        idx.append(e)
    return np.array(out, np.float32).reshape(-1, DET_WORDS), np.array(idx, np.int32)


def merge(rows, counts, origins, kdim=0, metric="ios", thr=0.5, nk=None):
    """rows [F, E, max_det, 58], counts [F, E], origins [F, E, 2] -> list of (merged rows, tile_idx) per frame"""
    return [merge_frame(rows[f], counts[f], origins[f], kdim, metric, thr, nk) for f in range(len(rows))]


def det_row(x1, y1, x2, y2, conf, cls=0, anchor=0, kpt=None):
    """one mi355_det row as 58 float32 words"""
    r = np.zeros(DET_WORDS, np.float32)
    r[:5] = (x1, y1, x2, y2, conf)
    r[5:7].view(np.int32)[:] = (cls, anchor)
    if kpt is not None:
        k = np.asarray(kpt, np.float32).reshape(-1)
        r[7:7 + len(k)] = k
    return r


def random_rows(rng, F, E, max_det, counts, extent=200.0, n_cls=2, kpt=True, ties=True, size_frac=0.3):
    """seeded row sets shaped like a detector's: boxes inside [0, extent) with sides up to size_frac * extent (larger: more of them
    suppress each other), conf descending per entry with repeated values (ties across and inside entries), a few classes, keypoint
    floats; rows at or beyond counts carry garbage that must not be read"""
    rows = rng.uniform(-5, 5, (F, E, max_det, DET_WORDS)).astype(np.float32)
    confs = np.round(rng.uniform(0.1, 0.95, 64), 2).astype(np.float32) if ties else None
    for f in range(F):
        for e in range(E):
            c = int(counts[f][e])
            xy = rng.uniform(0, extent * 0.8, (c, 2)).astype(np.float32)
            wh = rng.uniform(4, extent * size_frac, (c, 2)).astype(np.float32)
            rows[f, e, :c, 0:2] = xy
            rows[f, e, :c, 2:4] = xy + wh
            cf = rng.choice(confs, c) if ties else rng.uniform(0.1, 0.95, c).astype(np.float32)
            rows[f, e, :c, 4] = np.sort(cf)[::-1]
            iv = rows[f, e].view(np.int32)
            iv[:c, 5] = rng.integers(0, n_cls, c)
            iv[:c, 6] = rng.integers(0, 8400, c)
            if kpt:
                rows[f, e, :c, 7:] = rng.uniform(0, extent, (c, MAX_KPT_FLOATS)).astype(np.float32)
            else:
                rows[f, e, :c, 7:] = 0
    return rows


def _pair_metric(a, b, metric):
    """the metric of two boxes in the canonical fp32 order, and (iou) with w * h contracted into the subtraction, as an fma would give"""
    w = F32(min(a[2], b[2]) - max(a[0], b[0]))
    h = F32(min(a[3], b[3]) - max(a[1], b[1]))
    inter = F32(w * h)
    aa = F32(F32(a[2] - a[0]) * F32(a[3] - a[1]))
    ab = F32(F32(b[2] - b[0]) * F32(b[3] - b[1]))
    if metric == "ios":
        return F32(inter / min(aa, ab)), None
    s = F32(aa + ab)
    fused = F32(np.float64(s) - np.float64(w) * np.float64(h))
    return F32(inter / F32(s - inter)), F32(inter / fused)


def threshold_pair(metric, seed=99):
    """two overlapping boxes a, b (float32 [4]) with their metric m strictly inside (0, 1) -> (a, b, m, fused m or None); for "iou" a
    pair on which the contracted arithmetic gives another m than the canonical one"""
    rng = np.random.default_rng(seed)
    for _ in range(10000):
        a = np.array([0, 0, rng.uniform(5, 50), rng.uniform(5, 50)], np.float32)
        b = np.array([rng.uniform(0, 4), rng.uniform(0, 4), rng.uniform(6, 60), rng.uniform(6, 60)], np.float32)
        m, mf = _pair_metric(a, b, metric)
        if 0.05 < m < 0.95 and (metric == "ios" or mf != m):
            return a, b, m, mf
    raise AssertionError("no pair found")
