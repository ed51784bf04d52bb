"""The evidence-frame rasteriser as a sequential numpy statement (include/mi355_yolo.h "evidence frames"): one Python
loop over the primitives, a boolean mask per primitive.  Written from the rules' text, not from csrc/render_raster.h: no tiles, no bins,
exact Python integers (object arrays) wherever a product could leave 64 bits.

    render(frame [H, W, 3] uint8, prims int32 [P, 8]) -> uint8 [H, W, 3]

A record is {type, a, b, c, d, size, colour, 0}; colour = B | G << 8 | R << 16."""
import numpy as np

MOSAIC, RECT, FILL, LINE, DISC, GLYPH = 1, 2, 3, 4, 5, 6

# 5 x 7, rows top to bottom, '#' = set
FONT = {
    "0": [".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."],
    "1": ["..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."],
    "2": [".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"],
    "3": ["#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."],
    "4": ["...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."],
    "5": ["#####", "#....", "####.", "....#", "....#", "#...#", ".###."],
    "6": ["..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."],
    "7": ["#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."],
    "8": [".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."],
    "9": [".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."],
    "#": [".#.#.", ".#.#.", "#####", ".#.#.", "#####", ".#.#.", ".#.#."],
    ".": [".....", ".....", ".....", ".....", ".....", ".##..", ".##.."],
    ":": [".....", ".##..", ".##..", ".....", ".##..", ".##..", "....."],
    "%": ["##...", "##..#", "...#.", "..#..", ".#...", "#..##", "...##"],
    "-": [".....", ".....", ".....", "#####", ".....", ".....", "....."],
    " ": ["....."] * 7,
}


def _grid(h, w):
    """exact integer pixel coordinates: py [H, 1], px [1, W]"""
    return np.arange(h, dtype=object).reshape(h, 1), np.arange(w, dtype=object).reshape(1, w)


def _rect(py, px, x0, y0, x1, y1):
    return ((px >= x0) & (px <= x1)) & ((py >= y0) & (py <= y1))


def _window(p, h, w):
    """rows and columns outside which the primitive certainly covers nothing (generous): only frames too large to evaluate every
    primitive on every pixel use it"""
    t, a, b, c, d, size = (int(v) for v in p[:6])
    if t == LINE:
        x0, x1, y0, y1 = min(a, c) - size, max(a, c) + size, min(b, d) - size, max(b, d) + size
    elif t == DISC:
        x0, x1, y0, y1 = a - size, a + size, b - size, b + size
    elif t == GLYPH:
        x0, x1, y0, y1 = a, a + 5 * size, b, b + 7 * size
    else:
        x0, x1, y0, y1 = a, c, b, d
    clip = lambda v, hi: max(0, min(hi, v))
    return clip(y0, h), clip(y1 + 1, h), clip(x0, w), clip(x1 + 1, w)


def mask_of(p, h, w):
    """the pixel set of one primitive other than a mosaic, as a boolean [H, W]"""
    if h * w > 64 * 64:
        r0, r1, c0, c1 = _window(p, h, w)
        m = np.zeros((h, w), bool)
        if r1 > r0 and c1 > c0:
            q = np.array(p).copy()
            q[1] -= c0
            q[2] -= r0
            if int(p[0]) in (MOSAIC, RECT, FILL, LINE):
                q[3] -= c0
                q[4] -= r0
            m[r0:r1, c0:c1] = _mask_full(q, r1 - r0, c1 - c0)
        return m
    return _mask_full(p, h, w)


def _mask_full(p, h, w):
    t, a, b, c, d, size = (int(v) for v in p[:6])
    py, px = _grid(h, w)
    if t == FILL:
        m = _rect(py, px, a, b, c, d)
    elif t == RECT:
        m = _rect(py, px, a, b, c, d) & ~_rect(py, px, a + size, b + size, c - size, d - size)
    elif t == DISC:
        m = (px - a) ** 2 + (py - b) ** 2 <= size * size
    elif t == LINE:
        dx, dy = c - a, d - b
        qx, qy = px - a, py - b
        u = qx * dx + qy * dy
        len2 = dx * dx + dy * dy
        before = u <= 0
        after = ~before & (u >= len2)
        near_a = 4 * (qx * qx + qy * qy) <= size * size
        near_b = 4 * ((px - c) ** 2 + (py - d) ** 2) <= size * size
        cross = dx * qy - dy * qx
        near_l = 4 * cross * cross <= size * size * len2
        m = np.where(before, near_a, np.where(after, near_b, near_l))
    elif t == GLYPH:
        rows = FONT[chr(c)]
        m = np.zeros((h, w), bool)
        for r in range(7):
            for col in range(5):
                if rows[r][col] == "#":
                    m |= _rect(py, px, a + col * size, b + r * size, a + (col + 1) * size - 1, b + (r + 1) * size - 1)
    else:
        raise ValueError(f"unknown primitive type {t}")
    return np.broadcast_to(m, (h, w)).astype(bool)


def mosaic_means(frame, B):
    """every pixel's block mean: blocks aligned to the origin, an edge block as large as the frame leaves it, halves rounded up"""
    h, w, _ = frame.shape
    out = np.empty_like(frame)
    for y in range(0, h, B):
        for x in range(0, w, B):
            blk = frame[y:y + B, x:x + B].astype(np.int64)
            n = blk.shape[0] * blk.shape[1]
            out[y:y + B, x:x + B] = (2 * blk.sum(axis=(0, 1)) + n) // (2 * n)
    return out


def render(frame, prims):
    frame = np.asarray(frame)
    h, w, _ = frame.shape
    prims = np.asarray(prims).reshape(-1, 8)
    out = frame.copy()
    py, px = _grid(h, w)
    for p in prims:                                   # the mosaics first: all of them read the SOURCE
        if int(p[0]) == MOSAIC:
            m = np.broadcast_to(_rect(py, px, int(p[1]), int(p[2]), int(p[3]), int(p[4])), (h, w)).astype(bool)
            if m.any():
                out[m] = mosaic_means(frame, int(p[5]))[m]
    for p in prims:                                   # then everything else, the last writer wins
        if int(p[0]) != MOSAIC:
            col = int(p[6])
            out[mask_of(p, h, w)] = (col & 255, (col >> 8) & 255, (col >> 16) & 255)
    return out
