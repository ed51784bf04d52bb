"""The case table of the evidence-frame rasteriser, shared by tests/test_render_cases.py (host twin) and
tests/test_gpu_render.py (kernel): CASES[name] = (frame uint8 [H, W, 3], prims int32 [P, 8]); reference(name) = the checker's picture,
computed once per process."""
import functools

import numpy as np

import _render_numpy as R

M, RECT, FILL, LINE, DISC, GLYPH = R.MOSAIC, R.RECT, R.FILL, R.LINE, R.DISC, R.GLYPH


def frame(h, w, seed=0):
    return np.random.default_rng(1000 * h + w + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def P(*rows):
    a = np.zeros((len(rows), 8), np.int32)
    for i, r in enumerate(rows):
        a[i, :len(r)] = r
    return a


def col(i):
    return [0x0000FF, 0x00FF00, 0xFF0000, 0x00FFFF, 0xFF00FF, 0xFFFF00, 0x102030, 0xFFFFFF][i % 8]


def _many(n, seed):
    """n mixed primitives whose bounding boxes all meet the tile (0, 0) .. (31, 31)"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        k = i % 5
        x, y = int(rng.integers(0, 32)), int(rng.integers(0, 32))
        if k == 0:
            rows.append((LINE, x, y, int(rng.integers(-10, 70)), int(rng.integers(-10, 60)), int(rng.integers(1, 4)), col(i)))
        elif k == 1:
            rows.append((DISC, x, y, 0, 0, int(rng.integers(0, 6)), col(i)))
        elif k == 2:
            rows.append((RECT, x - 9, y - 7, x + 9, y + 7, int(rng.integers(1, 3)), col(i)))
        elif k == 3:
            rows.append((GLYPH, x - 3, y - 3, ord("0123456789#.:%- "[i % 16]), 0, int(rng.integers(1, 3)), col(i)))
        else:
            rows.append((M, x - 5, y - 5, x + 12, y + 9, (4, 8, 16, 32)[i % 4], 0))
    return P(*rows)


def _build():
    c = {}
    f = frame(48, 64)
    # every primitive type alone on 64 x 48
    c["mosaic"] = (f, P((M, 10, 6, 45, 40, 8, 0)))
    c["rect"] = (f, P((RECT, 5, 4, 50, 40, 2, col(0))))
    c["fill"] = (f, P((FILL, 5, 4, 50, 40, 0, col(1))))
    c["line"] = (f, P((LINE, 3, 5, 60, 41, 3, col(2))))
    c["disc"] = (f, P((DISC, 30, 20, 0, 0, 5, col(3))))
    c["glyph"] = (f, P((GLYPH, 20, 10, ord("8"), 0, 3, col(4))))
    c["label"] = (f, P((FILL, 2, 2, 60, 12, 0, col(2)), *[(GLYPH, 3 + 6 * i, 4, ord(ch), 0, 1, col(7)) for i, ch in enumerate("#12 0.87:%-")]))
    # neither side a tile multiple; tiny frames
    g = frame(33, 70)
    c["33x70"] = (g, P((M, -3, 20, 69, 40, 16, 0), (RECT, 1, 1, 68, 31, 3, col(0)), (LINE, 0, 32, 69, 0, 2, col(1)), (DISC, 69, 32, 0, 0, 5, col(2)),
                       (GLYPH, 60, 27, ord("7"), 0, 2, col(3)), (FILL, 31, 31, 33, 32, 0, col(4))))
    c["1x1"] = (frame(1, 1), P((DISC, 0, 0, 0, 0, 0, col(0))))
    c["1x1_mosaic"] = (frame(1, 1), P((M, -5, -5, 5, 5, 32, 0)))
    c["1x1_untouched"] = (frame(1, 1), P((DISC, 1, 0, 0, 0, 0, col(0)), (LINE, 2, 2, 9, 9, 1, col(1))))
    c["1x40"] = (frame(1, 40), P((LINE, -5, 0, 50, 0, 1, col(1)), (M, 30, 0, 39, 0, 4, 0), (GLYPH, 33, -3, ord("4"), 0, 1, col(2)), (DISC, 36, 2, 0, 0, 2, col(5))))
    # primitives that straddle tile corners (the corner at x = 32, y = 32)
    c["corners"] = (f, P((DISC, 32, 32, 0, 0, 5, col(0)), (RECT, 28, 28, 36, 36, 2, col(1)), (LINE, 30, 30, 34, 34, 3, col(2)), (GLYPH, 30, 29, ord("#"), 0, 1, col(3)),
                         (FILL, 31, 31, 32, 32, 0, col(4)), (M, 30, 30, 34, 34, 4, 0)))
    # wholly and partly off the frame, negative and far coordinates
    far = 100000
    c["off_frame"] = (f, P((RECT, -far, -far, far, far, 3, col(0)), (RECT, -5, -5, 20, 20, 6, col(1)), (FILL, -far, 40, far, 50, 0, col(2)),
                           (LINE, -far, -far, far, far, 3, col(3)), (LINE, -far, 10, far, 30, 2, col(4)), (LINE, 70, 5, 200, 6, 1, col(5)),
                           (LINE, far, -far, -far, far, 6, col(6)), (DISC, -3, -3, 0, 0, 5, col(5)), (DISC, far, far, 0, 0, 5, col(6)),
                           (DISC, -far, 20, 0, 0, far + 4, col(7)), (GLYPH, -4, -6, ord("5"), 0, 3, col(7)), (GLYPH, far, 0, ord("5"), 0, 1, col(0)),
                           (M, -far, -far, 10, 10, 8, 0), (M, 60, 44, far, far, 16, 0), (M, far, far, far + 5, far + 5, 4, 0)))
    c["empty_rects"] = (f, P((FILL, 20, 10, 19, 30, 0, col(0)), (RECT, 20, 30, 40, 29, 2, col(1)), (M, 30, 10, 10, 30, 8, 0), (FILL, 10, 30, 30, 10, 0, col(2))))
    c["a_eq_b"] = (f, P(*[(LINE, 8 + 12 * i, 20, 8 + 12 * i, 20, t, col(i)) for i, t in enumerate((1, 2, 3, 6))], (LINE, 0, 0, 0, 0, 6, col(5))))
    for t in (1, 2, 3, 6):
        c[f"thickness_{t}"] = (f, P((LINE, 4, 40, 58, 8, t, col(t)), (RECT, 6, 6, 56, 42, t, col(t + 1)), (LINE, 10, 3, 10, 44, t, col(t + 2)), (LINE, 2, 24, 62, 24, t, col(t + 3))))
    c["radii"] = (f, P((DISC, 10, 10, 0, 0, 0, col(0)), (DISC, 20, 10, 0, 0, 1, col(1)), (DISC, 40, 25, 0, 0, 5, col(2))))
    c["slopes"] = (f, P((LINE, 5, 2, 9, 45, 2, col(0)), (LINE, 2, 40, 61, 44, 2, col(1)), (LINE, 0, 12, 63, 12, 1, col(2)), (LINE, 50, 0, 50, 47, 3, col(3)),
                        (LINE, 10, 5, 45, 40, 2, col(4)), (LINE, 45, 5, 10, 40, 1, col(5)), (LINE, 60, 47, 3, 1, 6, col(6))))
    h = frame(45, 75)                           # every block size cut by the right and the bottom edge
    for B in (4, 8, 16, 32):
        c[f"mosaic_edge_{B}"] = (h, P((M, 40, 20, 74, 44, B, 0), (M, 0, 0, 5, 5, B, 0)))
    c["mosaic_overlap"] = (f, P((M, 5, 5, 40, 30, 8, 0), (M, 20, 15, 60, 45, 8, 0)))
    c["mosaic_overlap_mixed"] = (f, P((M, 5, 5, 40, 30, 16, 0), (M, 20, 15, 60, 45, 4, 0), (M, 30, 0, 35, 47, 32, 0)))
    c["mosaic_under_line"] = (f, P((LINE, 0, 0, 63, 47, 3, col(0)), (M, 8, 8, 55, 40, 16, 0), (DISC, 30, 22, 0, 0, 5, col(3))))
    c["70_on_a_tile"] = (f, _many(70, 7))
    c["200_on_a_tile"] = (f, _many(200, 8))
    c["empty_list"] = (f, P())
    return c


CASES = _build()


@functools.lru_cache(maxsize=None)
def reference(name):
    f, p = CASES[name]
    out = R.render(f, p)
    out.setflags(write=False)
    return out
