"""Inputs, case list and references of tests/test_gpu_sparse_box.py: the three kernels of the sparse box branch
(csrc/conv_f32_sparse.hip) alone, through cvsd_amd.ops.sparse_box.

Nothing here needs a GPU: numpy and the canonical-order oracle (oracle.det) only.  tests/test_sparse_box_cases.py checks that the
planted score patterns hold every edge they claim and that they tell the true list reference from six wrong ones.

There are 9 cases (CASES): five on the main shape, one full-level case on it, one 1x1 map, one two-level case -- and two more
that rerun the `lengths` inputs with one list capacity one entry short (the overflow cases)."""
import functools
from collections import Counter

import numpy as np

MAIN = ((12, 20, 8), (6, 10, 16), (3, 5, 32))     # h, w, stride: A = 315 (two 256-anchor blocks, the second ragged), H != W everywhere,
MAIN_N = 3                                         # level 0 / 1 boundary at anchor 240 inside block 0, 720 level-0 positions in the batch
TWO = ((6, 10, 16), (3, 5, 32))
TINY = ((1, 1, 8),)
CONF = np.float32(0.25)
CLASS_LIST = (0, 31, 32, 63, 64, 79)               # both ends of mask words 0, 1 and 2 (nc 80)
LENGTHS = (1, 16, 17, 64, 65)                      # list lengths that must occur, and one above 128: the 16-entry waves and 64-entry
                                                   # blocks of the gathered convs exactly full, and one entry over


# ---------------------------------------------------------------------------------------------------------- score patterns
class Scores:
    """best[n, A, 2] under construction: every score 0 (below any conf used here), class 0"""

    def __init__(self, n, shapes):
        self.n, self.shapes = n, shapes
        self.A = sum(h * w for h, w, _ in shapes)
        self.a0 = np.cumsum([0] + [h * w for h, w, _ in shapes])[:-1]
        self.best = np.zeros((n, self.A, 2), np.float32)

    def put(self, b, l, y, x, score=0.9, cls=0):
        h, w, _ = self.shapes[l]
        assert 0 <= y < h and 0 <= x < w and 0 <= b < self.n
        self.best[b, self.a0[l] + y * w + x] = (score, cls)

    def block(self, b, l, ys, xs, score=0.9, cls=0):
        for y in ys:
            for x in xs:
                self.put(b, l, y, x, score, cls)


def _edges(s):
    """frame 0: the four corners and one pixel on each edge of level 0 ((5, 19) is the row end whose wrap-around neighbours (5, 0)
    and (6, 0) must stay clear), the first pixel of level 1, the last pixel of the frame; frame 1: nothing; frame 2: the special
    scores, each with a clear 5x5 neighbourhood"""
    for y, x in ((0, 0), (0, 19), (11, 0), (11, 19), (0, 9), (11, 9), (9, 0), (5, 19)):
        s.put(0, 0, y, x)
    s.put(0, 1, 0, 0)
    s.put(0, 2, 2, 4)
    s.put(2, 0, 3, 3, CONF)                                      # exactly conf: out
    s.put(2, 0, 3, 8, np.nextafter(CONF, np.float32(1)))         # one ulp above: in
    s.put(2, 0, 3, 13, np.inf)
    s.put(2, 0, 8, 3, np.nan)                                    # neither listed nor dilating
    s.put(2, 0, 8, 13, np.nextafter(CONF, np.float32(0)))        # one ulp below: out


def _lengths(s):
    """dilated lists of 64 (level 0: 4 interior singles 9 each, 4 corners 4 each, 2 top-edge singles 6 each), 16 (level 1: a run
    of 6 on the top edge, frame 1) and 17 (level 2: the centre of frame 0, two corners of frame 1)"""
    for y, x in ((3, 3), (3, 9), (6, 6), (9, 12), (0, 0), (0, 19), (11, 0), (11, 19), (0, 5), (0, 13)):
        s.put(0, 0, y, x)
    s.block(1, 1, (0,), range(2, 8))
    s.put(0, 2, 1, 2)
    s.put(1, 2, 0, 0)
    s.put(1, 2, 2, 4)


def _lengths2(s):
    """dilated 65 on level 0 (5 interior singles, 2 corners, 2 top-edge singles, over frames 0 and 2); candidates 16 on level 1 (a
    2x8 block of frame 2) and 17 on level 2 (all of frame 0, two of frame 2)"""
    for b, y, x in ((0, 3, 3), (0, 3, 9), (0, 6, 6), (2, 9, 12), (2, 6, 15), (0, 0, 0), (2, 11, 19), (0, 0, 5), (2, 0, 13)):
        s.put(b, 0, y, x)
    s.block(2, 1, (2, 3), range(1, 9))
    s.block(0, 2, range(3), range(5))
    s.put(2, 2, 0, 1)
    s.put(2, 2, 2, 3)


def _masked(s):
    """nc 80 behind the class list.  Level 0: anchors 0 .. 63 of frame 0 (a lists-kernel wave with every lane flagged; the wave
    behind it has none) and anchor 130 of frame 1 (its wave's first flagged lane is lane 2): 65 candidates, classes cycling through
    the list.  Level 1: all of frame 0 and four of frame 1: 64.  Level 2: one listed class, and classes outside the list at 0.99."""
    for a in range(64):
        s.put(0, 0, a // 20, a % 20, 0.5 + a / 256, CLASS_LIST[a % 6])
    s.put(1, 0, 6, 10, 0.9, 63)
    s.block(0, 1, range(6), range(10), 0.9, 32)
    for x in range(4):
        s.put(1, 1, 0, x, 0.9, CLASS_LIST[x + 2])
    s.put(0, 2, 0, 0, 0.9, 79)
    s.put(1, 2, 1, 3, 0.99, 5)                                   # not in the list
    s.put(2, 2, 1, 1, 0.99, 33)
    s.put(2, 0, 6, 6, 0.99, 78)


def _full(s):
    """every position of level 1 in every frame (180 > 128 entries in both lists); level 0 empty; level 2: the frame's last pixel"""
    for b in range(s.n):
        s.block(b, 1, range(6), range(10))
    s.put(1, 2, 2, 4)


def _tiny(s):
    s.put(0, 0, 0, 0)


def _last_frame_only(s):
    s.put(s.n - 1, 0, 0, 0)
    s.put(s.n - 1, 1, 1, 2)


# name: shapes, n, cin, (src cs, src_off), cout_a, (mid_cs, mid_off), nc, no, classes, pattern, scale of cv2.i.2, capacities
#   capacities: "ample" = every position; "exact" = the reference counts; "dil-1" / "cand-1": level 0's list one entry short
CASES = {
    "edges":      dict(shapes=MAIN, n=MAIN_N, cin=16, view=(16, 0), cout_a=64, mid=(64, 0), nc=1, no=5, pattern=_edges),
    "lengths":    dict(shapes=MAIN, n=MAIN_N, cin=64, view=(88, 8), cout_a=80, mid=(144, 16), nc=2, no=6, pattern=_lengths, caps="exact"),
    "lengths2":   dict(shapes=MAIN, n=MAIN_N, cin=128, view=(128, 0), cout_a=64, mid=(64, 0), nc=3, no=7, pattern=_lengths2),
    "masked":     dict(shapes=MAIN, n=MAIN_N, cin=16, view=(24, 4), cout_a=144, mid=(144, 80), nc=80, no=84, pattern=_masked,
                       classes=CLASS_LIST),
    "full":       dict(shapes=MAIN, n=MAIN_N, cin=64, view=(64, 0), cout_a=64, mid=(144, 64), nc=1, no=56, pattern=_full, scale_c=8.0),
    "tiny":       dict(shapes=TINY, n=1, cin=16, view=(16, 0), cout_a=64, mid=(64, 0), nc=1, no=5, pattern=_tiny, caps="exact"),
    "last_frame": dict(shapes=TWO, n=2, cin=128, view=(136, 8), cout_a=64, mid=(64, 0), nc=80, no=84, pattern=_last_frame_only),
    "over_dil":   dict(base="lengths", caps="dil-1"),
    "over_cand":  dict(base="lengths", caps="cand-1"),
}
PLAIN_CASES = tuple(k for k, v in CASES.items() if "base" not in v)
OVERFLOW_CASES = tuple(k for k, v in CASES.items() if "base" in v)


# -------------------------------------------------------------------------------------------------------------- references
def level_slices(shapes):
    a0 = 0
    for h, w, _ in shapes:
        yield a0, h, w
        a0 += h * w


def mask_words(classes, nc):
    m = np.zeros((nc + 31) // 32, np.uint32)
    for c in classes:
        m[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    return m


def candidates(best, conf, classes=None, nc=None, ge=False, nan_passes=False, word0_only=False):
    """[n, A] bool: score > conf, strictly (so a NaN is out), and the class in the list when there is one.  The three flags are
    the wrong variants the CPU test holds against it."""
    sc, cl = best[..., 0], best[..., 1]
    with np.errstate(invalid="ignore"):
        ok = (sc >= np.float32(conf)) if ge else (sc > np.float32(conf))
    if nan_passes:
        ok = ok | np.isnan(sc)
    if classes is not None:
        m = mask_words(classes, nc)
        c = cl.astype(np.int64)
        words = m[np.zeros_like(c)] if word0_only else m[c >> 5]
        ok = ok & ((words >> (c & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)
    return ok


def dilate(cand, shapes, wrong=None):
    """[n, A] bool -> [n, A] bool: any in-image 3x3 neighbour of the same frame and level is a candidate.
    wrong = "row" (x is not checked: the flat index wraps over the row end), "level" (y is not checked against the level: the flat
    anchor index runs into the next level), "frame" (y is not checked at all: the list index b*H*W + ... runs into the next frame)"""
    n, A = cand.shape
    out = np.zeros_like(cand)
    for a0, h, w in level_slices(shapes):
        c = cand[:, a0:a0 + h * w]
        for b, li in zip(*np.nonzero(c)):
            y, x = divmod(int(li), w)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if wrong == "row":
                        if 0 <= yy < h and 0 <= yy * w + xx < h * w:
                            out[b, a0 + yy * w + xx] = True
                    elif not 0 <= xx < w:
                        continue
                    elif wrong == "level":
                        if 0 <= a0 + yy * w + xx < A:
                            out[b, a0 + yy * w + xx] = True
                    elif wrong == "frame":
                        v = b * h * w + yy * w + xx
                        if 0 <= v < n * h * w:
                            out[v // (h * w), a0 + v % (h * w)] = True
                    elif 0 <= yy < h:
                        out[b, a0 + yy * w + xx] = True
    return out


def entries(flags, shapes):
    """[n, A] bool -> per level the sorted list entries b*H*W + y*W + x"""
    out = []
    for a0, h, w in level_slices(shapes):
        b, li = np.nonzero(flags[:, a0:a0 + h * w])
        out.append(np.sort(b * h * w + li).astype(np.int32))
    return out


class SparseCase:
    def __init__(self, name, shapes, n, cin, view, cout_a, mid, nc, no, pattern, classes=None, scale_c=1.0, caps="ample"):
        from oracle import det
        self.name, self.shapes, self.n, self.nc, self.no, self.classes, self.conf = name, shapes, n, nc, no, classes, CONF
        self.cin, self.view, self.cout_a, self.mid = cin, view, cout_a, mid
        s = Scores(n, shapes)
        pattern(s)
        self.best, self.A = s.best, s.A
        self.cand = candidates(self.best, CONF, classes, nc)
        self.dil = dilate(self.cand, shapes)
        self.ref_cand, self.ref_dil = entries(self.cand, shapes), entries(self.dil, shapes)
        rng = np.random.default_rng([len(name), cin, cout_a, no, n])
        cs, off = view
        box = np.zeros((n, 5, self.A), np.float32)
        self.inputs, self.ref_mid = [], []
        for (a0, h, w), (_, _, stride) in zip(level_slices(shapes), shapes):
            conv = lambda co, ci, k, sc=1.0: ((rng.standard_normal((co, ci, k, k)) / np.sqrt(ci * k * k) * sc).astype(np.float32),
                                             (rng.standard_normal(co) * sc).astype(np.float32))
            src = rng.standard_normal((n, h, w, cs), dtype=np.float32)
            (wA, bA), (wB, bB), (wC, bC) = conv(cout_a, cin, 3), conv(64, 64, 3), conv(64, 64, 1, scale_c)
            for a in (src, wA, bA, wB, bB, wC, bC):
                a.flags.writeable = False
            self.inputs.append(dict(src=src, src_off=off, cin=cin, wA=wA, bA=bA, wB=wB, bB=bB, wC=wC, bC=bC, stride=stride,
                                    mid_cs=mid[0], mid_off=mid[1]))
            # the dense chain in canonical order; the sparse kernels promise its bits at the listed positions
            m = np.ascontiguousarray(det.conv2d(src[..., off:off + cin], wA, bA)[..., :64])
            lg = det.conv2d(det.conv2d(m, wB, bB), wC, bC, act=False)
            det.lib().det_decode_level(lg.ctypes.data, np.zeros((n, h, w, 1), np.float32).ctypes.data, None, n, h, w, 1, 0, 0, stride,
                                       a0, self.A, box.ctypes.data)
            self.ref_mid.append(m)
        self.ref_box = np.ascontiguousarray(box.transpose(0, 2, 1)[:, :, :4])          # [n, A, 4]
        self.set_caps(caps)

    def set_caps(self, caps):
        self.caps = caps
        for l, (lv, (h, w, _)) in enumerate(zip(self.inputs, self.shapes)):
            nd, ncd, pos = len(self.ref_dil[l]), len(self.ref_cand[l]), self.n * h * w
            if caps == "ample" or (caps != "exact" and l > 0):
                lv["cap_dil"], lv["cap_cand"] = pos, pos
            elif caps == "exact":
                lv["cap_dil"], lv["cap_cand"] = max(nd, 1), max(ncd, 1)
            elif caps == "dil-1":
                lv["cap_dil"], lv["cap_cand"] = nd - 1, pos
            elif caps == "cand-1":
                lv["cap_dil"], lv["cap_cand"] = pos, ncd - 1
            else:
                raise ValueError(caps)
        self.overflows = caps in ("dil-1", "cand-1")

    def frame(self, i):
        """(levels, best) of frame i alone, every capacity ample"""
        lvs = [dict(lv, src=np.ascontiguousarray(lv["src"][i:i + 1]), cap_dil=None, cap_cand=None) for lv in self.inputs]
        return lvs, np.ascontiguousarray(self.best[i:i + 1])


@functools.lru_cache(maxsize=None)
def case(name):
    kw = dict(CASES[name])
    if "base" in kw:
        import copy
        c = copy.copy(case(kw["base"]))
        c.name, c.inputs = name, [dict(lv) for lv in c.inputs]
        c.set_caps(kw["caps"])
        return c
    return SparseCase(name, **kw)


# ------------------------------------------------------------------------------------------------------------------ census
def census(c):
    """what a case's scores hold, read back from best[] and the references (not from the pattern's intent)"""
    out = Counter()
    n, A, shapes = c.n, c.A, c.shapes
    sc = c.best[..., 0]
    lv = list(level_slices(shapes))
    for l, (a0, h, w) in enumerate(lv):
        cd, dl = c.cand[:, a0:a0 + h * w].reshape(n, h, w), c.dil[:, a0:a0 + h * w].reshape(n, h, w)
        if l == 0 and h > 2 and w > 2:
            if cd[:, 0, 0].any() and cd[:, 0, -1].any() and cd[:, -1, 0].any() and cd[:, -1, -1].any():
                out["four_corners"] += 1
            if cd[:, 0, 1:-1].any() and cd[:, -1, 1:-1].any() and cd[:, 1:-1, 0].any() and cd[:, 1:-1, -1].any():
                out["each_edge"] += 1
            for b, y in zip(*np.nonzero(cd[:, :-1, -1])):
                if not dl[b, y, 0] and not dl[b, y + 1, 0]:
                    out["row_end_with_clear_wrap_neighbours"] += 1
        if cd.all():
            out["full_level"] += 1
        for kind, cnt in (("dil", int(dl.sum())), ("cand", int(cd.sum()))):
            if cnt in LENGTHS:
                out[f"{kind}_len_{cnt}"] += 1
            if cnt > 128:
                out[f"{kind}_len_over_128"] += 1
            if cnt == 0:
                out[f"{kind}_len_0"] += 1
    if len(lv) > 1 and c.cand[0, lv[1][0] - 1] and c.cand[0, lv[1][0]]:
        out["last_of_level0_and_first_of_level1"] += 1
    if c.cand[0, A - 1] and n > 1:
        out["last_pixel_of_frame0"] += 1
    per_frame = c.cand.sum(1)
    if (per_frame == 0).any() and per_frame.any():
        out["a_frame_without_candidates"] += 1
    if n > 1 and per_frame[-1] > 0 and not per_frame[:-1].any():
        out["only_the_last_frame"] += 1
    # the special scores; "not dilating": nothing in the 3x3 around it is dilated (so nothing else hides a wrong answer)
    def clear_around(b, a):
        l = max(i for i, (a0, _, _) in enumerate(lv) if a >= a0)
        a0, h, w = lv[l]
        y, x = divmod(a - a0, w)
        return not c.dil[b, a0:a0 + h * w].reshape(h, w)[max(0, y - 1):y + 2, max(0, x - 1):x + 2].any()
    for b, a in zip(*np.nonzero(sc == c.conf)):
        if not c.cand[b, a]:
            out["score_equals_conf_not_listed"] += 1
    for b, a in zip(*np.nonzero(sc == np.nextafter(c.conf, np.float32(1)))):
        if c.cand[b, a]:
            out["score_one_ulp_above_conf_listed"] += 1
    for b, a in zip(*np.nonzero(np.isposinf(sc))):
        if c.cand[b, a]:
            out["inf_listed"] += 1
    for b, a in zip(*np.nonzero(np.isnan(sc))):
        if not c.cand[b, a] and clear_around(b, a):
            out["nan_neither_listed_nor_dilating"] += 1
    if c.classes is not None:
        if set(c.best[..., 1][c.cand].astype(int).tolist()) >= set(c.classes) and max(c.classes) >= 64:
            out["every_listed_class_kept"] += 1
        for b, a in zip(*np.nonzero((sc == np.float32(0.99)) & ~np.isin(c.best[..., 1], c.classes))):
            if not c.cand[b, a] and clear_around(b, a):
                out["excluded_class_at_0.99_neither_listed_nor_dilating"] += 1
    # the lists kernel's waves: 64 consecutive anchors of a frame; its append ballots one (flag, level) at a time
    for flags, kind in ((c.cand, "cand"), (c.dil, "dil")):
        for l, (a0, h, w) in enumerate(lv):
            f = np.zeros((n, A), bool)
            f[:, a0:a0 + h * w] = flags[:, a0:a0 + h * w]
            for b in range(n):
                for k in range(0, A, 64):
                    wv = f[b, k:k + 64]
                    if len(wv) == 64 and wv.all():
                        out[f"{kind}_wave_all_flagged"] += 1
                    if not wv.any():
                        out[f"{kind}_wave_none_flagged"] += 1
                    elif not wv[0]:
                        out[f"{kind}_wave_first_flag_not_lane0"] += 1
    nd, ncd = [len(e) for e in c.ref_dil], [len(e) for e in c.ref_cand]
    cd_, cc_ = [lv_["cap_dil"] for lv_ in c.inputs], [lv_["cap_cand"] for lv_ in c.inputs]
    if all(a == max(b, 1) for a, b in zip(cd_ + cc_, nd + ncd)) and sum(nd) > 0:
        out["caps_equal_counts"] += 1
    if any(a == b - 1 for a, b in zip(cd_, nd)):
        out["cap_dil_one_short"] += 1
    if any(a == b - 1 for a, b in zip(cc_, ncd)) and all(a >= b for a, b in zip(cd_, nd)):
        out["cap_cand_one_short_cap_dil_ample"] += 1
    # cv2.i.2 times 8: weights of N(0, 1 / 64) and biases of N(0, 1) stay below 1 and 5, eight times that does not
    if all(np.abs(lv_["wC"]).max() > 2 and np.abs(lv_["bC"]).max() > 8 for lv_ in c.inputs) and sum(ncd) > 128:
        out["peaked_dfl"] += 1
    return out


REQUIRED = (
    "four_corners", "each_edge", "last_of_level0_and_first_of_level1", "last_pixel_of_frame0", "row_end_with_clear_wrap_neighbours",
    "a_frame_without_candidates", "only_the_last_frame", "score_equals_conf_not_listed", "score_one_ulp_above_conf_listed", "inf_listed",
    "nan_neither_listed_nor_dilating", "every_listed_class_kept", "excluded_class_at_0.99_neither_listed_nor_dilating", "full_level",
    "cand_wave_all_flagged", "cand_wave_none_flagged", "cand_wave_first_flag_not_lane0", "caps_equal_counts", "cap_dil_one_short",
    "cap_cand_one_short_cap_dil_ample", "peaked_dfl",
) + tuple(f"{k}_len_{v}" for k in ("dil", "cand") for v in LENGTHS + ("over_128",))
