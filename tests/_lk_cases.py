"""Frame pairs, points and the traced float64 reference for the per-point tests of pyramidal Lucas-Kanade: the host C++
(csrc/gmc_host.cpp, tests/test_lk_cases.py) and the HIP kernel (csrc/gmc_kernels.hip: lk_kernel, tests/test_gpu_lk.py) against
tests/_lk_numpy.py:lk_traced, which is oracle/gmc_oracle.py:calc_optical_flow_pyr_lk bit for bit.

A frame pair is an analytic texture (a sum of sinusoids, a function of continuous coordinates) sampled on the pixel grid and at the
pre-image of the grid under a 2x3 motion, as tests/test_gmc.py renders its pairs; a flat patch and a vertical step edge are painted into
both frames where the plane has room for them.  "rough" holds frequencies up to 0.25 cycles / px, "smooth" up to 0.06 ("fine" only
those above 0.15, "deep" down to 0.0008, for the two cases that need them): windows of 7
and less are tracked on the smooth one with motions of at most 2.5 px per level, because a 3 x 3 window on a rough texture is chaotic
in float64 itself (re-associating the window sums moves 5 % of the points by more than 1e-3 px).

A point is STABLE when (a) the smallest relative margin of its decisions (tests/_lk_numpy.py) is >= MARGIN and (b) the reference with
re-associated window sums (assoc=1) gives the same status and the same float32 position to 1 ulp and (c) the reference started
NUDGE_PX = 1e-9 px away in x and y (positive: the start tests on the pad's ends keep their side) gives the same status and a position
within NUDGE_GAIN = 1000 times the nudge.  Float64 re-association noise of a 441-term sum is ~1e-14 relative, seven orders below MARGIN;
as a position error of ~1e-13 px it stays, amplified a thousand times, five orders below the tolerance.  Every stable point is compared, the dropped ones too (the routines write
the last position of a dropped point); the unstable share is capped by tests/test_lk_cases.py.

D_HOST_MEASURED_PX is the largest deviation of the host C++ from the reference on the stable points of this table, as measured by
tests/test_lk_cases.py (which prints it).  It is zero: on all 5.6k stable points the host routine, which adds the window's terms one by
one where numpy adds them pairwise, returns the reference's float32 bits.  That is luck of rounding, not a property: the two differ in
float64 by ~1e-13 px, which moves the float32 result by one ulp whenever it straddles a rounding boundary.  So D_HOST_PX is taken no
smaller than that quantum of the output format, 2^-16 px for the coordinates below 256 px that the table's moved points have, and
LK_TOL_PX = 4 * D_HOST_PX = 6.1e-5 px bounds the kernel, whose sums -- lane-wise, then a butterfly -- are a third association of the same
length.  It is never to exceed 1e-4 px."""
import functools

import numpy as np

import _lk_numpy as N

MARGIN = 1e-7
NUDGE_PX, NUDGE_GAIN = 1e-9, 1e3
D_HOST_MEASURED_PX = 0.0      # tests/test_lk_cases.py::test_host_routine_meets_the_reference_on_every_stable_point prints it
F32_ULP_PX = 2.0 ** -16       # one float32 ulp of a coordinate in [128, 256) px: 1.53e-5
D_HOST_PX = max(D_HOST_MEASURED_PX, F32_ULP_PX)
LK_TOL_PX = 4 * D_HOST_PX     # 6.1e-5 px
assert LK_TOL_PX <= 1e-4
COORD_MAX_PX = 256.0          # what F32_ULP_PX supposes of every stable point that has moved (asserted by the CPU test)
WAVES_PER_BLOCK = 4           # csrc/gmc_kernels.hip: MI355_LK_WAVES


def per_lane(win):
    """window pixels per lane of the one-wavefront-per-point kernel"""
    return (win * win + 63) // 64


# ---------------------------------------------------------------------------------------------------------------- frames
BANDS = {"rough": (0.008, 0.25), "smooth": (0.008, 0.06), "deep": (0.0008, 0.06), "fine": (0.15, 0.3)}      # cycles / px; "deep" has structure 7 halvings up
N_WAVES = 28


def texture(seed, band):
    """band-limited texture as a function of continuous (x, y): 28 sinusoids, frequencies log-uniform in ``band`` (so every pyramid
    level has structure), any orientation -> (amp, kx, ky, phase)"""
    rng = np.random.default_rng(seed)
    f = np.exp(rng.uniform(np.log(band[0]), np.log(band[1]), N_WAVES))
    th = rng.uniform(0, 2 * np.pi, N_WAVES)
    return rng.uniform(0.5, 1.0, N_WAVES), 2 * np.pi * f * np.cos(th), 2 * np.pi * f * np.sin(th), rng.uniform(0, 2 * np.pi, N_WAVES)


def render(tex, h, w, H=None):
    """the image whose pixel (x, y) shows the texture at the pre-image of (x, y) under the 2x3 motion H"""
    amp, kx, ky, ph = tex
    if H is None or (H[:, :2] == np.eye(2)).all():             # a shift: sin(a + b) by its addition theorem, two small matrix products
        x = np.arange(w) - (0.0 if H is None else H[0, 2])
        y = np.arange(h) - (0.0 if H is None else H[1, 2])
        ax, by = np.outer(kx, x) + ph[:, None], np.outer(y, ky)
        v = (np.cos(by) * amp) @ np.sin(ax) + (np.sin(by) * amp) @ np.cos(ax)
    else:
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
        Ai = np.linalg.inv(np.vstack([H, [0, 0, 1]]))
        xs, ys = Ai[0, 0] * xs + Ai[0, 1] * ys + Ai[0, 2], Ai[1, 0] * xs + Ai[1, 1] * ys + Ai[1, 2]
        v = np.zeros((h, w))
        for a, u, v_, p in zip(amp, kx, ky, ph):
            v += a * np.sin(u * xs + v_ * ys + p)
    return np.rint(np.clip(127.5 + v * 22.0, 0, 255)).astype(np.uint8)


def shift(dx, dy):
    return np.array([[1.0, 0.0, dx], [0.0, 1.0, dy]])


def similarity(deg, scale, dx, dy, h, w):
    """rotation by deg and scale about the plane's centre, then a shift"""
    c, s = scale * np.cos(np.radians(deg)), scale * np.sin(np.radians(deg))
    cx, cy = (w - 1) / 2, (h - 1) / 2
    return np.array([[c, -s, cx - c * cx + s * cy + dx], [s, c, cy - s * cx - c * cy + dy]])


def patches(h, w, win):
    """(flat, edge): top-left corner and side of the two painted squares, or None where the plane has no room"""
    side = min(win + 8, 29)
    if h < 2 * side + 6 or w < 2 * side + 6:
        return None
    return (4, 5, side), (w - side - 5, h - side - 4, side)


# ---------------------------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, shape, win, levels, motion, tex="rough", max_iters=30, eps=0.01, min_eig=1e-4, seed=1, pts=None):
        self.name, self.shape, self.win, self.levels, self.motion, self.tex = name, shape, win, levels, motion, tex
        self.max_iters, self.eps, self.min_eig, self.seed, self.pts = max_iters, eps, min_eig, seed, pts
        assert win > 7 or tex != "rough"

    @property
    def params(self):
        return dict(win=self.win, levels=self.levels, max_iters=self.max_iters, eps=self.eps, min_eig=self.min_eig)

    def __repr__(self):
        return self.name


MOTIONS = {
    "zero": lambda h, w: None,
    "sub": lambda h, w: shift(0.37, -0.61),
    "sim": lambda h, w: similarity(1.7, 1.02, 1.3, -0.8, h, w),
    "simsmall": lambda h, w: similarity(1.0, 1.01, 0.6, -0.4, h, w),      # under 3 px anywhere on a 97 x 131 plane; it runs at levels=3
    "big": lambda h, w: shift(5.5, 4.5),                                    # at levels=0: walks out of the 3-pixel margin
    "far": lambda h, w: shift(-27.0, 19.0),                                 # beyond reach of the levels it runs at
}


def _table():
    c = []
    P, Q, ODD = (97, 131), (64, 80), (75, 101)
    # every window (per = 1 .. 7, a region side and a box size each) at levels=3, under a similarity
    for win in range(3, 23, 2):
        c.append(Case(f"win{win}-sim", P, win, 3, "simsmall" if win <= 7 else "sim", "smooth" if win <= 7 else "rough", seed=win))
    # pyramid depth at the smallest tested and the largest window (the plane allows 3 levels above it at win 5, 2 at win 21)
    for win, tex in ((5, "smooth"), (21, "rough")):
        for levels in (0, 1, 2, 3, 5):
            c.append(Case(f"win{win}-levels{levels}", P if levels % 2 else Q, win, levels, "sub" if levels == 0 or win == 5 else "sim", tex, seed=20 + levels))
    # the loop's parameters
    for max_iters in (1, 30):
        for eps in (0.0, 0.01, 0.5):
            for min_eig in (1e-4, 1e-2):
                c.append(Case(f"win9-it{max_iters}-eps{eps:g}-eig{min_eig:g}", Q, 9, 2, "sim", max_iters=max_iters, eps=eps, min_eig=min_eig, seed=31))
    # motions
    for win, tex in ((5, "smooth"), (9, "rough"), (15, "rough"), (21, "rough")):
        c.append(Case(f"win{win}-zero", Q, win, 1, "zero", tex, seed=40))
        c.append(Case(f"win{win}-sub", P, win, 2, "sub", tex, seed=41))
        if win > 7:
            c.append(Case(f"win{win}-big-levels0", P if win == 21 else Q, win, 0, "big", tex, seed=42))
            c.append(Case(f"win{win}-far", Q, win, 1, "far", tex, seed=43))
    # a texture of fine detail only: two halvings blur it flat, so the upper levels REJECT most windows (at min_eig = 1e-2) and the point
    # goes on below, where it is tracked and kept -- a rejection above level 0 must not cost the point its status
    for win in (13, 15):
        c.append(Case(f"win{win}-fine-skips", Q, win, 3, "sub", "fine", min_eig=1e-2, seed=70))
    c.append(Case("win7-big-levels0-smooth", P, 7, 0, shift(2.4, -2.1), "smooth", seed=44))
    c.append(Case("win13-big-levels1", P, 13, 1, shift(-9.5, 8.5), seed=45))
    # shapes: a plane no larger than the window pad (no pyramid level exists), a thin one, one whose halvings are odd
    c.append(Case("win21-22x22", (22, 22), 21, 3, "sub", seed=50))
    c.append(Case("win3-5x64", (5, 64), 3, 3, "sub", "smooth", seed=51))
    c.append(Case("win5-5x64-levels0", (5, 64), 5, 0, "sub", "smooth", seed=52))
    c.append(Case("win21-5x64", (5, 64), 21, 2, "sub", seed=53))
    for win, tex in ((5, "smooth"), (11, "rough"), (21, "rough")):
        c.append(Case(f"win{win}-75x101", ODD, win, 3, "simsmall" if win <= 7 else "sim", tex, seed=54))
    assert len({k.name for k in c}) == len(c)
    return c


CASES = _table()
# The level cap (csrc/gmc_kernels.hip: kMaxLevels = 8 planes): at win=3 this plane allows 8 levels above it, 1300 x 1700 -> ... -> 6 x 7
# (the next, 3 x 4, is no larger than the window).  levels=7 fills the device pyramid; DEEP_REFUSED (levels=10) needs a ninth plane: host only.
# A dozen points, below COORD_MAX_PX so that the tolerance's float32 quantum holds for them.
_DEEP_PTS = ((20.0, 31.0), (100.5, 40.5), (63.21, 201.87), (250.0, 250.0), (7.75, 128.0), (181.3, 17.6), (0.0, 0.0), (144.9, 90.1), (33.3, 222.2),
             (212.0, 64.0), (90.62, 160.44), (236.5, 199.25))
DEEP = Case("win3-1300x1700-levels7", (1300, 1700), 3, 7, "sub", "deep", seed=60, pts=_DEEP_PTS)
DEEP_REFUSED = Case("win3-1300x1700-levels10", (1300, 1700), 3, 10, "sub", "deep", seed=60, pts=_DEEP_PTS)


@functools.lru_cache(maxsize=None)
def frames(case):
    h, w = case.shape
    fn = texture(case.seed, BANDS[case.tex])
    H = MOTIONS[case.motion](h, w) if isinstance(case.motion, str) else case.motion
    prev, cur = render(fn, h, w), render(fn, h, w, H)
    pt = patches(h, w, case.win)
    if pt is not None:
        (fx, fy, s), (ex, ey, _) = pt
        for img in (prev, cur):
            img[fy:fy + s, fx:fx + s] = 128
            img[ey:ey + s, ex:ex + s // 2] = 60
            img[ey:ey + s, ex + s // 2:ex + s] = 200
    prev.setflags(write=False); cur.setflags(write=False)
    return prev, cur


@functools.lru_cache(maxsize=None)
def points(case):
    """about 100 points: arbitrary sub-pixel, integer and half-integer positions, the four corners, points a pixel or two from a
    border, outside the frame but inside the window pad (p >= -(half + 1) and p < n + half pass the start test), on and beyond
    the pad's ends, in the flat patch and on the step edge"""
    if case.pts is not None:
        out = np.array(case.pts, np.float32)
        out.setflags(write=False)
        return out
    h, w = case.shape
    half = case.win // 2
    rng = np.random.default_rng(1000 + case.seed)
    p = [rng.uniform([0, 0], [w - 1, h - 1], (48, 2))]
    p.append(np.floor(rng.uniform([0, 0], [w - 1, h - 1], (10, 2))))
    p.append(np.floor(rng.uniform([0, 0], [w - 2, h - 2], (10, 2))) + 0.5)
    p.append([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]])
    ym, xm = (h - 1) * 0.43, (w - 1) * 0.57
    p.append([[1.25, ym], [w - 2.5, ym], [xm, 0.75], [xm, h - 1.5], [0.5, 1.0], [w - 1.0, h - 2.0], [2.0, h - 1.25], [w - 1.75, 1.5]])
    # outside the frame, inside the pad
    p.append([[-0.5, ym], [-half + 0.25, ym], [w + 0.5 * half, ym], [xm, -1.0], [xm, h + half - 0.5], [w - 0.01 + half, h - 0.01 + half],
              [-(half + 1.0), ym], [xm, -(half + 1.0)]])
    # on the first position past the pad, and beyond
    p.append([[w + half, ym], [xm, h + half], [-(half + 1.5), ym], [xm, -(half + 4.0)], [w + half + 7.25, ym], [3.0 * w, 2.0 * h]])
    pt = patches(h, w, case.win)
    if pt is not None:
        (fx, fy, s), (ex, ey, _) = pt
        c = (s - 1) / 2
        p.append([[fx + c, fy + c], [fx + c + 0.5, fy + c - 0.25], [fx + c - 1, fy + c + 1], [fx + c + 1, fy + c], [fx + c - 0.3, fy + c - 0.7]])
        e = ex + s // 2 - 0.5
        p.append([[e, ey + c], [e + 0.5, ey + c + 0.5], [e - 0.5, ey + c - 1], [e + 0.25, ey + c + 1], [e - 0.1, ey + c - 0.4]])
    out = np.concatenate([np.asarray(a, np.float64) for a in p]).astype(np.float32)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- reference
def ulp_apart(a, b):
    """distance of two float32 arrays in units in the last place"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


@functools.lru_cache(maxsize=None)
def reference(case):
    """the traced reference of a case (computed once, read-only) with ``stable`` bool [n]"""
    prev, cur = frames(case)
    pts = points(case)
    r = N.lk_traced(prev, cur, pts, **case.params)
    alt = N.lk_traced(prev, cur, pts, assoc=1, **case.params)
    same = (alt["status"] == r["status"]) & (ulp_apart(alt["next"], r["next"]).max(1) <= 1)
    near = N.lk_traced(prev, cur, pts, nudge=NUDGE_PX, **case.params)
    calm = (near["status"] == r["status"]) & (np.abs(near["next64"] - r["next64"]).max(1) <= NUDGE_GAIN * NUDGE_PX)
    r["stable"] = (r["margin"] >= MARGIN) & same & calm
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def compare(case, nxt, status):
    """-> (indices of stable points whose status differs, largest position deviation in px over the stable points)"""
    r = reference(case)
    st = r["stable"]
    bad = np.nonzero(st & (np.asarray(status, bool) != r["status"]))[0]
    dev = np.abs(np.asarray(nxt, np.float64) - r["next"].astype(np.float64)).max(1)
    return bad, float(dev[st].max()) if st.any() else 0.0
