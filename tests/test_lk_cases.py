"""The Lucas-Kanade case table (tests/_lk_cases.py) on the CPU: the traced reference is the committed numpy statement bit for bit, the
table reaches what it claims to reach -- every exit, the region refill, every per-lane count, on STABLE points -- and the product's
host C++ (csrc/gmc_host.cpp) meets the reference on every stable point.  tests/test_gpu_lk.py holds the HIP kernel to the same
reference."""
import numpy as np
import pytest

import _lk_cases as S
import _lk_numpy as N
from cvsd_amd import gmc
from oracle import gmc_oracle as G

IDS = [c.name for c in S.CASES]


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_traced_reference_is_the_committed_numpy_statement_bit_for_bit(case):
    prev, cur = S.frames(case)
    r = S.reference(case)
    nxt, status = G.calc_optical_flow_pyr_lk(prev, cur, S.points(case), **case.params)
    assert nxt.dtype == r["next"].dtype and np.array_equal(nxt, r["next"]) and np.array_equal(status, r["status"])
    # the trace is complete and consistent with the status it explains
    kept = np.isin(r["exit"], (N.CONVERGED, N.OSCILLATION, N.MAX_ITERS))
    assert (r["exit"] >= 0).all() and np.array_equal(kept, r["status"])
    assert (r["iters"][np.isin(r["exit"], (N.START_OUTSIDE, N.REJECTED))] == 0).all() and (r["iters"] <= case.max_iters).all()
    assert (r["iters"][r["exit"] == N.MAX_ITERS] == case.max_iters).all()


def test_reassociated_sums_are_another_rounding_of_the_same_algorithm():
    """the probe is not a no-op: float64 positions differ in their last bits on some stable points (a step's rounding noise, ~1e-16 px,
    mostly vanishes below the ulp of the position it is added to), and by no more than last bits"""
    case = S.CASES[IDS.index("win21-sim")]
    prev, cur = S.frames(case)
    r = S.reference(case)
    alt = N.lk_traced(prev, cur, S.points(case), assoc=1, **case.params)
    st = r["stable"] & (r["iters"] > 0)
    d = np.abs(alt["next64"] - r["next64"]).max(1)[st]
    assert (d > 0).sum() >= 5 and d.max() < 1e-9


def test_table_reaches_every_exit_window_and_the_refill_on_stable_points():
    n = unstable = 0
    exits = np.zeros(len(N.EXIT_NAMES), np.int64)
    refills = skips = 0
    for case in S.CASES:
        r = S.reference(case)
        st = r["stable"]
        share = 1.0 - st.mean()
        assert share <= 0.05, (case.name, share)
        n += len(st); unstable += int((~st).sum())
        exits += np.bincount(r["exit"][st], minlength=len(exits))
        refills += int((r["walk"][st] > 3).sum())
        skips += int((r["skipped"] & r["status"] & st).sum())
        # the float32 quantum behind D_HOST_PX: every stable point that moved stays below COORD_MAX_PX
        moved = st & (r["next"] != S.points(case)).any(1)
        assert np.abs(r["next"][moved]).max(initial=0.0) < S.COORD_MAX_PX, case.name
    print(f"points {n}, unstable {unstable} ({unstable / n:.2%}); exits on stable points {dict(zip(N.EXIT_NAMES, exits.tolist()))}; walk > 3 px: {refills}; "
          f"rejected above level 0 and kept: {skips}")
    assert unstable <= 0.01 * n
    assert (exits >= 20).all(), dict(zip(N.EXIT_NAMES, exits.tolist()))
    assert refills >= 20
    assert skips >= 20
    assert {S.per_lane(c.win) for c in S.CASES} == set(range(1, 8))
    assert {c.win for c in S.CASES if c.levels == 3} >= set(range(3, 23, 2))
    for win in (5, 21):
        assert {c.levels for c in S.CASES if c.win == win} >= {0, 1, 2, 3, 5}
    assert {(c.max_iters, c.eps, c.min_eig) for c in S.CASES} >= {(i, e, m) for i in (1, 30) for e in (0.0, 0.01, 0.5) for m in (1e-4, 1e-2)}
    shapes = {c.shape for c in S.CASES}
    assert {(97, 131), (64, 80), (22, 22), (5, 64), (75, 101)} <= shapes
    # the plane of the window's size has no pyramid level, whatever is asked
    assert S.reference(S.CASES[IDS.index("win21-22x22")])["top"] == 0
    # a pyramid of every depth 0 .. 4 is walked
    assert {S.reference(c)["top"] for c in S.CASES} >= {0, 1, 2, 3, 4}


def test_planted_points_take_the_exits_they_were_planted_for():
    case = S.CASES[IDS.index("win9-sub")]
    r = S.reference(case)
    pts = S.points(case)
    h, w = case.shape
    half = case.win // 2
    (fx, fy, s), (ex, ey, _) = S.patches(h, w, case.win)
    flat = (np.abs(pts[:, 0] - (fx + (s - 1) / 2)) <= 1) & (np.abs(pts[:, 1] - (fy + (s - 1) / 2)) <= 1)
    edge = (np.abs(pts[:, 0] - (ex + s // 2 - 0.5)) <= 0.5) & (np.abs(pts[:, 1] - (ey + (s - 1) / 2)) <= 1)
    assert flat.sum() == 5 and edge.sum() == 5
    assert (r["exit"][flat | edge] == N.REJECTED).all() and r["stable"][flat | edge].all()
    beyond = (pts[:, 0] < -(half + 1)) | (pts[:, 0] >= w + half) | (pts[:, 1] < -(half + 1)) | (pts[:, 1] >= h + half)
    assert beyond.sum() == 6 and (r["exit"][beyond] == N.START_OUTSIDE).all() and (r["exit"][~beyond] != N.START_OUTSIDE).all()
    # start tests are exact: a point on the pad's first and on its last-but-one position is decided, and stable
    on_end = ((pts[:, 0] == -(half + 1.0)) | (pts[:, 1] == -(half + 1.0)) | (pts[:, 0] == w + half) | (pts[:, 1] == h + half)) & (pts[:, 0] < 2 * w)
    assert on_end.sum() == 4 and (on_end & beyond).sum() == 2 and r["stable"][on_end].all()
    # zero motion: every kept point converges in one iteration on a zero difference patch -- no decision carries a margin below 0.1
    z = S.reference(S.CASES[IDS.index("win9-zero")])
    assert (z["iters"][z["status"]] == 1).all() and np.array_equal(z["next"][z["status"]], S.points(S.CASES[IDS.index("win9-zero")])[z["status"]])
    assert z["stable"].all()


def test_host_routine_meets_the_reference_on_every_stable_point():
    """csrc/gmc_host.cpp (device=None): the same status on every stable point, positions within D_HOST_PX.  Prints the measured
    deviation that tests/_lk_cases.py records as D_HOST_MEASURED_PX."""
    worst, compared = 0.0, 0
    for case in S.CASES:
        prev, cur = S.frames(case)
        nxt, status = gmc.calc_optical_flow_pyr_lk(prev, cur, S.points(case), device=None, **case.params)
        bad, dev = S.compare(case, nxt, status)
        assert len(bad) == 0, (case.name, bad.tolist())
        assert dev <= S.D_HOST_PX, (case.name, dev)
        worst = max(worst, dev)
        compared += int(S.reference(case)["stable"].sum())
    print(f"host C++ against the float64 reference on {compared} stable points: D_host = {worst:.3g} px (recorded {S.D_HOST_MEASURED_PX:.3g}, "
          f"taken as {S.D_HOST_PX:.3g}), LK_TOL_PX = {S.LK_TOL_PX:.3g}")
    assert worst <= S.D_HOST_PX < S.LK_TOL_PX <= 1e-4


def test_host_routine_builds_the_pyramid_as_deep_as_the_plane_allows():
    """1300 x 1700 at win=3: levels=10 tracks from a ninth plane (6 x 7) on the host, as the numpy statement does -- the depth the device
    routine refuses (tests/test_gpu_lk.py) -- and that is another answer than levels=7 gives"""
    case, deep = S.DEEP, S.DEEP_REFUSED
    prev, cur = S.frames(case)
    pts = S.points(case)
    assert S.reference(deep)["top"] == 8 and S.reference(case)["top"] == 7
    assert np.abs(S.reference(deep)["next64"] - S.reference(case)["next64"]).max() > 1.0
    for c in (deep, case):
        nxt, status = gmc.calc_optical_flow_pyr_lk(prev, cur, pts, device=None, **c.params)
        bad, dev = S.compare(c, nxt, status)
        assert len(bad) == 0 and dev <= S.D_HOST_PX and S.reference(c)["stable"].sum() >= 10, (c.name, bad, dev)
