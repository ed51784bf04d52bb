"""Lucas-Kanade on the GPU (csrc/gmc_kernels.hip: lk_kernel, one wavefront per point) against the traced float64 reference, per point:
every case of tests/_lk_cases.py -- every window 3 .. 21 (1 .. 7 window pixels per lane, a region side and a box size each), every
pyramid depth, the loop's parameters, sub-pixel motion, a similarity, motion that walks out of the region's margin and motion
beyond reach, planes of the window's size, thin and odd ones, points on and over every border.  On every STABLE point (the rule is in
tests/_lk_cases.py; tests/test_lk_cases.py caps the rest at 1 %) the status is the reference's and the position lies within LK_TOL_PX
-- the dropped points too: the kernel writes their last position.  tests/test_gpu_gmc.py keeps its own, statistical, comparison."""
import numpy as np
import pytest

import _lk_cases as S
from cvsd_amd import gmc

pytestmark = pytest.mark.gpu

_worst = {}          # window -> largest deviation seen so far in this session


def _meets_the_reference(case, nxt, status):
    r = S.reference(case)
    bad, dev = S.compare(case, nxt, status)
    _worst[case.win] = max(_worst.get(case.win, 0.0), dev)
    print(f"{case.name}: {int(r['stable'].sum())} stable points of {len(status)}, max |gpu - reference| = {dev:.3g} px; "
          f"largest so far at win={case.win}: {_worst[case.win]:.3g} px (LK_TOL_PX = {S.LK_TOL_PX:.3g})")
    assert len(bad) == 0, (case.name, bad.tolist(), r["exit"][bad].tolist(), r["status"][bad].tolist())
    assert dev <= S.LK_TOL_PX, (case.name, dev)


@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_device_lucas_kanade_meets_the_traced_reference_on_every_stable_point(case):
    prev, cur = S.frames(case)
    pts = S.points(case)
    nxt, status = gmc.calc_optical_flow_pyr_lk(prev, cur, pts, device=0, **case.params)
    assert np.isfinite(nxt).all()
    _meets_the_reference(case, nxt, status)
    # the same call again: the same bits
    nxt2, status2 = gmc.calc_optical_flow_pyr_lk(prev, cur, pts, device=0, **case.params)
    assert np.array_equal(nxt2, nxt) and np.array_equal(status2, status)
    # a point's result does not depend on the points it is launched with: a prefix that ends inside a block of four wavefronts
    k = 37
    assert k % S.WAVES_PER_BLOCK and k < len(pts)
    nxt3, status3 = gmc.calc_optical_flow_pyr_lk(prev, cur, pts[:k], device=0, **case.params)
    assert np.array_equal(nxt3, nxt[:k]) and np.array_equal(status3, status[:k])


def test_device_routine_refuses_a_pyramid_deeper_than_it_holds():
    """1300 x 1700 at win=3 allows eight levels above the plane; the device pyramid holds eight planes.  levels=10 is refused (the host
    routine tracks it from the ninth plane: tests/test_lk_cases.py), levels=7 fills the pyramid and meets the reference."""
    case, deep = S.DEEP, S.DEEP_REFUSED
    prev, cur = S.frames(case)
    pts = S.points(case)
    with pytest.raises(ValueError):
        gmc.calc_optical_flow_pyr_lk(prev, cur, pts, device=0, **deep.params)
    with pytest.raises(ValueError):
        gmc.calc_optical_flow_pyr_lk(prev, cur, pts, device=0, **dict(deep.params, levels=8))
    assert S.reference(case)["top"] == 7
    nxt, status = gmc.calc_optical_flow_pyr_lk(prev, cur, pts, device=0, **case.params)
    _meets_the_reference(case, nxt, status)
    assert S.reference(case)["stable"].sum() >= 10
    # where the plane stops the pyramid first, any levels is accepted: 97 x 131 at win=21 has two levels above it
    small = next(c for c in S.CASES if c.name == "win21-sim")
    assert S.reference(small)["top"] == 2
    p2, c2 = S.frames(small)
    a = gmc.calc_optical_flow_pyr_lk(p2, c2, S.points(small), device=0, **dict(small.params, levels=3))
    b = gmc.calc_optical_flow_pyr_lk(p2, c2, S.points(small), device=0, **dict(small.params, levels=1000))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
