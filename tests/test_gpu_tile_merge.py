"""The tile-merge kernel (csrc/post_kernels.hip: tile_merge_kernel, one block per source frame) through ops.tile_merge on the device,
against the sequential checker in tests/_tile_merge_numpy.py, bit for bit: the LDS sort, the hybrid LDS / global sort past 4096 keys,
one entry, empty frames, two frames with different counts in one launch, both metrics, pose and detect row forms.  Row sets come in
two densities: `dense` boxes suppress each other heavily, so the greedy pass walks every candidate and keeps fewer than max_det;
`sparse` ones fill max_det early and the pass stops there."""
import numpy as np
import pytest

from cvsd_amd import ops
from cvsd_amd.ops import SENTINEL_BITS

import _tile_merge_numpy as T

pytestmark = pytest.mark.gpu

DENSE = dict(extent=200.0, size_frac=0.9, omax=50)
SPARSE = dict(extent=1500.0, size_frac=0.3, omax=1500)
# metric -> threshold at which the dense sets keep fewer than max_det rows (measured on the checker: 117 / 117 of 2,086 candidates)
DENSE_THR = {"ios": 0.5, "iou": 0.1}


def check(rows, counts, origins, kdim, metric, thr=0.5):
    got, cnt, idx = ops.tile_merge(rows, counts, origins, kdim=kdim, metric=metric, thr=thr, device=0)
    host = ops.tile_merge(rows, counts, origins, kdim=kdim, metric=metric, thr=thr, device=-1)
    want = T.merge(rows, counts, origins, kdim=kdim, metric=metric, thr=thr)
    for f, (wr, wi) in enumerate(want):
        assert cnt[f] == len(wr), (f, cnt[f], len(wr))
        assert np.array_equal(got[f, :cnt[f]].view(np.uint32), wr.view(np.uint32)), f
        assert np.array_equal(idx[f, :cnt[f]], wi), f
        assert (got[f, cnt[f]:].view(np.uint32) == SENTINEL_BITS).all() and (idx[f, cnt[f]:] == -1).all()
    assert np.array_equal(got.view(np.uint32), host[0].view(np.uint32))          # ... and the host twin gives the kernel's bits
    assert np.array_equal(cnt, host[1]) and np.array_equal(idx, host[2])
    return cnt


def rows_for(seed, F, E, md, counts, kpt, extent, size_frac, omax):
    rng = np.random.default_rng(seed)
    rows = T.random_rows(rng, F, E, md, counts, extent=extent, n_cls=2, kpt=kpt, size_frac=size_frac)
    origins = rng.integers(0, omax, (F, E, 2)).astype(np.int32)
    return rows, origins


@pytest.mark.parametrize("metric", ["ios", "iou"])
@pytest.mark.parametrize("kdim", [3, 0])
def test_seven_entries_lds_sort(metric, kdim):
    """7 x 300 rows, 2,086 candidates: the keys are sorted in LDS"""
    counts = np.array([[300, 300, 287, 300, 1, 300, 299]], np.int32)
    rows, origins = rows_for(1, 1, 7, 300, counts, kdim == 3, **DENSE)
    cnt = check(rows, counts, origins, kdim, metric, DENSE_THR[metric])
    assert 0 < cnt[0] < 300                                       # every candidate was walked
    rows, origins = rows_for(1, 1, 7, 300, counts, kdim == 3, **SPARSE)
    assert check(rows, counts, origins, kdim, metric)[0] == 300   # the merge stopped at max_det


@pytest.mark.parametrize("metric,kdim", [("ios", 3), ("iou", 0)])
def test_fifteen_entries_hybrid_sort(metric, kdim):
    """15 x 300 = 4,500 keys, past the 4,096 that fit in LDS: the hybrid sort on the padded 8,192-key sequence"""
    counts = np.full((1, 15), 300, np.int32)
    rows, origins = rows_for(2, 1, 15, 300, counts, kdim == 3, **DENSE)
    cnt = check(rows, counts, origins, kdim, metric, DENSE_THR[metric])
    assert 0 < cnt[0] < 300
    rows, origins = rows_for(2, 1, 15, 300, counts, kdim == 3, **SPARSE)
    assert check(rows, counts, origins, kdim, metric)[0] == 300


def test_hybrid_capacity_but_few_rows():
    """sized for the hybrid form (15 x 300) but 4,096 and 4,097 candidates present: either side of the LDS limit, in one launch"""
    counts = np.zeros((2, 15), np.int32)
    counts[0, :13] = 300; counts[0, 13] = 196                     # 4,096
    counts[1, :13] = 300; counts[1, 13] = 196; counts[1, 14] = 1  # 4,097
    rows, origins = rows_for(3, 2, 15, 300, counts, False, **DENSE)
    check(rows, counts, origins, 0, "ios")


def test_one_entry_and_empty_frames():
    counts = np.array([[17]], np.int32)
    rows, origins = rows_for(4, 1, 1, 32, counts, True, **DENSE)
    check(rows, counts, origins, 3, "ios")
    counts = np.zeros((2, 3), np.int32)
    rows, origins = rows_for(5, 2, 3, 16, counts, True, **DENSE)
    cnt = check(rows, counts, origins, 3, "ios")
    assert cnt.tolist() == [0, 0]


@pytest.mark.parametrize("metric", ["ios", "iou"])
def test_two_frames_different_counts(metric):
    counts = np.array([[40, 0, 13, 64, 7], [0, 0, 64, 1, 0]], np.int32)
    rows, origins = rows_for(6, 2, 5, 64, counts, True, **DENSE)
    cnt = check(rows, counts, origins, 3, metric, DENSE_THR[metric])
    assert cnt[0] != cnt[1]


def test_kdim_two_and_ties_across_entries():
    """the same rows in every entry at the same origin: every tie goes to the lowest entry, all others die"""
    counts = np.full((1, 4), 20, np.int32)
    rows, origins = rows_for(7, 1, 1, 20, counts[:, :1], True, **DENSE)
    rows = np.repeat(rows, 4, axis=1)
    origins = np.repeat(origins, 4, axis=1)
    _, cnt, idx = ops.tile_merge(rows, counts, origins, kdim=2, metric="ios", thr=0.5, device=0)
    check(rows, counts, origins, 2, "ios")
    assert cnt[0] > 0 and (idx[0, :cnt[0]] == 0).all()


@pytest.mark.parametrize("metric", ["ios", "iou"])
def test_threshold_within_one_ulp(metric):
    """the pair of tests/test_tile_merge.py on the kernel: thr = m keeps both, thr = the float below m kills the second; for "iou" the
    pair's m changes when inter = w * h is contracted into the subtraction"""
    a, b, m, _ = T.threshold_pair(metric)
    rows = np.zeros((1, 2, 2, T.DET_WORDS), np.float32)
    rows[0, 0, 0], rows[0, 1, 0] = T.det_row(*a, 0.9), T.det_row(*b, 0.8)
    counts, origins = np.ones((1, 2), np.int32), np.zeros((1, 2, 2), np.int32)
    assert check(rows, counts, origins, 0, metric, float(m))[0] == 2
    assert check(rows, counts, origins, 0, metric, float(np.nextafter(m, np.float32(0))))[0] == 1
