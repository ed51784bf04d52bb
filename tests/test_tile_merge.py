"""The merge of a tiled predict's per-entry rows: the host twin of the kernel (ops.tile_merge with device=-1, the same per-frame
routine in host C++) against the sequential checker in tests/_tile_merge_numpy.py, bit for bit, on seeded random row sets with ties
and on hand cases.  No GPU."""
import numpy as np
import pytest

from cvsd_amd import ops
from cvsd_amd.ops import SENTINEL_BITS

import _tile_merge_numpy as T

F32 = np.float32


def run(rows, counts, origins, kdim=0, metric="ios", thr=0.5, device=-1):
    """ops.tile_merge against the checker, bit for bit: kept rows, counts, tile_idx, and untouched slots beyond the count"""
    rows = np.ascontiguousarray(rows, np.float32)
    counts = np.asarray(counts, np.int32).reshape(rows.shape[:2])
    origins = np.asarray(origins, np.int32).reshape(rows.shape[:2] + (2,))
    got, cnt, idx = ops.tile_merge(rows, counts, origins, kdim=kdim, metric=metric, thr=thr, device=device)
    want = T.merge(rows, counts, origins, kdim=kdim, metric=metric, thr=thr)
    for f, (wr, wi) in enumerate(want):
        assert cnt[f] == len(wr), (f, cnt[f], len(wr))
        assert np.array_equal(got[f, :cnt[f]].view(np.uint32), wr.view(np.uint32)), f
        assert np.array_equal(idx[f, :cnt[f]], wi), f
        assert (got[f, cnt[f]:].view(np.uint32) == SENTINEL_BITS).all() and (idx[f, cnt[f]:] == -1).all()
    return [w[0] for w in want], [w[1] for w in want]


def one_frame(entry_rows, max_det=4):
    """entry_rows = list (per entry) of lists of det rows -> rows [1, E, max_det, 58] with garbage beyond the counts, counts [1, E]"""
    E = len(entry_rows)
    rows = np.full((1, E, max_det, T.DET_WORDS), 12345.678, np.float32)
    counts = np.zeros((1, E), np.int32)
    for e, rs in enumerate(entry_rows):
        counts[0, e] = len(rs)
        for r, row in enumerate(rs):
            rows[0, e, r] = row
    return rows, counts


@pytest.mark.parametrize("metric", ["ios", "iou"])
@pytest.mark.parametrize("kdim", [0, 2, 3])
def test_random_rows_with_ties(metric, kdim):
    rng = np.random.default_rng(7 + kdim)
    F, E, md = 3, 5, 24
    counts = rng.integers(0, md + 1, (F, E))
    counts[1, 2] = 0
    counts[2] = [md, md, md, md, md]                              # full entries: more than max_det survive -> truncation
    rows = T.random_rows(rng, F, E, md, counts, extent=400.0 if metric == "iou" else 200.0, n_cls=2)
    origins = rng.integers(0, 300, (F, E, 2))
    kept, _ = run(rows, counts, origins, kdim=kdim, metric=metric, thr=0.5)
    assert any(0 < len(k) < c.sum() for k, c in zip(kept, counts))          # something was suppressed somewhere
    confs = np.concatenate([rows[f, e, :counts[f, e], 4] for f in range(F) for e in range(E)])
    assert len(np.unique(confs)) < len(confs)                     # the set does hold ties


def test_contained_box_ios_against_iou():
    a, b = T.det_row(0, 0, 10, 10, 0.9), T.det_row(2, 2, 6, 6, 0.8)         # IoU 16 / 100 = 0.16, IoS 16 / 16 = 1
    rows, counts = one_frame([[a], [b]])
    kept, idx = run(rows, counts, np.zeros((1, 2, 2)), metric="ios")
    assert len(kept[0]) == 1 and idx[0].tolist() == [0] and kept[0][0, 4] == F32(0.9)
    kept, idx = run(rows, counts, np.zeros((1, 2, 2)), metric="iou")
    assert len(kept[0]) == 2 and idx[0].tolist() == [0, 1]


def test_same_box_from_two_tiles_keeps_the_lower_entry():
    # the same frame box seen by the entry at (0, 0) and by the entry at (72, 0), equal conf: the stable order keeps entry 0's copy
    rows, counts = one_frame([[T.det_row(80, 10, 90, 30, 0.5, anchor=11)], [T.det_row(8, 10, 18, 30, 0.5, anchor=22)]])
    kept, idx = run(rows, counts, [[[0, 0], [72, 0]]])
    assert idx[0].tolist() == [0] and kept[0][0, 6:7].view(np.int32)[0] == 11
    # ... and inside one entry the lower row
    rows, counts = one_frame([[T.det_row(1, 1, 9, 9, 0.5, anchor=1), T.det_row(1, 1, 9, 9, 0.5, anchor=2)]])
    kept, idx = run(rows, counts, [[[5, 5]]])
    assert len(kept[0]) == 1 and kept[0][0, 6:7].view(np.int32)[0] == 1 and kept[0][0, :4].tolist() == [6, 6, 14, 14]


def test_different_classes_do_not_suppress():
    rows, counts = one_frame([[T.det_row(0, 0, 10, 10, 0.9, cls=0)], [T.det_row(0, 0, 10, 10, 0.8, cls=1)]])
    for metric in ("ios", "iou"):
        kept, idx = run(rows, counts, np.zeros((1, 2, 2)), metric=metric)
        assert idx[0].tolist() == [0, 1]


def test_zero_area_box_survives_and_suppresses_nothing():
    z = T.det_row(5, 5, 5, 9, 0.95)                                # zero width, inside the others
    rows, counts = one_frame([[z, T.det_row(0, 0, 10, 10, 0.9)], [T.det_row(5, 5, 5, 9, 0.85), T.det_row(4, 4, 6, 10, 0.8)]])
    for metric in ("ios", "iou"):
        kept, idx = run(rows, counts, np.zeros((1, 2, 2)), metric=metric, thr=0.0)
        # both zero-area rows live (0 / 0 is NaN under ios, 0 under iou: neither is > 0); the 2 x 6 box dies under both (IoS 1, IoU 0.12)
        assert idx[0].tolist() == [0, 0, 1], metric


def test_empty_entries():
    rows, counts = one_frame([[], [T.det_row(0, 0, 4, 4, 0.5)], []])
    kept, idx = run(rows, counts, [[[0, 0], [3, 4], [9, 9]]])
    assert idx[0].tolist() == [1] and kept[0][0, :4].tolist() == [3, 4, 7, 8]
    rows, counts = one_frame([[], [], []])
    kept, _ = run(rows, counts, np.zeros((1, 3, 2)))
    assert len(kept[0]) == 0
    # two frames, one of them empty
    r2 = np.concatenate([rows, one_frame([[T.det_row(0, 0, 4, 4, 0.5)], [], []])[0]])
    kept, _ = run(r2, [[0, 0, 0], [1, 0, 0]], np.zeros((2, 3, 2)))
    assert [len(k) for k in kept] == [0, 1]


def test_max_det_truncation():
    # 2 entries x 3 disjoint boxes, max_det 3: the three highest confidences, in order, whatever entry they came from
    e0 = [T.det_row(20 * i, 0, 20 * i + 10, 10, c) for i, c in enumerate((0.9, 0.6, 0.3))]
    e1 = [T.det_row(20 * i, 50, 20 * i + 10, 60, c) for i, c in enumerate((0.8, 0.7, 0.2))]
    rows, counts = one_frame([e0, e1], max_det=3)
    kept, idx = run(rows, counts, np.zeros((1, 2, 2)))
    assert kept[0][:, 4].tolist() == [F32(0.9), F32(0.8), F32(0.7)] and idx[0].tolist() == [0, 1, 1]


def test_keypoints_shift_and_pass_through():
    kp = np.arange(51, dtype=np.float32) + 0.25
    rows, counts = one_frame([[T.det_row(1, 2, 3, 4, 0.5, cls=3, anchor=77, kpt=kp)]])
    for kdim in (3, 2):
        kept, _ = run(rows, counts, [[[100, 1000]]], kdim=kdim)
        k = kept[0][0, 7:]
        groups = 51 // kdim
        want = kp.copy()
        want[0:groups * kdim:kdim] += 100
        want[1:groups * kdim:kdim] += 1000                        # conf (kdim 3) and what lies beyond the last whole group are untouched
        assert np.array_equal(k, want) and kept[0][0, :4].tolist() == [101, 1002, 103, 1004]
        assert kept[0][0, 5:7].view(np.int32).tolist() == [3, 77]
    kept, _ = run(rows, counts, [[[100, 1000]]], kdim=0)
    assert np.array_equal(kept[0][0, 7:], kp)                     # kdim 0: the columns are no keypoints


@pytest.mark.parametrize("metric", ["ios", "iou"])
def test_threshold_within_one_ulp(metric):
    """A pair whose metric m sits exactly at the threshold (thr = m: NOT greater, both live) and one ulp above it (thr = the float
    below m: the second dies).  For "iou" the pair is chosen so that contracting inter = w * h into `area_i + area_j - inter` changes m:
    a build that fuses them flips one of the two decisions (a fused m above m flips the first, below m the second)."""
    a, b, m, fused = T.threshold_pair(metric)
    assert metric == "ios" or fused != m
    rows, counts = one_frame([[T.det_row(*a, 0.9)], [T.det_row(*b, 0.8)]])
    kept, idx = run(rows, counts, np.zeros((1, 2, 2)), metric=metric, thr=float(m))
    assert idx[0].tolist() == [0, 1]
    kept, idx = run(rows, counts, np.zeros((1, 2, 2)), metric=metric, thr=float(np.nextafter(m, F32(0))))
    assert idx[0].tolist() == [0]


def test_refusals():
    rows, counts = one_frame([[T.det_row(0, 0, 1, 1, 0.5)]])
    org = np.zeros((1, 1, 2))
    with pytest.raises(ValueError, match="tile_metric"):
        ops.tile_merge(rows, counts, org, metric="giou", device=-1)
    with pytest.raises(ValueError, match="thr"):
        ops.tile_merge(rows, counts, org, thr=1.5, device=-1)
    with pytest.raises(ValueError, match="kdim"):
        ops.tile_merge(rows, counts, org, kdim=4, device=-1)
    with pytest.raises(ValueError, match="counts"):
        ops.tile_merge(rows, [[9]], org, device=-1)
    with pytest.raises(ValueError, match="entries"):
        ops.tile_merge(np.zeros((1, 65, 1, T.DET_WORDS), np.float32), np.zeros((1, 65)), np.zeros((1, 65, 2)), device=-1)
    with pytest.raises(ValueError, match="max_det"):
        ops.tile_merge(np.zeros((1, 1, 1025, T.DET_WORDS), np.float32), np.zeros((1, 1)), np.zeros((1, 1, 2)), device=-1)
