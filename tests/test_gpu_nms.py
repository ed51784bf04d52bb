"""The detector's tail alone (csrc/post_kernels.hip: candidate filter, LDS / hybrid / multi-launch sort, greedy suppression on 8
and on 16 waves, scale-back, rows, row compaction) through cvsd_amd.ops.postprocess, against oracle.yolo_oracle's
non_max_suppression + scale_boxes + scale_coords.  Every comparison is equality of bits.

Inputs, cases and reference: tests/_nms_cases.py (checked on the CPU by tests/test_nms_cases.py).  Which launches a run takes
follows from (n, A): A > 16384 the multi-launch sort, else n <= 16 the fused kernel, else nms_sort_kernel + nms_greedy_kernel."""
import functools

import numpy as np
import pytest

import _nms_cases as S

pytestmark = pytest.mark.gpu

WORDS = ("x1", "y1", "x2", "y2", "score", "class", "anchor")


def _post(c, n, **kw):
    from cvsd_amd import ops
    pred, _ = c.batch(n)
    args = dict(c.kwargs(), geom=c.geom(n), pack=c.pack)
    args.update(kw)
    return ops.postprocess(pred, **args)


@functools.lru_cache(maxsize=None)
def _run(name, n):
    """one call per (case, batch size), shared by the tests that look at its parts"""
    return _post(S.case(name), n)


def _expected(c, n):
    from cvsd_amd import ops
    return c.expected_rows(n, ops.SENTINEL_BITS)


def _check_rows(c, n, r, what):
    want, counts = _expected(c, n)
    assert r.rows.shape == want.shape and r.rows.dtype == np.uint32
    np.testing.assert_array_equal(r.counts, counts, err_msg=f"{what}: kept rows per frame")
    order = c.order(n)
    for i in range(n):                                   # the kept anchors and their order first: the readable failure
        k = counts[i]
        got, ref = r.rows[i, :k, 6].astype(np.int64), c.ref()[order[i]][1]
        assert list(got) == list(ref), f"{what}: frame {i} (pool frame {order[i]}): kept anchors differ from the oracle's"
    bad = np.argwhere(r.rows != want)
    if len(bad):
        i, k, q = bad[0]
        word = WORDS[q] if q < 7 else f"kpt[{q - 7}]"
        slot = "a kept row" if k < counts[i] else "a slot beyond count (must keep the sentinel)"
        pytest.fail(f"{what}: {len(bad)} words differ, first at frame {i} slot {k} word {q} ({word}, {slot}): "
                    f"got {r.rows[i, k, q]:#010x} ({r.rows[i, k, q:q + 1].view(np.float32)[0]!r}), "
                    f"want {want[i, k, q]:#010x} ({want[i, k, q:q + 1].view(np.float32)[0]!r})")


def _check_packed(c, n, r, what):
    from cvsd_amd import ops
    want, counts = _expected(c, n)
    scan = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    np.testing.assert_array_equal(r.offsets, scan, err_msg=f"{what}: offsets are the exclusive scan of the counts")
    assert r.total == int(counts.sum()) == int(r.offsets[n])
    cat = np.concatenate([want[i, :counts[i]] for i in range(n)])
    assert r.packed.shape == (n * c.max_det, S.ROW_WORDS)
    np.testing.assert_array_equal(r.packed[:r.total], cat, err_msg=f"{what}: packed rows = the slot rows in frame order")
    assert (r.packed[r.total:] == ops.SENTINEL_BITS).all(), f"{what}: a packed row beyond total was written"


@pytest.mark.parametrize("name,n", S.RUNS, ids=[f"{k}-n{n}" for k, n in S.RUNS])
def test_rows_counts_and_untouched_slots_equal_the_oracle(name, n):
    """kept anchors, their order and the counts; the 58 words of every kept row (box, score, class as int, anchor, keypoints, zeros
    behind them); every slot beyond count still the sentinel; with pack, the packed rows, the offsets and the total"""
    c, r = S.case(name), _run(name, n)
    _check_rows(c, n, r, f"{name}, n = {n}")
    if c.pack:
        _check_packed(c, n, r, f"{name}, n = {n}")


@pytest.mark.parametrize("A", sorted(S.PATH_POOLS))
def test_a_frame_does_not_depend_on_the_batch_or_the_launch_path(A):
    """the fullest frame alone (n = 1, fused), as frame 0 of 16 (fused), of 17 (sort + greedy on 8 waves) and of 33"""
    name = f"paths_{A}"
    one = _run(name, 1)
    assert one.counts[0] > 200
    for n in (16, 17, 33):
        r = _run(name, n)
        assert r.counts[0] == one.counts[0]
        np.testing.assert_array_equal(r.rows[0], one.rows[0], err_msg=f"{name}: frame 0 of {n} against the frame alone")
        np.testing.assert_array_equal(r.rows[len(S.case(name).pool)], one.rows[0])       # and where the pool comes round again


@pytest.mark.parametrize("name,n", [("paths_5000", 17), ("paths_16385", 1), ("sole", 16), ("scale_table", 17), ("compact", 1025)])
def test_the_same_call_twice_gives_the_same_bits(name, n):
    a, b = _run(name, n), _post(S.case(name), n)
    np.testing.assert_array_equal(a.rows, b.rows)
    np.testing.assert_array_equal(a.counts, b.counts)
    if a.packed is not None:
        np.testing.assert_array_equal(a.packed, b.packed)
        np.testing.assert_array_equal(a.offsets, b.offsets)


@pytest.mark.parametrize("name,n", [("thresholds", 1), ("thresholds", 17), ("classes_70", 17), ("paths_2048", 16), ("scale_pose51", 4)])
def test_a_best_of_the_caller_gives_the_rows_of_the_computed_one(name, n):
    """best [n, A, 2] = (max class score, first argmax) stated in numpy and handed in, against launch_best_from_pred's"""
    c = S.case(name)
    pred, _ = c.batch(n)
    cls = pred[:, 4:4 + c.nc]
    best = np.stack([cls.max(1), cls.argmax(1).astype(np.float32)], -1)
    r = _post(c, n, best=best)
    _check_rows(c, n, r, f"{name}, n = {n}, best of the caller")
    np.testing.assert_array_equal(r.rows, _run(name, n).rows)


@pytest.mark.parametrize("name", ["scale_pose51", "scale_pose34_gain2", "scale_kpt4", "scale_detect"])
@pytest.mark.parametrize("n", [4, 17])
def test_a_scalar_geometry_and_the_same_one_per_frame_give_the_same_bits(name, n):
    c = S.case(name)
    scalar = _run(name, n)
    table = _post(c, n, geom=c.geom(n, as_table=True))
    assert c.geom(n).shape == (7,) and c.geom(n, as_table=True).shape == (n, 7)
    _check_rows(c, n, table, f"{name}, n = {n}, geometry as [n, 7]")
    np.testing.assert_array_equal(scalar.rows, table.rows)


@pytest.mark.parametrize("name,n", [("paths_2048", 17), ("scale_table", 4), ("maxdet_dups_1024", 1), ("classes_none", 17)])
def test_packed_rows_are_the_slot_rows_in_frame_order(name, n):
    """compaction behind cases with empty frames, full frames (count = max_det) and keypoints"""
    c = S.case(name)
    r = _post(c, n, pack=True)
    _check_rows(c, n, r, f"{name}, n = {n}, pack")
    _check_packed(c, n, r, f"{name}, n = {n}, pack")


def test_a_refused_call_leaves_the_next_one_alone():
    from cvsd_amd import ops
    c = S.case("thresholds")
    pred, _ = c.batch(1)
    with pytest.raises(ValueError, match="max_det"):
        ops.postprocess(pred, **dict(c.kwargs(), max_det=1025))
    _check_rows(c, 1, _post(c, 1), "thresholds after a refusal")
