"""CPU side of tests/test_gpu_nms.py: a census of the planted edges (a later edit of a builder must not be able to drop one
silently), the proof that the inputs tell the oracle from eleven wrong variants of the detector's tail, and the refusals of
ops.postprocess / mi355_op_nms_ex that need no GPU.  Cases and reference: tests/_nms_cases.py."""
import numpy as np
import pytest

import _nms_cases as S

F32 = np.float32


def _bits(v):
    return np.asarray(v, F32).view(np.uint32)


def _walk(c, f=0, **kw):
    """the restated walk of pool frame f: sorted anchors, offset boxes, areas, positions of every kept candidate"""
    t = {}
    args = dict(c.kwargs(), hw=None if c.hw is None else c.hw[f if c.table else 0])
    args.update(kw)
    S.restate(c.pool[f], trace=t, **args)
    return t


def _launch_path(n, A):
    return "multi" if A > 16384 else "fused" if n <= 16 else "pair"


def test_every_launch_path_and_sort_has_runs():
    seen = {(_launch_path(n, S.case(name).A) if name.startswith(("paths", "order", "trunc")) else None) for name, n in S.RUNS}
    assert {"multi", "fused", "pair"} <= seen
    assert set(S.NS) == {1, 16, 17, 33} and set(S.PATH_POOLS) == {2048, 5000, 16384, 16385}
    for A in S.PATH_POOLS:
        assert [(f"paths_{A}", n) in S.RUNS for n in S.NS] == [True] * 4
    # every case is small: one frame at most 16385 anchors, pools of a few frames
    assert all(S.case(k).A <= 16385 and len(S.case(k).pool) <= 9 for k in S.CASES)


def test_census_candidate_counts_per_frame():
    for A, counts in S.PATH_POOLS.items():
        c = S.case(f"paths_{A}")
        got = [len(S.sorted_candidates(p, c.nc, c.conf)[0]) for p in c.pool]
        assert tuple(got) == counts and 0 in got and len(set(got)) == len(got)
        # the sort each count selects: LDS up to 4096 keys, hybrid above (one block), multi-launch for A > 16384
    assert {0, 1, 63, 64, 65, 2048} == set(S.PATH_POOLS[2048])
    assert {4097, 5000} <= set(S.PATH_POOLS[5000]) and 8192 < 9000 <= 16384 and 9000 in S.PATH_POOLS[16384]
    assert {0, 100, 4096, 4097, 16385} == set(S.PATH_POOLS[16385])
    # a batch of 16 and of 17 hold frames of different counts, the empty one among them
    for A in S.PATH_POOLS:
        c = S.case(f"paths_{A}")
        assert len(set(c.order(16))) == len(c.pool) and c.order(1)[0] == 0 and S.PATH_POOLS[A][0] == max(S.PATH_POOLS[A])


@pytest.mark.parametrize("A", sorted(S.TIES))
def test_census_tie_blocks_span_the_boundaries_and_ascending_anchors_win(A):
    c = S.case(f"order_{A}")
    an, score, _ = S.sorted_candidates(c.pool[0], c.nc, c.conf)
    kept = list(c.ref()[0][1])
    blocks = S.TIES[A]
    assert any(a < 64 < b for a, b in blocks)
    assert any(a < 4096 < b for a, b in blocks) or A == 2048
    for a, b in blocks:
        assert len(set(_bits(score[a:b]))) == 1 and score[a - 1] > score[a] > score[b]
        blk = an[a:b]
        assert (np.diff(blk) > 0).all()
        placed = c.notes["ranked"][a:b]                                  # the order the builder wrote them in: not sorted
        assert sorted(placed) == list(blk) and list(placed) != list(blk) and list(placed) != list(blk[::-1])
        pos = [kept.index(x) for x in blk]                               # every one is kept, in ascending anchor order
        assert pos == list(range(pos[0], pos[0] + len(blk)))


@pytest.mark.parametrize("A", sorted(S.TRUNC))
@pytest.mark.parametrize("max_nms", [64, 1000, 4096])
def test_census_truncation_cuts_a_box_that_would_have_been_kept(A, max_nms):
    c = S.case(f"trunc_{A}_{max_nms}")
    an, score, _ = S.sorted_candidates(c.pool[0], c.nc, c.conf)              # uncut
    assert len(an) == S.TRUNC[A] and len(np.unique(score)) == len(score)    # distinct: the oracle's argsort at the cut is not stable
    kept = set(c.ref()[0][1])
    uncut = set(S.restate(c.pool[0], **dict(c.kwargs(), max_nms=30000))[1])
    if max_nms < len(an):
        assert an[max_nms - 1] in kept and an[max_nms] not in kept and an[max_nms] in uncut
    else:
        assert kept == uncut                                                 # fewer candidates than max_nms: nothing is cut


def test_census_sole_suppressors_cover_every_wave_and_chains_hold():
    c = S.case("sole")
    t = _walk(c)
    b, area, kept = t["b"], t["area"], t["kept_all"]
    thr = F32(c.iou)
    assert list(kept[:48]) == list(range(48)) and len(kept) == 62
    residues = set()
    for v in range(240, 288):
        before = kept[kept < v]
        hits = before[S.iou_row(b, area, v, before) > thr]
        assert len(hits) == 1 and v not in kept
        k = int(np.nonzero(kept == hits[0])[0][0])                            # index among the kept boxes: k mod waves picks the wave
        assert v // 64 >= hits[0] // 64 + 2
        residues.add(k)
    assert {k % 16 for k in residues} == set(range(16)) and {k % 8 for k in residues} == set(range(8)) and len(residues) >= 32
    for (ra, rb, rc), same_chunk in (((300, 301, 302), True), ((303, 330, 400), False)):
        assert ra in kept and rb not in kept and rc in kept
        assert S.iou_row(b, area, ra, [rb])[0] > thr and S.iou_row(b, area, rb, [rc])[0] > thr and not S.iou_row(b, area, ra, [rc])[0] > thr
        assert (len({ra // 64, rb // 64, rc // 64}) == 1) == same_chunk and (same_chunk or len({ra // 64, rb // 64, rc // 64}) == 3)
    assert set(range(410, 420)) <= set(kept)


def test_census_max_det_is_reached_mid_chunk_and_at_a_chunk_end():
    where = {}
    for kind in ("plain", "dups"):
        for m in S.MAX_DETS:
            c = S.case(f"maxdet_{kind}_{m}")
            kept = _walk(c)["kept_all"]
            assert len(kept) == 1100 > m and len(c.ref()[0][1]) == m               # live candidates are left over
            where[kind, m] = (kept[m - 1] + 1) % 64                                # 0: the last kept box closes its chunk
    assert where["plain", 64] == 0 and where["plain", 1024] == 0
    assert all(where["dups", m] != 0 for m in (7, 64, 300, 1024)) and where["plain", 7] != 0 and where["plain", 300] != 0


def test_census_thresholds():
    c = S.case("thresholds")
    p, plan = c.pool[0], c.notes["plan"]
    t = _walk(c)
    rank = {name: int(np.nonzero(t["an"] == a)[0][0]) if a in t["an"] else None for name, a in plan.items()}
    kept = set(c.ref()[0][1])
    b, area = t["b"], t["area"]
    iou = lambda x, y: S.iou_row(b, area, rank[x], [rank[y]])[0]
    assert c.iou == 0.5
    for x, y in (("exact_a", "exact_b"), ("exact1_a", "exact1_b")):
        assert _bits(iou(x, y)) == _bits(0.5) and plan[x] in kept and plan[y] in kept
    assert iou("close_a", "close_b") > F32(0.5) and plan["close_a"] in kept and plan["close_b"] not in kept
    assert _bits(p[4, plan["at_conf"]]) == _bits(c.conf) and rank["at_conf"] is None and plan["at_conf"] not in kept
    assert _bits(p[4, plan["above_conf"]]) == _bits(c.conf) + 1 and plan["above_conf"] in kept
    assert (p[:4, plan["two_cls_a"]] == p[:4, plan["two_cls_b"]]).all() and {plan["two_cls_a"], plan["two_cls_b"]} <= kept
    assert (p[:4, plan["one_cls_a"]] == p[:4, plan["one_cls_b"]]).all() and plan["one_cls_a"] in kept and plan["one_cls_b"] not in kept
    for x, y in (("zero_a", "zero_b"), ("flat_a", "flat_b")):
        assert area[rank[x]] == 0 and np.isnan(iou(x, y)) and {plan[x], plan[y]} <= kept
    assert np.isfinite(p).all()


def test_census_class_filter():
    c = S.case("classes_70")
    rows = c.ref()[0][0]
    assert c.nc == 70 and sorted(rows[:, 5].tolist()) == [0, 0, 31, 31, 32, 32, 69, 69]          # bits 0 and 31 of word 0, 0 of word 1, 5 of word 2
    c80 = S.case("classes_80")
    assert c80.nc == 80 and sorted(c80.ref()[0][0][:, 5].tolist()) == [31, 31, 32, 32, 79, 79]
    e = S.case("classes_none")
    assert len(e.ref()[0][1]) == 0 and len(S.sorted_candidates(e.pool[0], e.nc, e.conf)[0]) == 2 * 69


def test_census_scale_back():
    g0, g1 = S.geom7(*S.GEOMS[0]), S.geom7(*S.GEOMS[1])
    assert g0[2] == 107 and g0[2] != g0[4] and abs(float(g0[4]) - 106.88) < 1e-4           # rounded box pad, unrounded keypoint pad
    assert g1[0] > 2 and S.geom7(*S.GEOMS[2])[0] < 0.5 and S.geom7(*S.GEOMS[3])[1] != S.geom7(*S.GEOMS[3])[3]
    assert len(set(S.case("scale_table").hw)) >= 3 and S.case("scale_table").table
    kinds = {(S.case(k).extra, S.case(k).kdim) for k in S.CASES if k.startswith("scale_")}
    assert {(51, 3), (34, 2), (4, 2), (4, 0), (0, 0)} <= kinds
    for name in [k for k in S.CASES if k.startswith("scale_")]:
        c = S.case(name)
        for f, (rows, idx) in enumerate(c.ref()):
            hw = c.hw[f if c.table else 0]
            gain, pad_x, pad_y, kpad_x, kpad_y, ow, oh = S.geom7(*hw)
            box = rows[:, :4].view(F32)
            raw = S.xyxy_of(c.pool[f], idx)
            # below 0, beyond the frame, exactly on the pad -- in the INPUT; clipped / zero in the reference
            assert (raw[:, 0] < pad_x).any() and (raw[:, 1] < pad_y).any() and (raw[:, 0] == pad_x).any() and (raw[:, 1] == pad_y).any()
            assert (raw[:, 2] > pad_x + ow * gain).any() and (raw[:, 3] > pad_y + oh * gain).any()
            assert (box[:, 0] == 0).sum() >= 2 and (box[:, 2] == ow).any() and (box[:, 3] == oh).any() and box.min() >= 0
            assert (rows[:, 7 + c.extra:] == 0).all()                                      # words past the keypoints
            ext_in = np.ascontiguousarray(c.pool[f].T[idx, 5:])
            ext = rows[:, 7:7 + c.extra]
            if c.kdim == 0:
                assert (ext == ext_in.view(np.uint32)).all()                               # no keypoints: untouched
                continue
            kin, kout = ext_in.reshape(len(idx), -1, c.kdim), ext.view(F32).reshape(len(idx), -1, c.kdim)
            assert (kin[:, 0, 0] == kpad_x).all() and (kout[:, 0, :2] == 0).all()          # exactly on the keypoint pads
            if kin.shape[1] > 2:                                                           # keypoints beside the two planted ones
                assert (kin[..., 0] < kpad_x).any() and (kin[..., 1] > kpad_y + oh * gain).any()
                assert kout[..., :2].min() == 0 and kout[..., 0].max() == ow and kout[..., 1].max() == oh
            if c.extra > c.kdim and kpad_y != pad_y:
                assert (kout[:, 1, 1] > 0).all()                                           # on the BOX pad: not 0 for a keypoint
            if c.kdim == 3:
                assert (_bits(kout[..., 2]) == _bits(kin[..., 2])).all()                   # the confidence word comes back untouched


def test_census_compaction():
    c = S.case("compact")
    assert (c.A, c.max_det, c.ns, c.pack) == (32, 8, (1, 2, 1023, 1024, 1025, 2500), True)
    per_frame = [len(r[1]) for r in c.ref()]
    assert {0, 8} <= set(per_frame) and len(S.sorted_candidates(c.pool[7], 1, c.conf)[0]) == 12      # cut at max_det
    for n in c.ns[2:]:
        counts = np.asarray(per_frame)[c.order(n)]
        assert {0, 8} <= set(counts.tolist()) and len(set(counts.tolist())) >= 6
    assert 1023 <= 1024 < 1025                                                                       # scan_counts_kernel: per = 1, 1, 2, 3


# ------------------------------------------------------------------------------------------------------------ wrong variants
def _same(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all()


def _restated(c, f, flaw):
    return S.restate(c.pool[f], hw=None if c.hw is None else c.hw[f if c.table else 0], flaw=flaw, **c.kwargs())


@pytest.mark.parametrize("name", S.SMALL + ("paths_2048", "classes_70", "scale_kpt4", "scale_pose34_gain2", "compact"))
def test_the_restatement_without_a_flaw_is_the_oracle(name):
    c = S.case(name)
    for f, ref in enumerate(c.ref()):
        got = _restated(c, f, None)
        assert _same(got, ref) and list(got[1]) == list(ref[1]), (name, f)


@pytest.mark.parametrize("flaw", S.FLAWS)
def test_the_inputs_tell_the_oracle_from_a_wrong_variant(flaw):
    caught = [name for name in S.SMALL
              if any(not _same(_restated(S.case(name), f, flaw), ref) for f, ref in enumerate(S.case(name).ref()))]
    assert caught, f"no case tells the oracle from '{flaw}'"


# ----------------------------------------------------------------------------------------------------------------- refusals
@pytest.fixture
def no_library(monkeypatch):
    from cvsd_amd import _lib

    def boom():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(_lib, "lib", boom)


def test_wrapper_refuses_bad_arguments(no_library):
    from cvsd_amd import ops
    z = lambda *s: np.zeros(s, F32)
    bad = [
        dict(pred=z(5, 8), nc=1),                                   # not [n, no, A]
        dict(pred=z(1, 4, 8), nc=1),                                # no class column
        dict(pred=z(1, 5, 8), nc=2),
        dict(pred=z(1, 5, 8), nc=1, max_det=0),
        dict(pred=z(1, 5, 8), nc=1, max_det=1025),
        dict(pred=z(1, 5, 8), nc=1, max_nms=0),
        dict(pred=z(1, 57, 8), nc=1),                               # 52 extra columns
        dict(pred=z(1, 9, 8), nc=1, kdim=3),                        # 3 does not divide 4
        dict(pred=z(1, 9, 8), nc=1, kdim=1),
        dict(pred=z(1, 5, 8), nc=1, kdim=2),                        # keypoints without columns
        dict(pred=z(1, 5, 8), nc=1, conf=-0.5),
        dict(pred=z(1, 5, 8), nc=1, conf=float("nan")),
        dict(pred=z(2, 5, 8), nc=1, geom=z(6)),
        dict(pred=z(2, 5, 8), nc=1, geom=z(3, 7)),
        dict(pred=z(1, 5, 8), nc=1, classes=[]),
        dict(pred=z(1, 5, 8), nc=1, best=z(1, 7, 2)),
        dict(pred=z(1, 8, 8), nc=4, best=z(1, 8, 2) + F32([0, 4]), classes=[1]),       # a class the mask has no bit for
        dict(pred=z(1, 8, 8), nc=4, best=z(1, 8, 2) - F32([0, 1]), classes=[1]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.postprocess(**kw)


def test_entry_point_refuses_bad_arguments_before_touching_a_device():
    """the C side repeats the checks (MI355_EINVAL = -1, no GPU needed) and leaves every output as it was"""
    import ctypes as C
    from cvsd_amd import _lib
    L = _lib.lib()
    pred = np.zeros(4096, F32)
    best = np.zeros(64, F32)
    rows, packed = np.full(1024 * 58, 7, np.uint32), np.full(1024 * 58, 7, np.uint32)
    counts, offsets = np.full(8, 5, np.int32), np.full(9, 5, np.int32)
    geom = np.ones(14, F32)

    def call(n=1, nc=1, extra=0, anchors=8, conf=0.25, classes=None, max_det=8, max_nms=30000, kdim=0, geom_mode=0, g=None, pack=0,
             best_=None, rows_=rows, packed_=None):
        cl = (C.c_int * len(classes))(*classes) if classes else None
        return L.mi355_op_nms_ex(0, pred.ctypes.data, best_, n, nc, extra, anchors, conf, 0.7, cl, len(classes or ()), max_det, max_nms,
                                 kdim, g, geom_mode, pack, rows_.ctypes.data if rows_ is not None else None, counts.ctypes.data,
                                 packed_, offsets.ctypes.data)
    assert call(max_det=0) == -1 and b"max_det" in L.mi355_last_error()
    assert call(max_det=1025) == -1
    assert call(max_nms=0) == -1 and b"max_nms" in L.mi355_last_error()
    assert call(extra=52) == -1 and b"extra" in L.mi355_last_error()
    assert call(extra=4, kdim=3) == -1 and b"kdim" in L.mi355_last_error()
    assert call(extra=4, kdim=1) == -1 and call(extra=0, kdim=2) == -1 and call(extra=4, kdim=4) == -1
    assert call(conf=-0.25) == -1 and b"conf" in L.mi355_last_error()
    assert call(conf=float("nan")) == -1
    assert call(geom_mode=1) == -1 and call(geom_mode=0, g=geom.ctypes.data) == -1 and call(geom_mode=3, g=geom.ctypes.data) == -1
    assert call(pack=1) == -1 and call(n=0) == -1 and call(nc=0) == -1 and call(anchors=0) == -1 and call(rows_=None) == -1
    best[1] = 4.0                                                                    # a class the mask of nc = 4 has no bit for
    assert call(nc=4, classes=[1], best_=best.ctypes.data) == -1 and b"class" in L.mi355_last_error()
    best[1] = -1.0
    assert call(nc=4, classes=[1], best_=best.ctypes.data) == -1
    assert (rows == 7).all() and (packed == 7).all() and (counts == 5).all() and (offsets == 5).all()
