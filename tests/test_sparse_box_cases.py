"""CPU side of tests/test_gpu_sparse_box.py: the wrapper's and the entry's argument checks, the census of the planted score
patterns (a later edit of a pattern must not be able to drop an edge silently), the proof that the inputs tell the true list
reference from six wrong ones, and the references themselves.  9 cases (tests/_sparse_box_cases.py)."""
from collections import Counter

import numpy as np
import pytest

import _sparse_box_cases as S


@pytest.fixture
def no_library(monkeypatch):
    """any library call from the wrapper is a failure: validation comes first"""
    from cvsd_amd import _lib

    def boom():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(_lib, "lib", boom)


def _level(cin=16, cs=None, h=2, w=3, n=1, cout_a=64, **kw):
    z = lambda *s: np.zeros(s, np.float32)
    lv = dict(src=z(n, h, w, cs or cin), cin=cin, wA=z(cout_a, cin, 3, 3), bA=z(cout_a), wB=z(64, 64, 3, 3), bB=z(64),
              wC=z(64, 64, 1, 1), bC=z(64), stride=8)
    lv.update(kw)
    return lv


def test_the_case_list_stays_small():
    assert len(S.CASES) == 9 and len(S.PLAIN_CASES) == 7 and S.OVERFLOW_CASES == ("over_dil", "over_cand")
    for name in S.CASES:
        c = S.case(name)
        assert c.n * c.A <= 3 * 315 and c.cin in (16, 64, 128)


def test_cases_cover_the_shapes_the_kernels_branch_on():
    cs = [S.case(k) for k in S.PLAIN_CASES]
    assert {c.cin for c in cs} == {16, 64, 128}
    assert {c.no for c in cs} == {5, 6, 7, 56, 84} and {c.no % 4 == 0 for c in cs} == {True, False}
    assert {c.mid for c in cs} >= {(64, 0)} and any(m[0] == 144 and m[1] > 0 for m in (c.mid for c in cs))
    assert any(c.view == (c.cin, 0) for c in cs) and any(c.view[0] > c.cin and c.view[1] > 0 for c in cs)
    assert any(c.cout_a > 64 for c in cs) and any(c.cout_a == 64 for c in cs)
    assert {len(c.shapes) for c in cs} == {1, 2, 3}
    main = S.case("edges")
    assert main.A == 315 and main.n == 3 and all(h != w for h, w, _ in main.shapes) and 240 < 256 < main.A
    assert S.case("tiny").shapes == ((1, 1, 8),) and S.case("tiny").n == 1


def test_census_every_planted_property_holds_for_some_case():
    seen = Counter()
    for name in S.CASES:
        seen.update(S.census(S.case(name)))
    missing = [k for k in S.REQUIRED if seen[k] < 1]
    assert not missing, (missing, dict(seen))
    # an empty list beside busy ones, too
    assert seen["cand_len_0"] >= 1 and seen["dil_len_0"] >= 1


def test_census_of_named_cases():
    """the properties sit in the cases whose docstrings claim them"""
    e = S.census(S.case("edges"))
    for k in ("four_corners", "each_edge", "last_of_level0_and_first_of_level1", "last_pixel_of_frame0", "row_end_with_clear_wrap_neighbours",
              "a_frame_without_candidates", "score_equals_conf_not_listed", "score_one_ulp_above_conf_listed", "inf_listed",
              "nan_neither_listed_nor_dilating"):
        assert e[k] >= 1, k
    m = S.census(S.case("masked"))
    assert m["every_listed_class_kept"] == 1 and m["excluded_class_at_0.99_neither_listed_nor_dilating"] == 3
    assert m["cand_wave_all_flagged"] >= 1 and m["cand_len_64"] == 1 and m["cand_len_65"] == 1
    ln = S.case("lengths")
    assert [len(v) for v in ln.ref_dil] == [64, 16, 17] and S.census(ln)["caps_equal_counts"] == 1
    l2 = S.case("lengths2")
    assert len(l2.ref_dil[0]) == 65 and [len(v) for v in l2.ref_cand[1:]] == [16, 17]
    f = S.case("full")
    assert [len(v) for v in f.ref_cand] == [0, 180, 1] and [len(v) for v in f.ref_dil] == [0, 180, 4]
    assert S.census(f)["full_level"] == 1 and S.census(f)["peaked_dfl"] == 1
    t = S.case("tiny")
    assert [len(v) for v in t.ref_cand] == [1] and [len(v) for v in t.ref_dil] == [1]
    assert S.census(S.case("last_frame"))["only_the_last_frame"] == 1
    od, oc = S.case("over_dil"), S.case("over_cand")
    assert od.overflows and oc.overflows and not ln.overflows
    assert od.inputs[0]["cap_dil"] == 63 and oc.inputs[0]["cap_cand"] == 9 and oc.inputs[0]["cap_dil"] == 720
    assert S.census(od)["cap_dil_one_short"] == 1 and S.census(oc)["cap_cand_one_short_cap_dil_ample"] == 1
    assert ln.inputs[0]["cap_dil"] == 64                         # the base case keeps its own capacities


@pytest.mark.parametrize("wrong", ["ge", "row", "level", "frame", "word0", "nan"])
def test_inputs_tell_the_true_list_reference_from_a_wrong_one(wrong):
    """each deliberately wrong reference differs from the true one on at least one case, in the sorted list entries themselves"""
    differs = []
    for name in S.PLAIN_CASES:
        c = S.case(name)
        cand = S.candidates(c.best, c.conf, c.classes, c.nc, ge=wrong == "ge", nan_passes=wrong == "nan", word0_only=wrong == "word0")
        dil = S.dilate(cand, c.shapes, wrong if wrong in ("row", "level", "frame") else None)
        same = all(np.array_equal(a, b) for a, b in zip(S.entries(cand, c.shapes) + S.entries(dil, c.shapes), c.ref_cand + c.ref_dil))
        if not same:
            differs.append(name)
    assert differs, wrong
    if wrong in ("row", "level", "frame"):                       # the dilation variants leave the candidates alone
        assert np.array_equal(cand, c.cand)


def test_list_reference_on_a_hand_made_map():
    """3 x 4 map, one frame: the statement itself, checked by eye"""
    shapes = ((3, 4, 8),)
    best = np.zeros((1, 12, 2), np.float32)
    best[0, 3, 0] = 0.5                                          # (0, 3)
    best[0, 8, 0] = np.nan                                       # (2, 0)
    cand = S.candidates(best, 0.25)
    assert np.nonzero(cand[0])[0].tolist() == [3]
    assert np.nonzero(S.dilate(cand, shapes)[0])[0].tolist() == [2, 3, 6, 7]
    assert np.nonzero(S.dilate(cand, shapes, "row")[0])[0].tolist() == [2, 3, 4, 6, 7, 8]
    assert S.entries(cand, shapes)[0].dtype == np.int32
    two = np.zeros((2, 12, 2), np.float32)
    two[1, 5, 0] = 1.0
    assert S.entries(S.candidates(two, 0.25), shapes)[0].tolist() == [17]
    m = S.mask_words(S.CLASS_LIST, 80)
    assert m.tolist() == [0x80000001, 0x80000001, 0x00008001]


def test_references_are_finite_where_they_must_be():
    for name in S.PLAIN_CASES:
        c = S.case(name)
        assert c.ref_box.shape == (c.n, c.A, 4) and c.ref_box.dtype == np.float32
        assert np.isfinite(c.ref_box).all() and (c.ref_box[..., 2:] > 0).all()          # widths and heights
        for m, (h, w, _) in zip(c.ref_mid, c.shapes):
            assert m.shape == (c.n, h, w, 64) and np.isfinite(m).all()
        assert all(len(np.unique(e)) == len(e) for e in c.ref_cand + c.ref_dil)
        for cd, dl in zip(c.ref_cand, c.ref_dil):
            assert set(cd.tolist()) <= set(dl.tolist())
    # the peaked case's boxes are not the flat 15-stride boxes of a uniform DFL
    f = S.case("full")
    assert np.ptp(f.ref_box[:, 240:300, 2]) > 16
    # frame() is the frame's slice
    lvs, best = S.case("lengths").frame(1)
    assert best.shape == (1, 315, 2) and all(lv["src"].shape[0] == 1 and lv["cap_dil"] is None for lv in lvs)


def test_wrapper_refuses_bad_arguments(no_library):
    from cvsd_amd import ops
    best = np.zeros((1, 6, 2), np.float32)
    bad = [
        dict(levels=[], best=best, conf=0.25, nc=1),
        dict(levels=[_level()] * 4, best=np.zeros((1, 24, 2), np.float32), conf=0.25, nc=1),     # more than 3 levels
        dict(levels=[_level(cin=24)], best=best, conf=0.25, nc=1),                                # cin % 16
        dict(levels=[_level(cin=16, cs=18)], best=best, conf=0.25, nc=1),                         # pixel stride not 16-byte aligned
        dict(levels=[_level(cin=16, cs=24, src_off=12)], best=best, conf=0.25, nc=1),             # view past the tensor
        dict(levels=[_level(cin=16, cs=24, src_off=2)], best=best, conf=0.25, nc=1),
        dict(levels=[_level(mid_cs=72, mid_off=12)], best=best, conf=0.25, nc=1),                 # 64 from 12 do not fit 72
        dict(levels=[_level(mid_cs=66)], best=best, conf=0.25, nc=1),
        dict(levels=[_level(cout_a=48)], best=best, conf=0.25, nc=1),                             # fewer than 64 couts
        dict(levels=[_level(wB=np.zeros((64, 32, 3, 3), np.float32))], best=best, conf=0.25, nc=1),
        dict(levels=[_level(stride=0)], best=best, conf=0.25, nc=1),
        dict(levels=[_level(cap_dil=0)], best=best, conf=0.25, nc=1),
        dict(levels=[_level(cap_cand=7)], best=best, conf=0.25, nc=1),                            # more than n*h*w
        dict(levels=[_level(), _level(n=2)], best=np.zeros((1, 12, 2), np.float32), conf=0.25, nc=1),
        dict(levels=[_level()], best=np.zeros((1, 5, 2), np.float32), conf=0.25, nc=1),           # A
        dict(levels=[_level()], best=best, conf=0.25, nc=0),
        dict(levels=[_level()], best=best, conf=0.25, nc=2, no=5),                                # no < 4 + nc
        dict(levels=[_level()], best=best, conf=0.25, nc=1, act=3),
        dict(levels=[_level()], best=best + np.float32([0, 4]), conf=0.25, nc=4, classes=[1]),    # a class the mask has no bit for
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.sparse_box(**kw)


def test_entry_point_refuses_bad_arguments_before_touching_a_device():
    """the C side repeats the checks (MI355_EINVAL = -1, no GPU needed) and leaves every output as it was"""
    import ctypes as C
    from cvsd_amd import _lib
    L = _lib.lib()
    z = np.zeros(64 * 64 * 9, np.float32)
    out = np.full(4096, 7, np.int32)
    pred = np.full(4096, 3.0, np.float32)
    state = (C.c_int * 12)(*[5] * 12)
    best = np.zeros(2 * 4 * 6, np.float32)

    def call(n_levels=1, geom=(2, 3, 16, 0, 16, 64, 8, 64, 0, 6, 6), nc=1, no=5, act=1, classes=None, ptr_null=None):
        p = [z.ctypes.data] * 7 + [out.ctypes.data] * 3
        if ptr_null is not None:
            p[ptr_null] = None
        ptrs = (C.c_void_p * 40)(*(p * 4))
        g = (C.c_int * 44)(*(list(geom) * 4))
        cl = (C.c_int * len(classes))(*classes) if classes else None
        return L.mi355_op_sparse_box(0, ptrs, g, n_levels, 1, best.ctypes.data, 0.25, cl, len(classes or ()), nc, no, act,
                                     pred.ctypes.data, state)
    assert call(n_levels=4) == -1 and b"1 to 3 levels" in L.mi355_last_error()
    assert call(n_levels=0) == -1
    assert call(geom=(2, 3, 24, 0, 24, 64, 8, 64, 0, 6, 6)) == -1 and b"multiple of 16" in L.mi355_last_error()
    assert call(geom=(2, 3, 16, 0, 0, 64, 8, 64, 0, 6, 6)) == -1
    assert call(geom=(2, 3, 18, 0, 16, 64, 8, 64, 0, 6, 6)) == -1                  # src stride
    assert call(geom=(2, 3, 32, 20, 16, 64, 8, 64, 0, 6, 6)) == -1                 # src view past the tensor
    assert call(geom=(2, 3, 16, 0, 16, 64, 8, 72, 12, 6, 6)) == -1                 # mid view past the tensor
    assert call(geom=(2, 3, 16, 0, 16, 64, 8, 64, 2, 6, 6)) == -1
    assert call(geom=(2, 3, 16, 0, 16, 48, 8, 64, 0, 6, 6)) == -1                  # cout_a
    assert call(geom=(2, 3, 16, 0, 16, 64, 0, 64, 0, 6, 6)) == -1                  # stride
    assert call(geom=(2, 3, 16, 0, 16, 64, 8, 64, 0, 0, 6)) == -1                  # capacities
    assert call(geom=(2, 3, 16, 0, 16, 64, 8, 64, 0, 6, 7)) == -1
    assert call(no=4) == -1 and call(nc=0) == -1 and call(act=3) == -1 and call(ptr_null=8) == -1
    best[1] = 4.0                                                                    # a class the mask of nc = 4 has no bit for
    assert call(nc=4, no=8, classes=[1]) == -1 and b"class" in L.mi355_last_error()
    assert (out == 7).all() and (pred == 3.0).all() and list(state) == [5] * 12
