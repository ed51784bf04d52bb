"""BoT-SORT's appearance half in the product's tracker core (csrc/tracker_host.cpp, ``with_reid``) against its checker
(tests/_botsort_reid_numpy.py: the numpy oracle plus BOTrack's feature bookkeeping and BOTSORT.get_dists in stated arithmetic orders),
hand-derived known answers for the cost and its two gates, and the ``tracker=`` argument's parsing.  No GPU is touched."""
import numpy as np
import pytest

import _botsort_reid_numpy as B
from cvsd_amd import tracker as P
from test_tracker_core import _clip

DIM = 16


def _clip_with_feats(seed, n_frames=60, n_people=5):
    """``test_tracker_core._clip``'s detections, each given an appearance: a box belongs to the person whose (hidden) walk it is nearest
    to in size -- the generator does not say who a box is, so the identity is recovered from the box SIZE, which is fixed per person --
    a fixed random unit vector per person plus small per-frame noise; spurious boxes get a random vector."""
    clip = _clip(seed, n_frames=n_frames, n_people=n_people, camera=seed % 2 == 0)
    rng = np.random.default_rng(seed)                       # replays the generator's first draws: the people's box sizes
    rng.uniform([60, 60], [640 - 60, 480 - 60], size=(n_people, 2))
    rng.uniform(-5, 5, size=(n_people, 2))
    size = rng.uniform([24, 60], [60, 150], size=(n_people, 2))
    frng = np.random.default_rng(1000 + seed)
    person = frng.normal(size=(n_people, DIM))
    person /= np.linalg.norm(person, axis=1, keepdims=True)
    out, known, boxes = [], 0, 0
    for det, warp in clip:
        feats = np.empty((len(det), DIM), np.float32)
        for i, d in enumerate(det):
            wh = np.array([d[2] - d[0], d[3] - d[1]])
            err = np.abs(size - wh).sum(1)
            who = int(err.argmin())
            base = person[who] if err[who] < 12 else frng.normal(size=DIM)
            known, boxes = known + int(err[who] < 12), boxes + 1
            feats[i] = (3.0 * (base + frng.normal(0, 0.05, DIM))).astype(np.float32)      # not unit length: the tracker normalises
        out.append((det, warp, feats))
    # the replay above follows ``_clip``'s first three draws: were they reordered there, the sizes would no longer be the people's and
    # nearly every box would get a random vector (spurious boxes are ~0.4 per frame against several people)
    assert known >= 0.8 * boxes, f"only {known} of {boxes} boxes match a person's size: _clip's draws no longer match this replay"
    return out


@pytest.mark.parametrize("seed", range(8))
def test_cpp_core_with_features_reproduces_the_checker(seed):
    """Rows and every track's smooth_feat, bit for bit.  (The box columns come from the Kalman filter, whose 4x4 gain system the C++
    solves by Cholesky and the numpy oracle by LU: tests/test_tracker_core.py documents last-bit float64 differences there that a
    float32 row almost never shows.  They are asserted bit for bit here as well; the clips are short enough that none shows.)"""
    clip = _clip_with_feats(seed, n_people=4 + seed % 4)
    p, o = P.BYTETracker(gmc_method=None, with_reid=True), B.BOTSORT()
    n_feat = n_rows = 0
    for f, (det, warp, feats) in enumerate(clip):
        rp, ro = p.update(det, warp=warp, feats=feats), o.update(det, warp=warp, feats=feats)
        assert rp.shape == ro.shape, f"frame {f}: {len(rp)} rows vs the checker's {len(ro)}"
        assert rp.tobytes() == ro.tobytes(), f"frame {f}: rows differ\n{rp}\n{ro}"
        n_rows += len(rp)
        assert [t.track_id for t in p.tracked_stracks] == [t.track_id for t in o.tracked_stracks]
        assert [t.track_id for t in p.lost_stracks] == [t.track_id for t in o.lost_stracks]
        for t in o.tracked_stracks + o.lost_stracks:
            want, got = getattr(t, "smooth_feat", None), p.smooth_feat(t.track_id)
            assert (want is None) == (got is None), f"frame {f}, track {t.track_id}"
            if want is not None:
                assert want.dtype == np.float32 and got.tobytes() == want.tobytes(), f"frame {f}: smooth_feat of track {t.track_id}"
                n_feat += 1
    assert n_rows > 100 and n_feat > 100
    print(f"[reid] clip {seed}: {n_rows} rows and {n_feat} smooth_feat vectors bit-identical, {p._ids_issued} ids")


def test_features_change_the_association_on_the_random_clips():
    """the comparison above would pass on a core that ignored its features if the checker ignored them too: on these clips the ids
    with and without features differ somewhere"""
    differ = 0
    for seed in range(8):
        a, b = P.BYTETracker(gmc_method=None, with_reid=True), P.BYTETracker(gmc_method=None)
        for det, warp, feats in _clip_with_feats(seed, n_people=4 + seed % 4):
            ra, rb = a.update(det, warp=warp, feats=feats), b.update(det, warp=warp)
            differ += ra.shape != rb.shape or not np.array_equal(ra[:, 4:], rb[:, 4:])
    assert differ > 0


@pytest.mark.parametrize("seed", range(4))
def test_with_reid_and_no_features_is_the_iou_tracker(seed):
    """``feats=None`` on a with_reid tracker = Ultralytics' ``encoder is None``: today's tracker, row for row"""
    a, b = P.BYTETracker(gmc_method=None, with_reid=True), P.BYTETracker(gmc_method=None)
    for det, warp in _clip(seed, n_frames=120, camera=seed % 2 == 0):
        ra, rb = a.update(det, warp=warp), b.update(det, warp=warp)
        assert ra.tobytes() == rb.tobytes()
        assert [t.track_id for t in a.lost_stracks] == [t.track_id for t in b.lost_stracks]
    assert a._ids_issued == b._ids_issued > 0


E1, E2 = np.float32([1, 0, 0, 0]), np.float32([0, 1, 0, 0])


def _box(x1, score=0.9, w=40):
    return [x1, 100, x1 + w, 200, score, 0]


def test_known_answer_two_people_cross():
    """Frame 1: person 1 (det row 0) at x in [100, 140], person 2 (row 1) at [110, 150], y in [100, 200], score 0.9 -> tracks 1 and 2,
    confirmed at once (frame 1), zero velocity, so frame 2 predicts the same boxes T1, T2.
    Frame 2: the two have crossed: person 1 (row 0) at [106, 146], person 2 (row 1) at [104, 144].
      IoU(T1, row 1) = 36/44 = .818   IoU(T1, row 0) = 34/46 = .739   IoU(T2, row 0) = 36/44 = .818   IoU(T2, row 1) = 34/46 = .739
      every IoU cost (.182 / .261) is below 1 - proximity_thresh = .5: all four pairs are in mutual proximity
      fused with score .9: 1 - .818 * .9 = .264 (T1-row 1, T2-row 0), 1 - .739 * .9 = .335 (T1-row 0, T2-row 1)
    Without features the crossed pairing T1-row 1 + T2-row 0 costs .527 against .670: person 1 (row 0) now carries id 2.
    With features e1, e2 orthogonal: emb = 0 for the same person, (1 - 0) / 2 = .5 > 1 - appearance_thresh = .2 -> 1 for the other;
    min(fused, emb) = 0 for T1-row 0 and T2-row 1, .264 for the crossed pairs: the straight pairing costs 0: person 1 keeps id 1."""
    f1 = np.float32([_box(100), _box(110)])
    f2 = np.float32([_box(106), _box(104)])
    feats = np.stack([E1, E2])
    for tracker in (P.BYTETracker(gmc_method=None), P.BYTETracker(gmc_method=None, with_reid=True)):       # IoU only, both ways to get it
        r1, r2 = tracker.update(f1), tracker.update(f2)
        assert {int(r[7]): int(r[4]) for r in r1} == {0: 1, 1: 2}
        assert {int(r[7]): int(r[4]) for r in r2} == {0: 2, 1: 1}, "IoU + score: the ids cross"
    reid = P.BYTETracker(gmc_method=None, with_reid=True)
    r1, r2 = reid.update(f1, feats=feats), reid.update(f2, feats=feats)
    assert {int(r[7]): int(r[4]) for r in r1} == {0: 1, 1: 2}
    assert {int(r[7]): int(r[4]) for r in r2} == {0: 1, 1: 2}, "with features the ids stay with the people"
    assert reid._ids_issued == 2
    np.testing.assert_array_equal(reid.smooth_feat(1), E1)
    np.testing.assert_array_equal(reid.smooth_feat(2), E2)
    # the checker gives the same answers
    o = B.BOTSORT()
    o.update(f1, feats=feats)
    assert {int(r[7]): int(r[4]) for r in o.update(f2, feats=feats)} == {0: 1, 1: 2}


def test_proximity_gate_no_match_by_appearance_alone():
    """a detection with the track's very feature, but 30 px aside: IoU = 10/70 = .143, IoU cost .857 > 1 - proximity_thresh = .5, so the
    embedding cost is 1 however similar; the fused cost 1 - .143 * .9 = .871 exceeds match_thresh .8: no match, the track is lost and the
    detection starts track 2.  With proximity_thresh lowered to .1 (gate .9) the same pair matches through its embedding cost 0."""
    for prox, matched in ((0.5, False), (0.1, True)):
        t = P.BYTETracker(gmc_method=None, with_reid=True, proximity_thresh=prox)
        t.update(np.float32([_box(100)]), feats=E1[None])
        rows = t.update(np.float32([_box(130)]), feats=E1[None])
        if matched:
            assert len(rows) == 1 and int(rows[0, 4]) == 1 and t._ids_issued == 1
        else:
            assert len(rows) == 0 and t._ids_issued == 2 and [v.track_id for v in t.lost_stracks] == [1]


@pytest.mark.parametrize("cos, matched", [(0.62, True), (0.58, False)])
def test_appearance_gate_just_below_and_just_above(cos, matched):
    """track at [100, 140], detection at [110, 150] with score .3: IoU = 30/50 = .6, IoU cost .4 < .5 (in proximity), fused cost
    1 - .6 * .3 = .82 > match_thresh .8: IoU alone does not match.  Features at an angle with cosine c: emb = (1 - c) / 2 =
    .19 for c = .62 (below 1 - appearance_thresh = .2: kept, min(.82, .19) matches) and .21 for c = .58 (above: set to 1, no match)."""
    t = P.BYTETracker(gmc_method=None, with_reid=True)
    t.update(np.float32([_box(100)]), feats=np.float32([[1, 0]]))
    rows = t.update(np.float32([_box(110, score=0.3)]), feats=np.float32([[cos, np.sqrt(1 - cos * cos)]]))
    o = B.BOTSORT()
    o.update(np.float32([_box(100)]), feats=np.float32([[1, 0]]))
    rows_o = o.update(np.float32([_box(110, score=0.3)]), feats=np.float32([[cos, np.sqrt(1 - cos * cos)]]))
    assert rows.tobytes() == rows_o.tobytes()
    if matched:
        assert len(rows) == 1 and int(rows[0, 4]) == 1 and t._ids_issued == 1
        assert t.smooth_feat(1).tobytes() == o.tracked_stracks[0].smooth_feat.tobytes()
    else:
        assert len(rows) == 0 and t._ids_issued == 2
    plain = P.BYTETracker(gmc_method=None)
    plain.update(np.float32([_box(100)]))
    assert len(plain.update(np.float32([_box(110, score=0.3)]))) == 0


def test_zero_norm_feature():
    """a zero-norm feature stays zeros and costs 1 (numpy would make NaN of it): the pair associates as on IoU alone, nothing becomes NaN,
    and the track's smooth_feat takes the direction of the first real feature it absorbs"""
    z = np.zeros((1, 4), np.float32)
    t, o = P.BYTETracker(gmc_method=None, with_reid=True), B.BOTSORT()
    for det, f in ((_box(100), z), (_box(102), z), (_box(104), E2[None] * 5), (_box(106), z)):
        rp, ro = t.update(np.float32([det]), feats=f), o.update(np.float32([det]), feats=f)
        assert rp.tobytes() == ro.tobytes() and np.isfinite(rp).all() and len(rp) == 1 and int(rp[0, 4]) == 1
        assert t.smooth_feat(1).tobytes() == o.tracked_stracks[0].smooth_feat.tobytes()
    np.testing.assert_array_equal(t.smooth_feat(1), E2)


def test_results_carry_feats_through_every_index_form():
    import torch
    from cvsd_amd.results import Results
    f = np.arange(12, dtype=np.float32).reshape(4, 3)
    boxes = torch.zeros((4, 6))
    boxes[:, 4] = torch.arange(4)
    r = Results(None, "x", {0: "person"}, boxes=boxes, orig_shape=(10, 10), feats=f)
    for idx in (0, -1, np.int64(2), slice(1, 3), [3, 0], np.array([2, 2, 1]), torch.tensor([1, 3])):
        sub = r[idx]
        want = np.atleast_1d(np.arange(4)[idx.numpy() if isinstance(idx, torch.Tensor) else idx])
        assert sub.boxes.conf.numpy().astype(int).tolist() == want.tolist()
        np.testing.assert_array_equal(sub.feats, f[want])


def test_update_argument_checks():
    t = P.BYTETracker(gmc_method=None, with_reid=True)
    with pytest.raises(ValueError):
        t.update(np.float32([_box(100)]), feats=np.zeros((2, 4), np.float32))      # one row per detection
    t.update(np.float32([_box(100)]), feats=E1[None])
    with pytest.raises(ValueError):
        t.update(np.float32([_box(100)]), feats=np.zeros((1, 8), np.float32))      # the width is fixed by the first frame
    with pytest.raises(ValueError):
        P.BYTETracker(gmc_method=None, with_reid=True, appearance_thresh=1.5)
    with pytest.raises(KeyError):
        t.smooth_feat(99)
    # features handed to a tracker without with_reid are not read
    plain = P.BYTETracker(gmc_method=None)
    assert len(plain.update(np.float32([_box(100)]), feats=np.zeros((7, 3), np.float32))) == 1


def test_tracker_argument_parsing(tmp_path):
    cfg = P.tracker_config
    assert cfg(None) == {}
    assert cfg({"with_reid": True}) == {"with_reid": True}
    full = {"tracker_type": "botsort", "track_high_thresh": 0.25, "track_low_thresh": 0.1, "new_track_thresh": 0.25, "track_buffer": 30,
            "match_thresh": 0.8, "fuse_score": True, "gmc_method": "sparseOptFlow", "proximity_thresh": 0.4, "appearance_thresh": 0.7,
            "with_reid": True, "model": "auto"}
    assert cfg(full) == {"with_reid": True, "proximity_thresh": 0.4, "appearance_thresh": 0.7}
    path = tmp_path / "botsort.yaml"
    path.write_text("".join(f"{k}: {str(v) if not isinstance(v, bool) else str(v).lower()}\n" for k, v in full.items()))
    assert cfg(str(path)) == cfg(full)
    P.BYTETracker(gmc_method=None, **cfg(full))
    refusals = [({"tracker_type": "bytetrack"}, "tracker_type"), ({"with_reid": True, "model": "yolo11n-cls.pt"}, "model"),
                ({"match_thresh": 0.7}, "match_thresh"), ({"track_buffer": 60}, "track_buffer"), ({"fuse_score": False}, "fuse_score"),
                ({"gmc_method": "orb"}, "gmc_method"), ({"with_reid": "yes"}, "with_reid"), ({"proximity_thresh": 2}, "proximity_thresh"),
                ({"appearance_thresh": True}, "appearance_thresh"), ({"wtih_reid": True}, "wtih_reid")]
    for bad, key in refusals:
        with pytest.raises(ValueError, match=key):
            cfg(bad)
    bt = tmp_path / "bytetrack.yaml"                         # Ultralytics' bytetrack.yaml contents
    bt.write_text("tracker_type: bytetrack\ntrack_high_thresh: 0.25\ntrack_low_thresh: 0.1\nnew_track_thresh: 0.25\ntrack_buffer: 30\n"
                  "match_thresh: 0.8\nfuse_score: True\n")
    with pytest.raises(ValueError, match="tracker_type"):
        cfg(str(bt))
