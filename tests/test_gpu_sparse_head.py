"""The sparse box branch (box chain of the Detect head at the NMS candidates only) against the dense head: identical rows.

Every comparison is np.array_equal on rows (boxes, conf, class, anchor index, keypoints) and counts.  The sparse engine is
forced on through MI355_SPARSE_BOX=1 (below the frames-per-pass threshold it would otherwise stay dense); the dense engine is
built with OPT_NO_SPARSE_BOX.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODELS = ["yolov8n", "yolov8n-pose", "yolov5nu", "yolo11n"]


def _rows_equal(a, b, tag):
    ra, ca, _ = a
    rb, cb, _ = b
    assert np.array_equal(ca, cb), f"{tag}: counts differ {ca} vs {cb}"
    for i in range(len(ca)):
        assert np.array_equal(ra[i, :ca[i]].view(np.uint32), rb[i, :cb[i]].view(np.uint32)), f"{tag}: rows of frame {i} differ"


def _pair(name, monkeypatch, chunk, cap=None, nc=None):
    from cvsd_amd import YOLO, _lib
    from tools import synth
    _, sd = synth.synthetic_checkpoint(name, seed=0, nc=nc)
    monkeypatch.setenv("MI355_SPARSE_BOX", "1")
    if cap is not None:
        monkeypatch.setenv("MI355_SPARSE_CAP", str(cap))
    sparse = YOLO.from_state_dict(name, sd, nc=nc, batch_chunk=chunk)
    dense = YOLO.from_state_dict(name, sd, nc=nc, batch_chunk=chunk, flags=_lib.OPT_NO_SPARSE_BOX)
    return sparse, dense, sd


@pytest.mark.parametrize("name", MODELS)
def test_sparse_rows_equal_dense_rows(name, monkeypatch):
    from tools import synth
    # cap = 1: whatever share of the anchors a checkpoint passes on these frames (yolov5nu / yolo11n: most of them), the SPARSE kernels
    # do the work in every pass; the fall-back has its own test below
    sparse, dense, _ = _pair(name, monkeypatch, chunk=16, cap=1.0)
    frames = synth.synthetic_frames(33, 640, 640, seed=1000)
    nc_filter = [0] if name.endswith("-pose") else [0, 3, 17, 42]
    for n in (1, 5, 33):                                        # 33 = two chunks of 16 and a tail chunk of 1
        for conf, classes, max_det in ((0.25, None, 300), (0.1, None, 300), (0.99, None, 300), (1.0, None, 300), (0.25, nc_filter, 300), (0.25, None, 5)):
            got = sparse._infer_rows(frames[:n], conf, 0.7, classes, max_det, 640)
            want = dense._infer_rows(frames[:n], conf, 0.7, classes, max_det, 640)
            _rows_equal(got, want, f"{name} n={n} conf={conf} classes={classes} max_det={max_det}")
            st = sparse.sparse_stats()
            assert st["enabled"] and not st["last_overflow"], st
            if conf == 1.0:                                     # no score exceeds 1: empty lists (the synthetic checkpoint saturates past 0.99)
                assert sum(st["candidates"]) == 0 and int(got[1].sum()) == 0
    st = sparse.sparse_stats()
    assert st["passes"] >= 3 * 6 and st["dense_fallbacks"] == 0, st
    assert not dense.sparse_stats()["enabled"]


@pytest.mark.parametrize("name", MODELS)
def test_over_the_cap_the_dense_fallback_runs(name, monkeypatch):
    """conf 0.001 with the lists capped at a quarter of a level's positions (MI355_SPARSE_CAP=0.25; the default holds every position, so
    that nothing overflows): every chunk overflows its lists, so the gated dense launches are the ones that do the work --
    the merged conv split into its two cout ranges (also the pose head's ragged one), an unmerged cv2.i.0 (yolo11n), and the tail
    chunk's rewritten grids (33 = 16 + 16 + 1)"""
    from tools import synth
    sparse, dense, _ = _pair(name, monkeypatch, chunk=16, cap=0.25)
    frames33 = synth.synthetic_frames(33, 640, 640, seed=1000)
    for n in (1, 5, 33):
        before = sparse.sparse_stats()["dense_fallbacks"]
        got = sparse._infer_rows(frames33[:n], 0.001, 0.7, None, 300, 640)
        want = dense._infer_rows(frames33[:n], 0.001, 0.7, None, 300, 640)
        _rows_equal(got, want, f"{name} conf 0.001 n={n}")
        st = sparse.sparse_stats()
        assert st["enabled"] and st["last_overflow"] and st["dense_fallbacks"] == before + (n + 15) // 16, st
    frames = frames33[:5]
    before = sparse.sparse_stats()["dense_fallbacks"]
    # the same engine, next call under the cap: lists and flag are reset per chunk
    got = sparse._infer_rows(frames, 0.25, 0.7, None, 300, 640)
    want = dense._infer_rows(frames, 0.25, 0.7, None, 300, 640)
    _rows_equal(got, want, "conf 0.25 after an overflow")
    st = sparse.sparse_stats()
    assert st["dense_fallbacks"] == before + int(st["last_overflow"]), st      # the flag is this chunk's, not the last call's
    if name == "yolov8n":                                                     # these frames stay under a cap of 0.25 at conf 0.25
        assert not st["last_overflow"], st


@pytest.mark.parametrize("name", ["yolov8n", "yolov8n-pose"])
def test_sparse_kernels_on_every_anchor(name, monkeypatch):
    """cap = 1: at conf 0.001 the sparse kernels compute (nearly) every anchor, all four borders and corners included"""
    from tools import synth
    sparse, dense, _ = _pair(name, monkeypatch, chunk=4, cap=1.0)
    frames = synth.synthetic_frames(3, 640, 640, seed=1000)
    got = sparse._infer_rows(frames, 0.001, 0.7, None, 300, 640)
    want = dense._infer_rows(frames, 0.001, 0.7, None, 300, 640)
    _rows_equal(got, want, f"{name} cap 1.0 conf 0.001")
    st = sparse.sparse_stats()
    assert st["enabled"] and not st["last_overflow"] and st["dense_fallbacks"] == 0, st
    assert st["candidates"][0] > 0.5 * 3 * 6400 and st["dilated"][0] >= st["candidates"][0], st


def test_sparse_rows_against_the_canonical_order_oracle(monkeypatch):
    from oracle import det
    from tools import synth
    # frames 8 and 15 of the benchmark's base set are its busiest (frame 8: 30 % of the 80x80 anchors pass); cap = 1 keeps the sparse
    # kernels in charge of them
    sparse, _, sd = _pair("yolov8n", monkeypatch, chunk=2, cap=1.0)
    frames = synth.synthetic_frames(16, 640, 640, seed=1000)[[8, 15]]
    got = sparse.predict(frames, imgsz=640)
    st = sparse.sparse_stats()
    assert st["enabled"] and not st["last_overflow"] and st["dense_fallbacks"] == 0 and sum(st["candidates"]) > 1000, st
    want, _ = det.predict(det.DetOracleModel("yolov8n", sd), list(frames), imgsz=640)
    for g, w in zip(got, want):
        assert np.array_equal(g.anchor_idx, w["anchor_idx"].numpy())
        assert np.array_equal(g.boxes.data.numpy(), w["boxes"].numpy())


def test_same_call_twice_and_mixed_sizes(monkeypatch):
    from tools import synth
    # cap = 1: frame 8 alone (the 1-frame tail chunk) passes 30 % of its anchors, over the default cap; here the sparse kernels keep it
    sparse, dense, _ = _pair("yolov8n", monkeypatch, chunk=4, cap=1.0)
    frames = synth.synthetic_frames(9, 640, 640, seed=1000)      # more frames than batch_chunk
    a = sparse._infer_rows(frames, 0.25, 0.7, None, 300, 640)
    b = sparse._infer_rows(frames, 0.25, 0.7, None, 300, 640)
    _rows_equal(a, b, "same call twice")
    _rows_equal(a, dense._infer_rows(frames, 0.25, 0.7, None, 300, 640), "9 frames, chunk 4")
    st = sparse.sparse_stats()
    assert st["enabled"] and not st["last_overflow"] and st["dense_fallbacks"] == 0, st
    mixed = [synth.synthetic_frames(1, 480, 640, seed=7)[0], synth.synthetic_frames(1, 640, 640, seed=8)[0], synth.synthetic_frames(1, 360, 500, seed=9)[0]]
    got = sparse.predict(mixed, imgsz=640)
    want = dense.predict(mixed, imgsz=640)
    st = sparse.sparse_stats()
    assert st["enabled"] and not st["last_overflow"] and st["dense_fallbacks"] == 0, st
    for g, w in zip(got, want):
        assert np.array_equal(g.anchor_idx, w.anchor_idx) and np.array_equal(g.boxes.data.numpy(), w.boxes.data.numpy())


def test_call_to_call_feedback_without_the_override(monkeypatch):
    """The default engine (no MI355_SPARSE_BOX) at 32 frames per pass: a call whose dilated share exceeds sparse_max_share (conf 0.001)
    makes the following calls with the same filter run the dense head (`passes` stands still), the 64th of them probes the sparse
    kernels again, and a call with another conf starts afresh.  Rows equal the dense engine's every time."""
    from cvsd_amd import YOLO, _lib
    from tools import synth
    monkeypatch.delenv("MI355_SPARSE_BOX", raising=False)
    monkeypatch.delenv("MI355_SPARSE_CAP", raising=False)
    _, sd = synth.synthetic_checkpoint("yolov8n", seed=0)
    eng = YOLO.from_state_dict("yolov8n", sd, batch_chunk=32)
    dense = YOLO.from_state_dict("yolov8n", sd, batch_chunk=32, flags=_lib.OPT_NO_SPARSE_BOX)
    frames = synth.synthetic_frames(32, 640, 640, seed=1000)
    want_lo = dense._infer_rows(frames, 0.001, 0.7, None, 300, 640)
    want_hi = dense._infer_rows(frames, 0.25, 0.7, None, 300, 640)
    _rows_equal(eng._infer_rows(frames, 0.001, 0.7, None, 300, 640), want_lo, "first call: sparse kernels on nearly every anchor")
    st = eng.sparse_stats()
    assert st["enabled"] and st["passes"] == 1 and not st["last_overflow"] and st["dense_fallbacks"] == 0, st
    assert st["dilated"][0] > 0.5 * 32 * 6400, st
    for k in range(63):                                        # calls 2 .. 64: the dense head
        _rows_equal(eng._infer_rows(frames, 0.001, 0.7, None, 300, 640), want_lo, f"dense call {k}")
    assert eng.sparse_stats()["passes"] == 1
    _rows_equal(eng._infer_rows(frames, 0.001, 0.7, None, 300, 640), want_lo, "the probe")
    assert eng.sparse_stats()["passes"] == 2
    _rows_equal(eng._infer_rows(frames, 0.001, 0.7, None, 300, 640), want_lo, "dense again after the probe")
    assert eng.sparse_stats()["passes"] == 2
    _rows_equal(eng._infer_rows(frames, 0.25, 0.7, None, 300, 640), want_hi, "another conf: sparse at once")
    assert eng.sparse_stats()["passes"] == 3
    _rows_equal(eng._infer_rows(frames, 0.25, 0.7, None, 300, 640), want_hi, "and it stays sparse (share under the bound)")
    assert eng.sparse_stats()["passes"] == 4


def _sparse_equals_dense_and_ran(sparse, dense, frames, conf, imgsz, tag):
    """rows equal the dense engine's, and the sparse kernels (not the fall-back) produced them"""
    before = sparse.sparse_stats()["passes"]
    got = sparse._infer_rows(frames, conf, 0.7, None, 300, imgsz)
    want = dense._infer_rows(frames, conf, 0.7, None, 300, imgsz)
    _rows_equal(got, want, tag)
    st = sparse.sparse_stats()
    assert st["enabled"] and st["passes"] > before and st["dense_fallbacks"] == 0 and not st["last_overflow"], (tag, st)
    return got, st


@pytest.mark.parametrize("nc", [1, 2])
def test_one_and_two_class_detectors_take_the_element_wise_box_store(nc, monkeypatch):
    """no = 5 and 6: rows of `pred` are not 16-byte aligned, so the box leaves the sparse kernel word by word.  320 x 320 frames
    (40 / 20 / 10 levels), 5 frames in chunks of 4: a tail chunk of one frame"""
    from tools import synth
    sparse, dense, _ = _pair("yolov8n", monkeypatch, chunk=4, cap=1.0, nc=nc)
    assert sparse.nc == nc
    frames = synth.synthetic_frames(5, 320, 320, seed=1000)
    for conf in (0.25, 0.001):
        got, st = _sparse_equals_dense_and_ran(sparse, dense, frames, conf, 320, f"nc={nc} conf={conf}")
        if conf == 0.001:
            assert sum(st["candidates"]) > 0 and int(got[1].sum()) > 0, st
    assert sparse.sparse_stats()["passes"] >= 4


def test_rectangular_levels(monkeypatch):
    """a uniform batch of 480 x 640 frames: the rect letterbox gives 60 x 80, 30 x 40 and 15 x 20 levels, so the kernels' y / x
    arithmetic sees H != W"""
    from tools import synth
    sparse, dense, _ = _pair("yolov8n", monkeypatch, chunk=4, cap=1.0)
    frames = synth.synthetic_frames(5, 480, 640, seed=1000)
    for conf in (0.25, 0.001):
        got, st = _sparse_equals_dense_and_ran(sparse, dense, frames, conf, 640, f"480x640 conf={conf}")
        if conf == 0.001:
            assert st["candidates"][0] > 0 and int(got[1].sum()) > 0, st
