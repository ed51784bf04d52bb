"""JPEG ingest on the GPU (csrc/jpeg_decode_kernels.hip): the case table of tests/_jpeg_decode_cases.py through
``ops.jpeg_decode`` against the host twin, bit for bit, with the entropy stage on the GPU's lanes and on the host (the host twin is
checked against the sequential checker and Pillow in tests/test_jpeg_decode_cases.py); batching; the round trip through the GPU
encoder; and ``JPEGFrame`` sources of predict / track / track_cameras against the same calls on the decoded frames.  The feature is
integer arithmetic: nothing here has a tolerance.  Every stream here is well-formed."""
import numpy as np
import pytest
import torch

import _jpeg_decode_cases as K
from cvsd_amd import JPEGFrame, ops
from tools import synth

pytestmark = pytest.mark.gpu

GROUPS = K.groups()


@pytest.fixture(scope="module")
def twin():
    """the host twin's pixels and coefficients of every stream of the table, computed once"""
    out = {}
    for (name, lay), members in GROUPS.items():
        for cid, q, enc in members:
            d = K.stream(name, lay, q, enc)
            out[cid] = (ops.jpeg_decode(d, device=-1), ops.jpeg_decode_coefficients(d, device=-1))
    return out


@pytest.mark.parametrize("entropy", ["gpu", "host"])
@pytest.mark.parametrize("group", list(GROUPS), ids=lambda g: f"{g[0]}-{g[1]}")
def test_every_case_matches_the_host_twin(twin, group, entropy):
    """the streams of one input and layout -- every quality and encoder -- in ONE call"""
    members = GROUPS[group]
    streams = [K.stream(group[0], group[1], q, enc) for _, q, enc in members]
    info = []
    got = ops.jpeg_decode(streams, device=0, entropy=entropy, timing=info)
    coef = ops.jpeg_decode_coefficients(streams, device=0, entropy=entropy)
    assert info[0]["entropy"] == [entropy] * len(streams)
    for (cid, _, _), g, c in zip(members, got, coef):
        assert g.dtype == np.uint8 and g.shape == twin[cid][0].shape and np.array_equal(g, twin[cid][0]), cid
        assert c.dtype == np.int16 and np.array_equal(c, twin[cid][1]), cid


def test_auto_takes_the_lanes_for_restart_streams_only():
    plain, rst = K.stream("33x70", "420", 85, "std"), K.stream("33x70", "420", 85, "rr1")
    own = K.stream("33x70", "420", 50, "own")
    assert (JPEGFrame(plain).restart_interval, JPEGFrame(plain).segments) == (0, 1)
    assert JPEGFrame(rst).restart_interval > 0 and JPEGFrame(own).segments == 3
    info = []
    got = ops.jpeg_decode([plain, rst, own], device=0, timing=info)
    assert info[0]["entropy"] == ["host", "gpu", "gpu"] and info[0]["ms"] > 0
    for g, d in zip(got, (plain, rst, own)):
        assert np.array_equal(g, ops.jpeg_decode(d, device=-1))


def _mixed():
    """all four layouts, eight sizes, optimised and standard tables, restart and no-restart streams"""
    picks = [("33x70", "420", 85, "std"), ("17x17", "444", 100, "opt"), ("20x5", "422", 50, "rb2"), ("35x18", "gray", 1, "rr1"),
             ("rows144x8", "420", 100, "rr1"), ("rows72x8", "444", 50, "own"), ("1x1", "422", 85, "rb1"), ("9x4", "420", 85, "std"),
             ("40x1", "gray", 100, "opt"), ("33x70", "422", 100, "rr1")]
    return [K.stream(*p) for p in picks]


@pytest.mark.parametrize("entropy", ["auto", "gpu", "host"])
def test_one_call_over_a_mixed_list_equals_the_single_calls(entropy):
    streams = _mixed()
    want = [ops.jpeg_decode(d, device=-1) for d in streams]
    got = ops.jpeg_decode(streams, device=0, entropy=entropy)
    single = [ops.jpeg_decode(d, device=0, entropy=entropy) for d in streams]
    for w, g, s in zip(want, got, single):
        assert np.array_equal(g, w) and np.array_equal(s, w)
    tens = ops.jpeg_decode(streams, device=0, entropy=entropy, as_tensor=True)
    for w, t in zip(want, tens):
        assert t.is_cuda and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), w)


def test_pitched_device_and_host_destinations():
    streams = _mixed()[:4]
    want = [ops.jpeg_decode(d, device=-1) for d in streams]
    bufs = [torch.full((w.shape[0] + 2, w.shape[1] + 5, 3), 0x5A, dtype=torch.uint8, device="cuda:0") for w in want]
    views = [b[1:1 + w.shape[0], 2:2 + w.shape[1]] for b, w in zip(bufs, want)]           # rows 15 bytes longer, first byte at an odd offset
    ops.jpeg_decode(streams, device=0, out=views)
    for b, v, w in zip(bufs, views, want):
        assert np.array_equal(v.cpu().numpy(), w)
        mask = torch.ones_like(b, dtype=torch.bool)
        mask[1:1 + w.shape[0], 2:2 + w.shape[1]] = False
        assert bool((b[mask] == 0x5A).all()), "bytes outside the destination were written"
    host = [np.full((w.shape[0], w.shape[1] + 3, 3), 0x5A, np.uint8) for w in want]
    ops.jpeg_decode(streams, device=0, out=[h[:, :w.shape[1]] for h, w in zip(host, want)])
    for h, w in zip(host, want):
        assert np.array_equal(h[:, :w.shape[1]], w) and (h[:, w.shape[1]:] == 0x5A).all()


def _model(name="yolov8n-pose", **kw):
    from cvsd_amd import YOLO
    _, sd = synth.synthetic_checkpoint(name, seed=0)
    return YOLO.from_state_dict(name, sd, device=0, **kw)


@pytest.fixture(scope="module")
def pose():
    return _model()


def test_a_larger_second_batch_reuses_the_handles_work_buffer(pose):
    streams = _mixed()
    want = [ops.jpeg_decode(d, device=-1) for d in streams]
    first = ops.jpeg_decode(streams[:2], device=0, handle=pose._h)
    second = ops.jpeg_decode(streams * 3, device=0, handle=pose._h, entropy="gpu")
    third = ops.jpeg_decode(streams[3:6], device=0, handle=pose._h, as_tensor=True)
    for g, w in zip(first, want[:2]):
        assert np.array_equal(g, w)
    for g, w in zip(second, want * 3):
        assert np.array_equal(g, w)
    for g, w in zip(third, want[3:6]):
        assert np.array_equal(g.cpu().numpy(), w)


@pytest.mark.parametrize("ss", ["420", "444"])
def test_gpu_round_trip(ss):
    """the project's own streams -- a restart segment per MCU row -- are the lanes' natural input"""
    frames = [synth.synthetic_frames(1, 120, 168, seed=5)[0], K._frames()["33x70"], K._frames()["rows144x8"]]
    streams = ops.jpeg_encode(frames, quality=90, subsampling=ss, device=0)
    info = []
    got = ops.jpeg_decode(streams, device=0, timing=info)
    assert info[0]["entropy"] == ["gpu"] * 3
    for f, d, g in zip(frames, streams, got):
        assert JPEGFrame(d).segments == -(-f.shape[0] // (16 if ss == "420" else 8))
        assert np.array_equal(g, ops.jpeg_decode(d, device=-1)) and np.array_equal(g, K.pillow_decode(d))


# ---- JPEGFrame sources of the detector's entry points ---------------------------------------------------------------------------------------
KW = dict(conf=0.05, max_det=12)


def _same(a, b):
    assert np.array_equal(a.boxes.data.numpy(), b.boxes.data.numpy()) and np.array_equal(a.anchor_idx, b.anchor_idx)
    assert np.array_equal(a.keypoints.data.numpy(), b.keypoints.data.numpy())


@pytest.fixture(scope="module")
def shots():
    """two 240 x 320 frames and a 200 x 300 one as JPEG streams (4:2:0 with restart rows, 4:4:4 optimised, 4:2:2), their JPEGFrames and
    the host twin's decode of each"""
    a, b = synth.synthetic_frames(2, 240, 320, seed=3)
    c = synth.synthetic_frames(1, 200, 300, seed=5)[0]
    data = [K.pillow_encode(a, 90, "420", restart_marker_rows=1), K.pillow_encode(b, 95, "444", optimize=True), K.pillow_encode(c, 90, "422")]
    return [JPEGFrame(d) for d in data], [ops.jpeg_decode(d, device=-1) for d in data]


def test_predict_takes_jpeg_frames(pose, shots):
    jf, bgr = shots
    for idx in ([0], [0, 1, 2]):                                           # one frame; mixed shapes
        src, host = [jf[i] for i in idx], [bgr[i] for i in idx]
        got = pose.predict(src if len(src) > 1 else src[0], imgsz=320, **KW)
        dev = pose.predict([torch.from_numpy(h).cuda() for h in host], imgsz=320, **KW)
        want = pose.predict(host, imgsz=320, **KW)
        assert sum(len(r) for r in want) > 0
        for g, d, w in zip(got, dev, want):
            _same(g, d)
            _same(g, w)
    with pytest.raises(ValueError, match="all host arrays or all CUDA"):
        pose.predict([jf[0], bgr[1]], imgsz=320, **KW)


def test_predict_render_encode_feats_and_tile(pose, shots):
    jf, bgr = shots
    got = pose.predict(jf[:2], imgsz=320, render=True, encode="jpeg", **KW)
    want = pose.predict(bgr[:2], imgsz=320, render=True, encode="jpeg", **KW)
    for g, w in zip(got, want):
        _same(g, w)
        assert g.jpeg is not None and g.jpeg == w.jpeg
    got = pose.predict(jf, imgsz=320, feats=True, **KW)
    want = pose.predict(bgr, imgsz=320, feats=True, **KW)
    for g, w in zip(got, want):
        _same(g, w)
        assert g.feats is not None and np.array_equal(g.feats, w.feats)
    got = pose.predict(jf, imgsz=160, tile=160, **KW)
    want = pose.predict(bgr, imgsz=160, tile=160, **KW)
    dev = pose.predict([torch.from_numpy(h).cuda() for h in bgr], imgsz=160, tile=160, **KW)
    assert sum(len(r) for r in want) > 0
    for g, d, w in zip(got, dev, want):
        _same(g, w)
        _same(g, d)
        assert np.array_equal(g.tile_idx, w.tile_idx)


def test_track_and_track_cameras_take_jpeg_frames(shots):
    clip = np.ascontiguousarray(synth.synthetic_clip(4, 240, 320, seed=3))
    data = [K.pillow_encode(f, 92, "420", restart_marker_rows=1) for f in clip]
    host = [ops.jpeg_decode(d, device=-1) for d in data]
    a, b = _model(), _model()
    tracked = 0
    for i, (d, h) in enumerate(zip(data, host)):
        want = a.track(h, persist=i > 0, imgsz=320, **KW)[0]
        got = b.track(JPEGFrame(d), persist=i > 0, imgsz=320, **KW)[0]
        assert np.array_equal(got.boxes.data.numpy(), want.boxes.data.numpy())
        assert (got.boxes.id is None) == (want.boxes.id is None)
        if want.boxes.id is not None:
            assert np.array_equal(got.boxes.id.numpy(), want.boxes.id.numpy())
            tracked += len(want.boxes.id)
    assert tracked > 0
    jf, bgr = shots
    for t in range(2):
        want = a.track_cameras([host[t], None, bgr[2]], persist=t > 0, imgsz=320, **KW)
        got = b.track_cameras([JPEGFrame(data[t]), None, jf[2]], persist=t > 0, imgsz=320, **KW)
        assert got[1] is None and want[1] is None
        for g, w in ((got[0], want[0]), (got[2], want[2])):
            assert np.array_equal(g.boxes.data.numpy(), w.boxes.data.numpy())
    mixed = b.track_cameras([JPEGFrame(data[2]), None, bgr[2]], persist=True, imgsz=320, **KW)      # a JPEG camera beside a BGR camera
    ref = a.track_cameras([host[2], None, bgr[2]], persist=True, imgsz=320, **KW)
    for g, w in ((mixed[0], ref[0]), (mixed[2], ref[2])):
        assert np.array_equal(g.boxes.data.numpy(), w.boxes.data.numpy())
