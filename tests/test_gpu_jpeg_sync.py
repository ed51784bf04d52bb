"""``entropy="sync"`` on the GPU (csrc/jpeg_decode_kernels.hip, csrc/jpeg_sync.h): the case table and the longer inputs of
tests/_jpeg_sync_cases.py against the host twin, bit for bit -- pixels, coefficients and, through the hook, every subsequence's entry
state, block index and the round counts (the twin executes the kernels' rounds synchronously; it is checked against the sequential
routine, Pillow and a sequential bit walk in tests/test_jpeg_sync_cases.py); calls that mix sync, lane and host frames; destinations;
the handle's work buffer; and ``JPEGFrame(data, entropy="sync")`` sources of predict / track / track_cameras.  Integer arithmetic:
nothing here has a tolerance.  Every stream here is well-formed."""
import numpy as np
import pytest
import torch

import _jpeg_decode_cases as K
import _jpeg_sync_cases as S
from cvsd_amd import JPEGFrame, ops
from tools import synth

pytestmark = pytest.mark.gpu

GROUPS = S.groups()
NEW_GROUPS = S.groups(new_only=True)


@pytest.fixture(scope="module")
def twin():
    """the sync twin's pixels and coefficients of every stream, computed once"""
    out = {}
    for (name, lay), members in GROUPS.items():
        streams = [S.stream(name, lay, q, enc) for _, q, enc in members]
        pix = ops.jpeg_decode(streams, device=-1, entropy="sync")
        coef = ops.jpeg_decode_coefficients(streams, device=-1, entropy="sync")
        for (cid, _, _), p, c in zip(members, pix, coef):
            out[cid] = (p, c)
    return out


@pytest.mark.parametrize("group", list(GROUPS), ids=lambda g: f"{g[0]}-{g[1]}")
def test_every_case_matches_the_host_twin(twin, group):
    """the streams of one input and layout -- every quality and encoder -- in ONE call"""
    members = GROUPS[group]
    streams = [S.stream(group[0], group[1], q, enc) for _, q, enc in members]
    info = []
    got = ops.jpeg_decode(streams, device=0, entropy="sync", timing=info)
    coef = ops.jpeg_decode_coefficients(streams, device=0, entropy="sync")
    assert info[0]["entropy"] == ["sync"] * len(streams) and info[0]["ms"] > 0
    for (cid, _, _), g, c in zip(members, got, coef):
        assert g.dtype == np.uint8 and g.shape == twin[cid][0].shape and np.array_equal(g, twin[cid][0]), cid
        assert c.dtype == np.int16 and np.array_equal(c, twin[cid][1]), cid


@pytest.mark.parametrize("group", list(NEW_GROUPS), ids=lambda g: f"{g[0]}-{g[1]}")
def test_hook_matches_the_host_twin(group):
    for cid, q, enc in NEW_GROUPS[group]:
        d = S.stream(group[0], group[1], q, enc)
        for sub, seq in S.SETTINGS:
            want, got = ops.jpeg_sync(d, -1, sub, seq), ops.jpeg_sync(d, 0, sub, seq)
            assert got["status"] == want["status"] == 0 and got["stats"] == want["stats"], (cid, sub, seq, got["stats"], want["stats"])
            assert np.array_equal(got["coefficients"], want["coefficients"]), (cid, sub, seq)
            assert np.array_equal(got["states"], want["states"]), (cid, sub, seq)


def _mixed():
    """sync, lane and host frames of different sizes and layouts, by per-frame request"""
    picks = [("noise48x64", "444", 100, "std", "sync"), ("33x70", "420", 85, "rr1", "gpu"), ("flat64x96", "422", 50, "opt", "host"),
             ("smooth64x96", "gray", 100, "rr1", "sync"), ("17x17", "444", 100, "opt", None), ("noise96x128", "420", 50, "std", "sync"),
             ("rows144x8", "420", 100, "rr1", None), ("noise96x128", "444", 100, "opt", "sync"), ("1x1", "422", 85, "rb1", "sync")]
    return [JPEGFrame(S.stream(*p[:4]), entropy=p[4]) for p in picks]


def test_one_call_mixing_sync_lane_and_host_frames():
    frames = _mixed()
    want = [ops.jpeg_decode(f.data, device=-1) for f in frames]
    info = []
    got = ops.jpeg_decode(frames, device=0, timing=info)
    assert info[0]["entropy"] == ["sync", "gpu", "host", "sync", "host", "sync", "gpu", "sync", "sync"]
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    for f, w in zip(frames, want):
        assert np.array_equal(ops.jpeg_decode(f, device=0), w)
    tens = ops.jpeg_decode(frames, device=0, as_tensor=True)
    for t, w in zip(tens, want):
        assert t.is_cuda and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), w)
    coef = ops.jpeg_decode_coefficients(frames, device=0)
    for c, f in zip(coef, frames):
        assert np.array_equal(c, ops.jpeg_decode_coefficients(f.data, device=-1, entropy="host"))


def test_pitched_device_and_host_destinations():
    streams = [f.data for f in _mixed()[:4]]
    want = [ops.jpeg_decode(d, device=-1) for d in streams]
    bufs = [torch.full((w.shape[0] + 2, w.shape[1] + 5, 3), 0x5A, dtype=torch.uint8, device="cuda:0") for w in want]
    views = [b[1:1 + w.shape[0], 2:2 + w.shape[1]] for b, w in zip(bufs, want)]
    ops.jpeg_decode(streams, device=0, out=views, entropy="sync")
    for b, v, w in zip(bufs, views, want):
        assert np.array_equal(v.cpu().numpy(), w)
        mask = torch.ones_like(b, dtype=torch.bool)
        mask[1:1 + w.shape[0], 2:2 + w.shape[1]] = False
        assert bool((b[mask] == 0x5A).all()), "bytes outside the destination were written"
    host = [np.full((w.shape[0], w.shape[1] + 3, 3), 0x5A, np.uint8) for w in want]
    ops.jpeg_decode(streams, device=0, out=[h[:, :w.shape[1]] for h, w in zip(host, want)], entropy="sync")
    for h, w in zip(host, want):
        assert np.array_equal(h[:, :w.shape[1]], w) and (h[:, w.shape[1]:] == 0x5A).all()


def test_auto_still_chooses_as_before():
    plain, rst = S.stream("noise48x64", "420", 50, "std"), S.stream("noise48x64", "420", 50, "rr1")
    info = []
    got = ops.jpeg_decode([plain, rst], device=0, timing=info)
    assert info[0]["entropy"] == ["host", "gpu"]
    got += ops.jpeg_decode([JPEGFrame(plain, entropy="auto"), JPEGFrame(rst, entropy="auto")], device=0, entropy="auto", timing=info)
    assert info[1]["entropy"] == ["host", "gpu"]
    for g, d in zip(got, (plain, rst, plain, rst)):
        assert np.array_equal(g, ops.jpeg_decode(d, device=-1))


def _model(name="yolov8n-pose", **kw):
    from cvsd_amd import YOLO
    _, sd = synth.synthetic_checkpoint(name, seed=0)
    return YOLO.from_state_dict(name, sd, device=0, **kw)


@pytest.fixture(scope="module")
def pose():
    return _model()


def test_a_handles_work_buffer_over_growing_batches(pose):
    frames = _mixed()
    want = [ops.jpeg_decode(f.data, device=-1) for f in frames]
    first = ops.jpeg_decode(frames[:1], device=0, handle=pose._h)
    second = ops.jpeg_decode([f.data for f in frames] * 2, device=0, handle=pose._h, entropy="sync")
    third = ops.jpeg_decode(frames[3:6], device=0, handle=pose._h, as_tensor=True)
    fourth = ops.jpeg_decode(frames * 3, device=0, handle=pose._h)
    assert np.array_equal(first[0], want[0])
    for g, w in zip(second, want * 2):
        assert np.array_equal(g, w)
    for g, w in zip(third, want[3:6]):
        assert np.array_equal(g.cpu().numpy(), w)
    for g, w in zip(fourth, want * 3):
        assert np.array_equal(g, w)


# ---- JPEGFrame(data, entropy="sync") sources of the detector's entry points ---------------------------------------------------------------------
KW = dict(conf=0.05, max_det=12)


def _same(a, b):
    assert np.array_equal(a.boxes.data.numpy(), b.boxes.data.numpy()) and np.array_equal(a.anchor_idx, b.anchor_idx)
    assert np.array_equal(a.keypoints.data.numpy(), b.keypoints.data.numpy())


@pytest.fixture(scope="module")
def shots():
    """two 240 x 320 frames and a 200 x 300 one as streams WITHOUT restart markers (4:2:0, 4:4:4 optimised, 4:2:2) that ask for sync, and
    the host route's decode of each"""
    a, b = synth.synthetic_frames(2, 240, 320, seed=3)
    c = synth.synthetic_frames(1, 200, 300, seed=5)[0]
    data = [K.pillow_encode(a, 90, "420"), K.pillow_encode(b, 95, "444", optimize=True), K.pillow_encode(c, 90, "422")]
    return [JPEGFrame(d, entropy="sync") for d in data], [ops.jpeg_decode(d, device=-1, entropy="host") for d in data]


def test_predict_takes_sync_frames(pose, shots):
    jf, bgr = shots
    info = []
    for g, w in zip(ops.jpeg_decode(jf, device=0, timing=info), bgr):
        assert np.array_equal(g, w)
    assert info[0]["entropy"] == ["sync"] * 3
    for idx in ([0], [0, 1, 2]):
        src, host = [jf[i] for i in idx], [bgr[i] for i in idx]
        got = pose.predict(src if len(src) > 1 else src[0], imgsz=320, **KW)
        want = pose.predict(host, imgsz=320, **KW)
        assert sum(len(r) for r in want) > 0
        for g, w in zip(got, want):
            _same(g, w)
    got = pose.predict(jf, imgsz=160, tile=160, **KW)
    want = pose.predict(bgr, imgsz=160, tile=160, **KW)
    assert sum(len(r) for r in want) > 0
    for g, w in zip(got, want):
        _same(g, w)
        assert np.array_equal(g.tile_idx, w.tile_idx)


def test_track_and_track_cameras_take_sync_frames(shots):
    clip = np.ascontiguousarray(synth.synthetic_clip(3, 240, 320, seed=3))
    data = [K.pillow_encode(f, 92, "420") for f in clip]
    host = [ops.jpeg_decode(d, device=-1, entropy="host") for d in data]
    a, b = _model(), _model()
    tracked = 0
    for i, (d, h) in enumerate(zip(data, host)):
        want = a.track(h, persist=i > 0, imgsz=320, **KW)[0]
        got = b.track(JPEGFrame(d, entropy="sync"), persist=i > 0, imgsz=320, **KW)[0]
        assert np.array_equal(got.boxes.data.numpy(), want.boxes.data.numpy())
        assert (got.boxes.id is None) == (want.boxes.id is None)
        if want.boxes.id is not None:
            assert np.array_equal(got.boxes.id.numpy(), want.boxes.id.numpy())
            tracked += len(want.boxes.id)
    assert tracked > 0
    jf, bgr = shots
    for t in range(2):
        want = a.track_cameras([host[t], None, bgr[2]], persist=t > 0, imgsz=320, **KW)
        got = b.track_cameras([JPEGFrame(data[t], entropy="sync"), None, jf[2]], persist=t > 0, imgsz=320, **KW)
        assert got[1] is None and want[1] is None
        for g, w in ((got[0], want[0]), (got[2], want[2])):
            assert np.array_equal(g.boxes.data.numpy(), w.boxes.data.numpy())
