"""The Python layer of the facade: the same pixels give the same rows whatever form the source takes.

The suite pins every C entry point bit for bit (test_gpu_detector_entry_points.py); this file closes what it leaves open above them, in
``cvsd_amd/sources.py`` and ``engine.py``: the forms of one frame, host against CUDA lists (untiled and tiled), the three ways ``track``
hands a frame to the detector, and which engine ``last_timing`` / ``plan_info`` answer for.  Every comparison is on the uint32 view of
``boxes.data`` and ``keypoints_raw``.  The synthetic yolov8n-pose checkpoint at imgsz 96, conf 0.001; frames 64 x 96, 48 x 80, 96 x 128.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S, CONF = 96, 0.001
ID, RS, BIG = (64, 96), (48, 80), (96, 128)


@pytest.fixture(scope="module")
def case():
    from cvsd_amd import YOLO
    from tools import synth
    name = "yolov8n-pose"
    sd = synth.synthetic_checkpoint(name, seed=0)[1]
    frames = {shape: synth.synthetic_frames(3, shape[0], shape[1], seed=40 + i) for i, shape in enumerate((ID, RS, BIG))}
    return {"name": name, "sd": sd, "model": YOLO.from_state_dict(name, sd), "frames": frames}


def _bits(results):
    """per frame (boxes.data, keypoints_raw) as uint32; a comparison of nothing proves nothing, so every call must have found rows"""
    out = [(r.boxes.data.numpy().view(np.uint32), r.keypoints_raw.view(np.uint32)) for r in results]
    assert all(len(b) for b, _ in out), "a frame without rows"
    return out


def _same(got, want, tag):
    assert len(got) == len(want), tag
    for i, ((b, k), (wb, wk)) in enumerate(zip(got, want)):
        assert np.array_equal(b, wb) and np.array_equal(k, wk), f"{tag}: frame {i} differs"


def test_six_forms_of_one_frame(case):
    m, f = case["model"], case["frames"][ID][0]
    kw = dict(conf=CONF, imgsz=S)
    want = _bits(m.predict(f, **kw))
    dev = torch.from_numpy(f).cuda()
    _same(_bits(m.predict(f[None], **kw)), want, "4-D array")
    _same(_bits(m.predict([f], **kw)), want, "one-element list")
    _same(_bits(m.predict(torch.from_numpy(f[None].copy()), **kw)), want, "CPU 4-D tensor")
    _same(_bits(m.predict(dev[None], **kw)), want, "CUDA 4-D tensor")
    _same(_bits(m.predict([dev, dev.clone()], **kw)), want * 2, "list of two equal CUDA tensors (stacked)")


@pytest.mark.parametrize("tiling", [{}, {"tile": 96, "overlap": 0.25}], ids=["untiled", "tiled"])
def test_three_shapes_host_against_cuda(case, tiling):
    m = case["model"]
    host = [case["frames"][shape][0] for shape in (ID, RS, BIG)]
    want = m.predict(host, conf=CONF, imgsz=S, **tiling)
    got = m.predict([torch.from_numpy(f).cuda() for f in host], conf=CONF, imgsz=S, **tiling)
    _same(_bits(got), _bits(want), "CUDA list")
    assert [r.orig_shape for r in got] == [r.orig_shape for r in want] == [ID, RS, BIG]
    assert all(r.orig_img is f for r, f in zip(want, host)) and all(r.orig_img is None for r in got)


@pytest.mark.parametrize("tile", [None, 96], ids=["untiled", "tiled"])
def test_track_hands_the_same_frame_over_three_ways(case, tile, monkeypatch):
    """the copy the motion compensation uploaded (the default), the host frame (MI355_TRACK_SHARED_FRAME=0), and predict() (stream=True)"""
    m, frames = case["model"], list(case["frames"][BIG])
    kw = dict(conf=CONF, imgsz=S, **({} if tile is None else {"tile": tile}))

    def run(**more):
        res = m.track(frames, persist=False, **kw, **more)     # persist=False: every run starts a tracker of its own
        return [(r.boxes.data.numpy().view(np.uint32), None if r.boxes.id is None else r.boxes.id.numpy()) for r in res]

    monkeypatch.delenv("MI355_TRACK_SHARED_FRAME", raising=False)
    want = run()
    assert all(len(b) for b, _ in want), "a frame without rows"
    monkeypatch.setenv("MI355_TRACK_SHARED_FRAME", "0")
    not_shared = run()
    monkeypatch.delenv("MI355_TRACK_SHARED_FRAME")
    streamed = run(stream=True)
    m._tracker = None                                           # the model is shared by the module's tests
    for tag, got in (("MI355_TRACK_SHARED_FRAME=0", not_shared), ("stream=True", streamed)):
        for i, ((b, ids), (wb, wids)) in enumerate(zip(got, want)):
            assert np.array_equal(b, wb) and (ids is None) == (wids is None) and np.array_equal(ids, wids), f"{tag}: frame {i} differs"


def test_timing_and_plans_answer_for_the_engine_that_ran(case):
    from cvsd_amd import YOLO, _lib
    m = YOLO.from_state_dict(case["name"], case["sd"], half=False)
    f = case["frames"][ID][0]
    m.predict(f, conf=CONF, imgsz=S)
    assert m._last_handle.value == m._h.value
    m.predict(f, conf=CONF, imgsz=S, half=True)
    second = m._handle(True)
    assert second.value != m._h.value and m._last_handle.value == second.value
    t = _lib.Timing()
    _lib.check(_lib.lib().mi355_yolo_last_timing(second, C.byref(t)))
    assert m.last_timing() == {k: getattr(t, k) for k, _ in _lib.Timing._fields_}
    hsh, src, nl, ab, au = C.c_ulonglong(), C.c_int(), C.c_int(), C.c_longlong(), C.c_longlong()
    _lib.check(_lib.lib().mi355_yolo_plan_info(second, C.byref(hsh), C.byref(src), C.byref(nl), C.byref(ab), C.byref(au)))
    info = m.plan_info()
    assert (info["plan_hash"], info["launches_per_pass"], info["activation_bytes"], info["activation_bytes_unshared"]) == \
           (f"{hsh.value:016x}", nl.value, ab.value, au.value)
