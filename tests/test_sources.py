"""cvsd_amd.sources: what every kind of source becomes, tiled (by pointer) and untiled, and the detector arguments of a call.

One table, (source kind) x (by_pointer False / True), of tiny frames (4 x 8 and 6 x 10).  Every expectation is a literal: the batch kind
(a plain array / tensor of a given shape, Ragged, YuvBatch), n, the (h, w) list, the row strides, whether a frame is read where it lies
(pointer identity) or from a dense copy, and what the originals are.  Dense against by-pointer decides the letterbox and so the rows;
the originals decide ``Results.orig_img``.  No GPU is touched.
"""
import inspect

import numpy as np
import pytest
import torch

from cvsd_amd import YOLO, YUVFrame, sources


def _frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


A, A2, B = _frame(4, 8, 0), _frame(4, 8, 1), _frame(6, 10, 2)
PAIR = np.stack([A, A2])                                        # [2, 4, 8, 3]
WIDE = _frame(4, 12, 3)
SLICE = WIDE[:, 2:10]                                           # a column slice: rows 36 bytes apart, pixels dense
MIRROR = A[:, ::-1]                                             # pixel stride -3: no pointer + pitch describes it
TA, TA2, TB = torch.from_numpy(A.copy()), torch.from_numpy(A2.copy()), torch.from_numpy(B.copy())
TPAIR = torch.from_numpy(PAIR.copy())
YA = YUVFrame(np.full((4, 8), 90, np.uint8), uv=np.full((2, 8), 128, np.uint8))
YB = YUVFrame(np.full((6, 10), 90, np.uint8), u=np.full((3, 5), 128, np.uint8), v=np.full((3, 5), 128, np.uint8), fmt="i420")

S48, S610 = (4, 8), (6, 10)


def dense(kind, shape, copied, orig):
    return {"kind": kind, "shape": shape, "copied": copied, "orig": orig}


def ragged(shapes, strides, copied, orig):
    return {"kind": "ragged", "shapes": shapes, "strides": strides, "copied": copied, "orig": orig}


def yuv(shapes):
    return {"kind": "yuv", "shapes": shapes}


# orig: "none" = None; "same" = the caller's own objects; "views" = arrays over the source's memory
# id, source, its frames one by one, {by_pointer: expectation or exception class}
ACCEPTED = [
    ("array-3d", A, [A], {False: dense("array", (1, 4, 8, 3), False, "views"), True: ragged([S48], [24], [False], "same")}),
    ("array-4d", PAIR, [PAIR[0], PAIR[1]], {False: dense("array", (2, 4, 8, 3), False, "views"),
                                            True: ragged([S48, S48], [24, 24], [False, False], "views")}),
    ("column-slice", SLICE, [SLICE], {False: dense("array", (1, 4, 8, 3), True, "views"), True: ragged([S48], [36], [False], "same")}),
    ("negative-stride", MIRROR, [MIRROR], {False: dense("array", (1, 4, 8, 3), True, "views"), True: ragged([S48], [24], [True], "same")}),
    ("list-one-shape", [A, A2], [A, A2], {False: dense("array", (2, 4, 8, 3), True, "same"),
                                          True: ragged([S48, S48], [24, 24], [False, False], "same")}),
    ("list-two-shapes", [A, B], [A, B], {False: ragged([S48, S610], [24, 30], [False, False], "same"),
                                         True: ragged([S48, S610], [24, 30], [False, False], "same")}),
    ("list-with-slice", [SLICE, B], [SLICE, B], {False: ragged([S48, S610], [36, 30], [False, False], "same"),
                                                 True: ragged([S48, S610], [36, 30], [False, False], "same")}),
    ("tuple", (B, A), [B, A], {False: ragged([S610, S48], [30, 24], [False, False], "same"),
                               True: ragged([S610, S48], [30, 24], [False, False], "same")}),
    ("cpu-tensor-3d", TA, [TA], {False: ValueError, True: ragged([S48], [24], [False], "views")}),
    ("cpu-tensor-4d", TPAIR, [TPAIR[0], TPAIR[1]], {False: dense("tensor", (2, 4, 8, 3), False, "none"),
                                                    True: ragged([S48, S48], [24, 24], [False, False], "views")}),
    ("list-of-cpu-tensors", [TA, TB], [TA, TB], {False: ragged([S48, S610], [24, 30], [False, False], "same"),
                                                 True: ragged([S48, S610], [24, 30], [False, False], "views")}),
    ("list-of-cpu-tensors-one-shape", [TA, TA2], [TA, TA2], {False: dense("array", (2, 4, 8, 3), True, "same"),
                                                             True: ragged([S48, S48], [24, 24], [False, False], "views")}),
    ("yuv-frame", YA, [YA], {False: yuv([S48]), True: yuv([S48])}),
    ("list-of-yuv-frames", [YA, YB], [YA, YB], {False: yuv([S48, S610]), True: yuv([S48, S610])}),
]

REFUSED = [
    ("wrong-dtype", A.astype(np.float32), ValueError),
    ("wrong-dtype-in-list", [A.astype(np.int8), B], ValueError),
    ("wrong-last-dimension", np.zeros((4, 8, 4), np.uint8), ValueError),
    ("wrong-last-dimension-tensor", torch.zeros((2, 4, 8, 1), dtype=torch.uint8), ValueError),
    ("empty-list", [], ValueError),
    ("yuv-and-bgr", [YA, A], ValueError),
    ("bgr-and-yuv", [A, YA], ValueError),
    ("str", "clip.mp4", TypeError),
    ("none", None, TypeError),
]


def _ptr(x):
    return x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data


def _pixels(x):
    return x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _check_originals(originals, frames, how):
    if how == "none":
        assert originals is None
        return
    assert isinstance(originals, list) and len(originals) == len(frames)
    for o, f in zip(originals, frames):
        if how == "same":
            assert o is f
        else:
            assert isinstance(o, np.ndarray) and o.ctypes.data == _ptr(f) and o.shape == tuple(f.shape)


@pytest.mark.parametrize("by_pointer", [False, True], ids=["untiled", "tiled"])
@pytest.mark.parametrize("source, frames, want", [c[1:] for c in ACCEPTED], ids=[c[0] for c in ACCEPTED])
def test_as_batch_table(source, frames, want, by_pointer):
    want = want[by_pointer]
    if isinstance(want, type):
        with pytest.raises(want):
            sources.as_batch(source, by_pointer=by_pointer)
        return
    batch, originals = sources.as_batch(source, by_pointer=by_pointer)
    if want["kind"] == "yuv":
        assert isinstance(batch, sources.YuvBatch) and originals is None
        assert batch.n == len(frames) and batch.shape == (len(frames),) and batch.shapes == want["shapes"] and batch.on_device is False
        assert all(kept is f for kept, f in zip(batch.frames, frames))
        assert [(s.height, s.width) for s in batch.structs] == want["shapes"] and batch.structs[0].y == frames[0].y.ctypes.data
        return
    if want["kind"] == "ragged":
        assert isinstance(batch, sources.Ragged) and batch.raw is False and batch.on_device is False
        assert batch.n == len(frames) and batch.shape == (len(frames),) and batch.shapes == want["shapes"]
        assert batch.row_strides.tolist() == want["strides"]
        assert batch.heights.tolist() == [s[0] for s in want["shapes"]] and batch.widths.tolist() == [s[1] for s in want["shapes"]]
        for i, f in enumerate(frames):
            assert (batch.ptrs[i] != _ptr(f)) == want["copied"][i], f"frame {i}"
            assert batch.ptrs[i] == batch.frames[i].ctypes.data and np.array_equal(batch.frames[i], _pixels(f))
        assert batch.args()[4:] == (0, len(frames))
    else:
        assert type(batch) is (torch.Tensor if want["kind"] == "tensor" else np.ndarray)
        assert tuple(batch.shape) == want["shape"] and (batch.is_contiguous() if want["kind"] == "tensor" else batch.flags.c_contiguous)
        assert (_ptr(batch) != _ptr(frames[0])) == want["copied"]
        assert np.array_equal(_pixels(batch), np.stack([_pixels(f) for f in frames]))
    _check_originals(originals, frames, want["orig"])


@pytest.mark.parametrize("by_pointer", [False, True], ids=["untiled", "tiled"])
@pytest.mark.parametrize("source, exc", [c[1:] for c in REFUSED], ids=[c[0] for c in REFUSED])
def test_as_batch_refuses(source, exc, by_pointer):
    with pytest.raises(exc):
        sources.as_batch(source, by_pointer=by_pointer)


def test_facade_names_are_the_module_s():
    assert YOLO._Ragged is sources.Ragged and YOLO._DeviceFrames is sources.DeviceFrames and YOLO._YuvBatch is sources.YuvBatch
    batch, originals = YOLO._as_batch([A, B])
    assert isinstance(batch, YOLO._Ragged) and originals[1] is B
    dev = YOLO._RaggedDevice([4096, 8192], [S48, S610])
    assert isinstance(dev, sources.Ragged) and dev.raw is True and dev.on_device is True and dev.n == 2 and dev.shape == (2,)
    assert dev.shapes == [S48, S610] and dev.row_strides.tolist() == [24, 30] and [dev.ptrs[0], dev.ptrs[1]] == [4096, 8192]
    assert dev.args()[4:] == (1, 2)
    one = YOLO._DeviceFrames(4096, 3, 4, 8)
    assert one.raw is True and one.on_device is True and one.n == 3 and one.shape == (3, 4, 8, 3) and one.shapes == [S48] * 3
    for raw in (dev, one):
        sources.ready(raw, 0)                                   # raw pointers: nothing to check or wait for, no GPU is touched
    sources.ready(PAIR, 0)
    sources.ready(TPAIR, 0)


def test_bgr_view_edge_rules():
    v = sources.bgr_view(SLICE)
    assert v.keep is SLICE and (v.ptr, v.pitch, v.hw, v.on_device) == (SLICE.ctypes.data, 36, S48, False)
    d = sources.bgr_view(SLICE, dense=True)                      # track_cameras: C-contiguous frames only
    assert d.keep is not SLICE and d.pitch == 24 and np.array_equal(d.keep, SLICE)
    assert sources.bgr_view(A, dense=True).keep is A
    odd = np.lib.stride_tricks.as_strided(np.zeros(0, np.uint8), (0, 8, 3), (5, 3, 1))
    assert sources.bgr_view(odd, empty_ok=True)[:4] == (odd, odd.ctypes.data, 5, (0, 8))      # render / JPEG entries: passed on as it is
    f = sources.DeviceFrame(4096, 4, 8, pitch=64)
    assert tuple(sources.bgr_view(f)) == (f, 4096, 64, S48, True)
    for bad in (A.astype(np.float32), np.zeros((4, 8), np.uint8), np.zeros((4, 8, 4), np.uint8)):
        with pytest.raises(ValueError):
            sources.bgr_view(bad)


DET_ARGS = [
    ("defaults", dict(), dict(conf=0.25, iou=0.7, classes=None, max_det=300, imgsz=640, half=None, feats=None)),
    ("imgsz-pair", dict(imgsz=(96, 128)), dict(imgsz=128)),
    ("imgsz-list", dict(imgsz=[128, 96]), dict(imgsz=128)),
    ("one-class", dict(classes=3), dict(classes=[3])),
    ("class-list", dict(classes=[0, 2]), dict(classes=[0, 2])),
    ("no-classes", dict(classes=None), dict(classes=None)),
    ("all-given", dict(iou=0.5, max_det=7, imgsz=96, half=True, feats=False), dict(iou=0.5, max_det=7, imgsz=96, half=True, feats=False)),
]


@pytest.mark.parametrize("given, want", [c[1:] for c in DET_ARGS], ids=[c[0] for c in DET_ARGS])
def test_det_args_table(given, want):
    a = sources.det_args(0.25, **given)
    want = {**DET_ARGS[0][2], **want}
    arr, count = a.classes
    got_classes = None if arr is None else list(arr)
    assert got_classes == want["classes"] and count == (0 if want["classes"] is None else len(want["classes"]))
    assert (a.conf, a.iou, a.max_det, a.imgsz, a.half, a.feats) == tuple(want[k] for k in ("conf", "iou", "max_det", "imgsz", "half", "feats"))
    assert type(a.max_det) is int and type(a.imgsz) is int and type(a.conf) is float
    again = sources.det_args(*a)                                # resolved once: a resolved record passes through unchanged
    assert again == a and again.classes[0] is arr


def test_defaults_come_from_one_place():
    assert (sources.IOU, sources.MAX_DET, sources.IMGSZ) == (0.7, 300, 640)
    for fn in (YOLO.predict, YOLO.infer_async, YOLO.detect_rows):
        p = inspect.signature(fn).parameters
        assert (p["iou"].default, p["max_det"].default, p["imgsz"].default) == (0.7, 300, 640), fn.__name__
    a = sources.det_args_from(0.1, {"iou": 0.5, "tile": 96, "stream": True, "verbose": False})      # track's keywords: the others are not its business
    assert (a.conf, a.iou, a.max_det, a.imgsz, a.classes) == (0.1, 0.5, 300, 640, (None, 0))
