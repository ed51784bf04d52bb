"""Every entry point of the detector gives the rows of a blocking mi355_yolo_infer call on each frame alone.

The host code behind mi355_yolo_infer / _infer_device / _infer_device_async / _infer_multi / _raw_head / _raw_head_multi stages frames,
grows scratch, chunks the call and copies the rows out along three different tails; none of that may show in the rows.  The expected
value of a frame is what a blocking mi355_yolo_infer call returns for that frame alone (test_gpu_e2e.py ties that call to the oracle);
every comparison is on the uint32 view of the rows plus the counts.  Shapes are small (imgsz 96): 64 x 96 is its own canvas
(identity), 80 x 96 is padded only, 48 x 80 is resized and padded, and a 96 x 128 frame beside them makes a call mixed.

Mixed-size calls: a frame alone is never a mixed call (one frame has one shape, so it gets the rect canvas), so the expectation of a
frame in a mixed call is the blocking infer call where the rect canvas of its shape IS the square imgsz x imgsz canvas (80 x 96 and
96 x 128), and for the two other shapes its rows in the smallest mixed call there is: the frame beside one 96 x 128 companion.  That
pair is itself tied to something outside the mixed path: the frame letterboxed alone to the square canvas (mi355_op_letterbox_multi)
and given to the blocking infer call as a 96 x 96 image must keep the same anchors in the same order with the same scores, classes
and keypoint confidences (only the coordinates differ: they are scaled back against another shape), and raw_head of the canvases must
equal raw_head_multi of the mixed frames bit for bit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S = 96
ID, PAD, RS, BIG = (64, 96), (80, 96), (48, 80), (96, 128)
RS2 = (32, 48)        # resized too, onto the canvas of RS (64 x 96) with other tables
CONF = 0.001          # the synthetic checkpoints score low on frames this small: at 0.001 every frame keeps 10 .. 130 rows, at 0.25 most keep none
SENTINEL = 0xA5A5A5A5
EINVAL = -1


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _classes(classes):
    if classes is None:
        return None, 0
    return (C.c_int * len(classes))(*classes), len(classes)


class Eng:
    """One engine handle and the raw C calls on it; every call -> (rc, rows [n, cap, 58] uint32, counts [n])"""

    def __init__(self, case, **kw):
        from cvsd_amd import YOLO, _lib
        self.m = YOLO.from_state_dict(case["name"], case["sd"], **kw)
        self.h, self.lib, self.words = self.m._h, _lib.lib(), _lib.DET_WORDS

    def _out(self, n, cap):
        return np.full((max(n, 1), max(cap, 1), self.words), SENTINEL, np.uint32), np.full(max(n, 1), -7, np.int32)

    def infer(self, frames, conf=CONF, iou=0.7, classes=None, max_det=300, imgsz=S, cap=None, row_stride=0, n=None, h=None, w=None):
        n = frames.shape[0] if n is None else n
        h = frames.shape[1] if h is None else h
        w = frames.shape[2] if w is None else w
        cap = max_det if cap is None else cap
        rows, counts = self._out(n, cap)
        ca, nc = _classes(classes)
        rc = self.lib.mi355_yolo_infer(self.h, frames.ctypes.data, n, h, w, row_stride, conf, iou, ca, nc, max_det, imgsz, rows.ctypes.data, cap,
                                       _i32(counts))
        return rc, rows, counts

    def infer_device(self, frames, conf=CONF, iou=0.7, classes=None, max_det=300, imgsz=S, cap=None):
        n, h, w = frames.shape[:3]
        cap = max_det if cap is None else cap
        rows, counts = self._out(n, cap)
        ca, nc = _classes(classes)
        dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        torch.cuda.synchronize()
        rc = self.lib.mi355_yolo_infer_device(self.h, dev.data_ptr(), n, h, w, conf, iou, ca, nc, max_det, imgsz, rows.ctypes.data, cap,
                                              _i32(counts))
        return rc, rows, counts

    def infer_async(self, frames, conf=CONF, iou=0.7, classes=None, max_det=300, imgsz=S, sync=True):
        """-> (rc, packed rows tensor, counts tensor, total tensor, the frames' tensor): on the device, complete after mi355_yolo_sync"""
        n, h, w = frames.shape[:3]
        dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        rows = torch.full((n * max_det, self.words), -1, dtype=torch.int32, device="cuda")
        counts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        total = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        ca, nc = _classes(classes)
        torch.cuda.synchronize()
        rc = self.lib.mi355_yolo_infer_device_async(self.h, dev.data_ptr(), n, h, w, conf, iou, ca, nc, max_det, imgsz, rows.data_ptr(),
                                                    counts.data_ptr(), total.data_ptr())
        if sync and rc == 0:
            assert self.lib.mi355_yolo_sync(self.h) == 0
        return rc, rows, counts, total, dev

    def infer_multi(self, frames, on_device=False, conf=CONF, iou=0.7, classes=None, max_det=300, imgsz=S, cap=None):
        n = len(frames)
        cap = max_det if cap is None else cap
        if on_device:
            keep = [f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]
            ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in keep])
            strides = np.array([t.stride(0) for t in keep], np.int32)
            torch.cuda.synchronize()
        else:
            keep = frames
            ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in keep])
            strides = np.array([f.strides[0] for f in keep], np.int32)
        hs, ws = np.array([f.shape[0] for f in keep], np.int32), np.array([f.shape[1] for f in keep], np.int32)
        rows, counts = self._out(n, cap)
        ca, nc = _classes(classes)
        rc = self.lib.mi355_yolo_infer_multi(self.h, ptrs, _i32(hs), _i32(ws), _i32(strides), int(on_device), n, conf, iou, ca, nc, max_det, imgsz,
                                             rows.ctypes.data, cap, _i32(counts))
        return rc, rows, counts

    def err(self):
        return self.lib.mi355_last_error().decode()


@pytest.fixture(scope="module", params=["yolov8n", "yolov8n-pose"])
def case(request):
    """the checkpoint, 17 frames of every shape, a reference engine and the cache of per-frame expectations (computed once, left unchanged)"""
    from tools import synth
    name = request.param
    c = {"name": name, "sd": synth.synthetic_checkpoint(name, seed=0)[1], "want": {}}
    c["frames"] = {shape: synth.synthetic_frames(17, shape[0], shape[1], seed=40 + i) for i, shape in enumerate((ID, PAD, RS, BIG, RS2))}
    c["ref"] = Eng(c)
    c["eng"] = {}
    return c


def _eng(case, **kw):
    """engines are shared between the tests of a module run (one per option set): a test must leave no call in flight"""
    key = tuple(sorted(kw.items()))
    if key not in case["eng"]:
        case["eng"][key] = Eng(case, **kw)
    return case["eng"][key]


def _want(case, shape, i, conf=CONF, iou=0.7, classes=None, max_det=300):
    """rows [count, 58] uint32 of frame i of `shape` from a blocking infer call on it alone"""
    key = (shape, i, conf, iou, None if classes is None else tuple(classes), max_det)
    if key not in case["want"]:
        rc, rows, counts = case["ref"].infer(case["frames"][shape][i:i + 1], conf, iou, classes, max_det)
        assert rc == 0, case["ref"].err()
        got = rows[0, :counts[0]].copy()
        got.setflags(write=False)
        case["want"][key] = got
    return case["want"][key]


def _want_mixed(case, shape, i, **kw):
    """a frame's rows on the square canvas: the blocking call alone where the rect canvas is that canvas, else beside one 96 x 128 frame"""
    if shape in (PAD, BIG):
        return _want(case, shape, i, **kw)
    key = ("mixed", shape, i, tuple(sorted(kw.items())))
    if key not in case["want"]:
        rc, rows, counts = case["ref"].infer_multi([case["frames"][shape][i], case["frames"][BIG][0]], **kw)
        assert rc == 0, case["ref"].err()
        np.testing.assert_array_equal(rows[1, :counts[1]], _want(case, BIG, 0, **kw))       # the companion ties the pair to the blocking call
        got = rows[0, :counts[0]].copy()
        # ... and the canvas of the frame alone, as a 96 x 96 image, to the blocking call: same anchors, order, scores, classes, keypoint confidences
        from cvsd_amd import ops
        canvas = ops.letterbox_multi([case["frames"][shape][i]], S)
        rc, crow, ccnt = case["ref"].infer(canvas, **kw)
        assert rc == 0, case["ref"].err()
        same = [4, 5, 6] + list(range(9, 7 + 3 * case["ref"].m.kpt_shape[0], 3))
        assert ccnt[0] == counts[0] and np.array_equal(crow[0, :ccnt[0]][:, same], got[:, same]), f"{shape} frame {i}: the pair differs from its canvas alone"
        got.setflags(write=False)
        case["want"][key] = got
    return case["want"][key]


def _check(res, wants, tag, cap=None):
    """counts, the rows of every frame and the untouched slots behind them"""
    rc, rows, counts = res
    assert rc == 0, tag
    assert len(counts) == len(wants), tag
    for i, w in enumerate(wants):
        c = len(w) if cap is None else min(len(w), cap)
        assert counts[i] == c, f"{tag}: frame {i} has {counts[i]} rows, expected {c}"
        assert np.array_equal(rows[i, :c], w[:c]), f"{tag}: rows of frame {i} differ"
        assert (rows[i, c:] == SENTINEL).all(), f"{tag}: frame {i} wrote past its count"


def _check_async(res, wants, tag):
    rc, rows, counts, total, _ = res
    assert rc == 0, tag
    counts, rows = counts.cpu().numpy(), rows.cpu().numpy().view(np.uint32)
    assert list(counts) == [len(w) for w in wants], tag
    assert int(total.item()) == int(counts.sum()), tag
    at = 0
    for i, w in enumerate(wants):
        assert np.array_equal(rows[at:at + len(w)], w), f"{tag}: packed rows of frame {i} differ"
        at += len(w)


def _wants(case, shape, n, **kw):
    return [_want(case, shape, i, **kw) for i in range(n)]


# ------------------------------------------------------------------------------------------ every entry point gives the same rows
@pytest.mark.parametrize("shape", [ID, PAD, RS])
def test_every_single_shape_entry_point(case, shape):
    e, fr = _eng(case), case["frames"][shape][:3]
    wants = _wants(case, shape, 3)
    assert sum(len(w) for w in wants) > 0
    _check(e.infer(fr), wants, "infer")
    # rows 24 bytes further apart than a row is long, through the raw call
    h, w = shape
    wide = np.full((3, h, w + 8, 3), 77, np.uint8)
    wide[:, :, :w] = fr
    _check(e.infer(wide, row_stride=(w + 8) * 3, w=w), wants, "infer, padded row stride")
    _check(e.infer_device(fr), wants, "infer_device")
    _check_async(e.infer_async(fr), wants, "infer_device_async")
    for dev in (False, True):
        _check(e.infer_multi(list(fr), on_device=dev), wants, f"infer_multi, equal shapes, device={dev}")


@pytest.mark.parametrize("dev", [False, True])
def test_infer_multi_mixed_shapes(case, dev):
    e = _eng(case)
    picks = [(ID, 0), (BIG, 1), (RS, 2), (PAD, 3), (RS, 4), (ID, 5)]
    frames = [case["frames"][s][i] for s, i in picks]
    wants = [_want_mixed(case, s, i) for s, i in picks]
    assert sum(len(w) for w in wants) > 0
    _check(e.infer_multi(frames, on_device=dev), wants, f"mixed shapes, device={dev}")
    if not dev:
        from cvsd_amd import ops
        head = e.m.raw_head(frames, imgsz=S)                              # raw_head_multi on the mixed frames ...
        assert np.array_equal(head.view(np.uint32), e.m.raw_head(ops.letterbox_multi(frames, S), imgsz=S).view(np.uint32))    # ... raw_head on their canvases
        # a view whose rows lie further apart: the staging repacks it
        wide = np.full((48, 100, 3), 9, np.uint8)
        wide[:, 10:90] = case["frames"][RS][2]
        frames[2] = wide[:, 10:90]
        assert frames[2].strides[0] == 300
        _check(e.infer_multi(frames), wants, "mixed shapes, one strided frame")


def _head_query(e, n, h, w, multi):
    ch, an = C.c_int(-1), C.c_int(-1)
    if multi:
        hs, ws = np.full(n, h, np.int32), np.full(n, w, np.int32)
        ptrs = (C.c_void_p * n)(*[8] * n)                                # never read: the shape query leaves before any frame is
        rc = e.lib.mi355_yolo_raw_head_multi(e.h, ptrs, _i32(hs), _i32(ws), None, 0, n, S, None, C.byref(ch), C.byref(an))
    else:
        rc = e.lib.mi355_yolo_raw_head(e.h, None, n, h, w, 0, S, None, C.byref(ch), C.byref(an))
    assert rc == 0, e.err()
    return ch.value, an.value


@pytest.mark.parametrize("shape", [PAD, RS])
def test_raw_head_and_raw_head_multi(case, shape):
    e, fr = _eng(case, batch_chunk=4), case["frames"][shape][:5]         # 5 frames: a tail chunk, both staging slots
    _check(e.infer(case["frames"][ID][:1]), _wants(case, ID, 1), "infer before the queries")
    before = e.m.plan_info()
    q = _head_query(e, 5, shape[0], shape[1], False)
    assert q == _head_query(e, 5, shape[0], shape[1], True)
    assert e.m.plan_info() == before                                      # a query plans, allocates and launches nothing
    one = e.m.raw_head(fr, imgsz=S)
    assert one.shape == (5, q[0], q[1])
    for dev in (False, True):
        src = [torch.from_numpy(f).cuda() for f in fr] if dev else list(fr)
        hs, ws = np.full(5, shape[0], np.int32), np.full(5, shape[1], np.int32)
        ptrs = (C.c_void_p * 5)(*[f.data_ptr() if dev else f.ctypes.data for f in src])
        out = np.full((5, q[0], q[1]), np.nan, np.float32)
        ch, an = C.c_int(), C.c_int()
        torch.cuda.synchronize()
        rc = e.lib.mi355_yolo_raw_head_multi(e.h, ptrs, _i32(hs), _i32(ws), None, int(dev), 5, S, out.ctypes.data, C.byref(ch), C.byref(an))
        assert rc == 0, e.err()
        assert (ch.value, an.value) == q
        assert np.array_equal(out.view(np.uint32), one.view(np.uint32)), f"raw_head_multi (device={dev}) differs from raw_head"
    # a frame's head does not depend on the frames beside it
    assert np.array_equal(e.m.raw_head(fr[4:5], imgsz=S).view(np.uint32), one[4:5].view(np.uint32))


# ------------------------------------------------------------------------------------------ chunking
@pytest.mark.parametrize("n", [1, 4, 5, 9])
def test_chunks_of_four(case, n):
    """n = 5: a tail chunk of one frame; n = 9: three chunks, so both staging slots are used again"""
    e = _eng(case, batch_chunk=4)
    for shape in (RS, PAD):
        fr, wants = case["frames"][shape][:n], _wants(case, shape, n)
        _check(e.infer(fr), wants, f"host frames {shape}")
        _check(e.infer_device(fr), wants, f"device frames {shape}")
    picks = [((ID, RS, BIG, PAD)[i % 4], i) for i in range(n)] if n > 1 else [(BIG, 0)]
    frames = [case["frames"][s][i] for s, i in picks]
    wants = [_want_mixed(case, s, i) if n > 1 else _want(case, s, i) for s, i in picks]
    _check(e.infer_multi(frames), wants, "mixed host frames")
    _check(e.infer_multi(frames, on_device=True), wants, "mixed device frames")


def test_first_chunk_on_several_streams_tail_on_one(case):
    """batch_chunk 8, n = 11: eight frames run along the dependency DAG on several streams, the tail of three in program order"""
    e = _eng(case, batch_chunk=8)
    _check(e.infer(case["frames"][RS][:11]), _wants(case, RS, 11), "host frames")
    _check(e.infer_device(case["frames"][PAD][:11]), _wants(case, PAD, 11), "device frames")


@pytest.mark.parametrize("n", [16, 17])
def test_either_side_of_the_direct_rows_boundary(case, n):
    e = _eng(case, batch_chunk=32)
    _check(e.infer(case["frames"][RS][:n]), _wants(case, RS, n), f"n={n}")
    _check_async(e.infer_async(case["frames"][RS][:n]), _wants(case, RS, n), f"async n={n}")


# ------------------------------------------------------------------------------------------ output tails
def test_copy_tail_equals_direct_rows(case, monkeypatch):
    e = _eng(case, batch_chunk=32)
    for n in (1, 3, 16):
        fr, wants = case["frames"][PAD][:n], _wants(case, PAD, n)
        monkeypatch.setenv("MI355_DIRECT_ROWS", "0")
        _check(e.infer(fr), wants, f"copy tail n={n}")
        monkeypatch.delenv("MI355_DIRECT_ROWS")
        _check(e.infer(fr), wants, f"direct rows n={n}")


def test_more_rows_than_the_speculative_copy_holds(case, monkeypatch):
    """iou 1.0 (nothing is suppressed): more than 64 rows per frame, so the compact tail's second copy runs"""
    e = _eng(case, batch_chunk=32)
    kw = dict(iou=1.0)
    fr, wants = case["frames"][PAD][:3], _wants(case, PAD, 3, **kw)
    total = sum(len(w) for w in wants)
    print("rows kept:", [len(w) for w in wants])
    assert total > 64 * 3
    monkeypatch.setenv("MI355_DIRECT_ROWS", "0")
    _check(e.infer(fr, **kw), wants, "second copy")
    monkeypatch.delenv("MI355_DIRECT_ROWS")
    _check(e.infer(fr, **kw), wants, "direct rows")
    _check(_eng(case, batch_chunk=4).infer(case["frames"][PAD][:5], **kw), _wants(case, PAD, 5, **kw), "two chunks")


def test_capacity_smaller_than_a_count(case, monkeypatch):
    e = _eng(case, batch_chunk=32)
    fr, wants = case["frames"][PAD][:3], _wants(case, PAD, 3)
    cap = max(len(w) for w in wants) - 1                                 # at least one frame is clipped; a frame with fewer rows keeps sentinels
    assert cap >= 1
    monkeypatch.setenv("MI355_DIRECT_ROWS", "0")
    _check(e.infer(fr, cap=cap), wants, "copy tail", cap=cap)
    monkeypatch.delenv("MI355_DIRECT_ROWS")
    _check(e.infer(fr, cap=cap), wants, "direct rows", cap=cap)
    _check(e.infer_multi(list(fr), cap=cap), wants, "infer_multi", cap=cap)


# ------------------------------------------------------------------------------------------ filters
def test_filters(case):
    e, fr = _eng(case), case["frames"][RS][:3]
    nc = e.m.nc
    ids = [0] if nc == 1 else [3, 5, 10, 13]
    kw = dict(classes=ids)
    wants = _wants(case, RS, 3, **kw)
    assert sum(len(w) for w in wants) > 0
    _check(e.infer(fr, **kw), wants, "class list")
    _check(e.infer(fr, classes=[-1] + ids + [nc, nc + 40]), wants, "ids below 0 and at or above nc are ignored")
    _check_async(e.infer_async(fr, classes=[-5] + ids + [nc]), wants, "async, class list")
    if nc > 1:
        assert any(len(a) != len(b) for a, b in zip(wants, _wants(case, RS, 3))), "the class list filters nothing on these frames"
    wants5 = _wants(case, RS, 3, max_det=5)
    assert all(len(w) == 5 for w in wants5)
    _check(e.infer(fr, max_det=5), wants5, "max_det 5")
    _check(e.infer_device(fr, max_det=5), wants5, "max_det 5, device frames")
    _check(_eng(case, batch_chunk=4).infer(case["frames"][RS][:5], max_det=5), _wants(case, RS, 5, max_det=5), "max_det 5, two chunks")
    res = e.infer(fr, conf=1.0)
    _check(res, [np.zeros((0, e.words), np.uint32)] * 3, "conf 1.0")
    assert not res[2].any()


# ------------------------------------------------------------------------------------------ one handle, many calls
def test_one_handle_grows_every_buffer(case):
    e = Eng(case, batch_chunk=4)
    for n in (1, 9, 1):
        _check(e.infer(case["frames"][RS][:n]), _wants(case, RS, n), f"host n={n}")
    e = Eng(case, batch_chunk=4)
    for n in (1, 9, 1):
        picks = [((BIG, RS, ID, PAD)[i % 4], i) for i in range(n)]
        wants = [_want_mixed(case, s, i) if n > 1 else _want(case, s, i) for s, i in picks]
        _check(e.infer_multi([case["frames"][s][i] for s, i in picks]), wants, f"mixed n={n}")


def test_async_then_blocking_then_raw_head(case):
    e = _eng(case)
    fr = case["frames"][PAD]
    res = e.infer_async(fr[:3], classes=[0], sync=False)                  # its class mask and row slots are still in use ...
    _check(e.infer(fr[3:5]), [_want(case, PAD, 3), _want(case, PAD, 4)], "blocking call behind an asynchronous one")      # ... when this call comes
    _check_async(res, _wants(case, PAD, 3, classes=[0]), "the asynchronous call")
    head = e.m.raw_head(fr[:2], imgsz=S)
    assert np.array_equal(head.view(np.uint32), _eng(case, batch_chunk=4).m.raw_head(fr[:2], imgsz=S).view(np.uint32))
    res = e.infer_async(fr[:3], sync=False)
    head_m = e.m.raw_head([fr[0], fr[1]], imgsz=S)
    assert e.lib.mi355_yolo_sync(e.h) == 0
    _check_async(res, _wants(case, PAD, 3), "asynchronous call in front of raw_head_multi")
    assert np.array_equal(head_m.view(np.uint32), head.view(np.uint32))


def test_raw_head_on_other_resize_tables_behind_an_async_call(case):
    """An asynchronous call of three chunks on resized frames, then at once raw_head on another resized shape with the same canvas
    and the same frames per pass: nothing replans, and the new resize tables must not reach the device before the pending chunks'
    letterbox launches have read the old ones."""
    e = _eng(case, batch_chunk=4)
    fr, other = case["frames"][RS][:9], case["frames"][RS2][:5]
    want_head = _eng(case).m.raw_head(other, imgsz=S)
    for k in range(3):
        res = e.infer_async(fr, sync=False)
        head = e.m.raw_head(other, imgsz=S)
        assert e.lib.mi355_yolo_sync(e.h) == 0
        _check_async(res, _wants(case, RS, 9), f"asynchronous call in front of raw_head, round {k}")
        assert np.array_equal(head.view(np.uint32), want_head.view(np.uint32))
        _check(e.infer(fr[:5]), _wants(case, RS, 5), f"the tables of the first shape again, round {k}")


def test_equal_and_mixed_calls_alternate(case):
    e = _eng(case, batch_chunk=4)
    mixed = [(RS, 0), (BIG, 1), (ID, 2), (PAD, 3), (RS, 4)]
    for k in range(2):
        _check(e.infer(case["frames"][RS][:5]), _wants(case, RS, 5), f"equal shapes, round {k}")
        _check(e.infer_multi([case["frames"][s][i] for s, i in mixed]), [_want_mixed(case, s, i) for s, i in mixed], f"mixed, round {k}")
        _check(e.infer_multi(list(case["frames"][ID][:5])), _wants(case, ID, 5), f"infer_multi, equal shapes, round {k}")
        mixed = mixed[1:] + mixed[:1]                                       # other frames in the descriptors: they are uploaded again


def test_sparse_box_branch_on_and_off(case, monkeypatch):
    """MI355_SPARSE_BOX=1 against 0 at batch_chunk 4, n = 5: the sparse tail on a full chunk and on a tail chunk of one frame"""
    fr, wants = case["frames"][PAD][:5], _wants(case, PAD, 5)
    mixed = [(RS, 0), (BIG, 1), (ID, 2), (PAD, 3), (RS, 4)]
    for flag in ("1", "0"):
        monkeypatch.setenv("MI355_SPARSE_BOX", flag)
        e = Eng(case, batch_chunk=4)
        _check(e.infer(fr), wants, f"MI355_SPARSE_BOX={flag}")
        _check(e.infer_device(fr), wants, f"MI355_SPARSE_BOX={flag}, device frames")
        _check(e.infer_multi([case["frames"][s][i] for s, i in mixed]), [_want_mixed(case, s, i) for s, i in mixed], f"MI355_SPARSE_BOX={flag}, mixed")
        st = e.m.sparse_stats()                                            # of the shape last run
        if flag == "0":
            assert not st["enabled"] and st["passes"] == 0, st
        else:                       # shapes this small are sometimes tuned to an unfused cv2.i.1, which keeps the dense head: see below
            assert st["enabled"] or st["dense_because"].startswith("plan of"), st
    if case["name"] != "yolov8n":
        return
    # YOLOv8n at 4 x 640 x 640 and 1 x 640 x 640 runs the shipped launch plans, with which the sparse tail is on: a full chunk and a tail chunk of one
    from tools import synth
    big = synth.synthetic_frames(5, 640, 640, seed=1000)
    monkeypatch.setenv("MI355_SPARSE_BOX", "0")
    ref = Eng(case)
    wants = []
    for i in range(5):
        rc, rows, counts = ref.infer(big[i:i + 1], conf=0.25, imgsz=640)
        assert rc == 0, ref.err()
        wants.append(rows[0, :counts[0]].copy())
    assert sum(len(w) for w in wants) > 0
    monkeypatch.setenv("MI355_SPARSE_BOX", "1")
    e = Eng(case, batch_chunk=4)
    _check(e.infer(big, conf=0.25, imgsz=640), wants, "MI355_SPARSE_BOX=1 at 640")
    st = e.m.sparse_stats()
    assert st["enabled"] and st["passes"] == 2 and st["dense_fallbacks"] == 0, st


# ------------------------------------------------------------------------------------------ profiling
def test_profiling_leaves_the_rows_alone_and_survives_raw_head(case):
    e = Eng(case, batch_chunk=4)
    fr, wants = case["frames"][RS][:5], _wants(case, RS, 5)
    e.m.set_profiling(True)
    _check(e.infer(fr), wants, "profiling on")
    t = e.m.last_timing()
    assert t["frames"] == 5 and t["conv_launches"] > 0 and t["total_ms"] > 0, t
    for multi in (False, True):
        head = e.m.raw_head(list(fr[:2]) + ([case["frames"][BIG][0]] if multi else []), imgsz=S)
        assert np.isfinite(head).all()
        _check(e.infer(fr[:1]), wants[:1], "profiling on, after raw_head")
        t = e.m.last_timing()
        assert t["frames"] == 1 and t["conv_launches"] > 0, t               # raw_head put profiling back
    _check(e.infer_multi([fr[0], case["frames"][BIG][0]]), [_want_mixed(case, RS, 0), _want(case, BIG, 0)], "profiling on, mixed")
    assert e.m.last_timing()["letterbox_ms"] > 0
    e.m.set_profiling(False)
    _check(e.infer(fr), wants, "profiling off again")


# ------------------------------------------------------------------------------------------ refusals
def _refusals(fr, rows, counts, dev_ok):
    """(entry point, arguments, message): one row per check of infer_impl and of multi_check, in the order the checks run; the rows
    marked 'two rules' break a later rule as well and must get the earlier rule's message"""
    f, r, c = fr.ctypes.data, rows.ctypes.data, _i32(counts)
    n, (h, w) = 2, fr.shape[1:3]
    hs, ws = np.array([h, h], np.int32), np.array([w, w], np.int32)
    bad_h, bad_w = np.array([h, 0], np.int32), np.array([w, -1], np.int32)
    short = np.array([0, w * 3 - 1], np.int32)
    ptrs = (C.c_void_p * 2)(f, f + fr[0].nbytes)
    hole = (C.c_void_p * 2)(f, None)
    cl = (C.c_int * 1)(0)
    I = lambda a: _i32(a)
    return [
        ("infer", (None, n, h, w, 0, .25, .7, None, 0, 300, S, r, 300, c), "null argument"),
        ("infer", (f, n, h, w, 0, .25, .7, None, 0, 300, S, None, 300, c), "null argument"),
        ("infer", (f, n, h, w, 0, .25, .7, None, 0, 300, S, r, 300, None), "null argument"),
        ("infer", (None, 0, h, w, 0, .25, .7, None, 0, 300, S, r, 300, c), "null argument"),                       # two rules
        ("async", (dev_ok, n, h, w, .25, .7, None, 0, 300, S, None, dev_ok, dev_ok), "null argument"),
        ("async", (dev_ok, n, h, w, .25, .7, None, 0, 300, S, dev_ok, None, dev_ok), "null argument"),
        ("async", (dev_ok, n, h, w, .25, .7, None, 0, 300, S, dev_ok, dev_ok, None), "null argument"),
        ("multi", (ptrs, I(hs), I(ws), None, 0, n, .25, .7, None, 0, 300, S, None, 300, c), "null argument"),
        ("multi", (ptrs, I(hs), I(ws), None, 0, 0, .25, .7, None, 0, 300, S, r, 300, c), "n must be positive"),
        ("multi", (ptrs, None, I(ws), None, 0, -1, .25, .7, None, 0, 300, S, r, 300, c), "n must be positive"),    # two rules
        ("multi", (None, I(hs), I(ws), None, 0, n, .25, .7, None, 0, 300, S, r, 300, c), "null argument"),
        ("multi", (ptrs, None, I(ws), None, 0, n, .25, .7, None, 0, 300, S, r, 300, c), "null argument"),
        ("multi", (ptrs, I(hs), None, None, 0, n, .25, .7, None, 0, 300, S, r, 300, c), "null argument"),
        ("multi", (hole, I(hs), I(ws), None, 0, n, .25, .7, None, 0, 300, S, r, 300, c), "null frame pointer"),
        ("multi", (hole, I(bad_h), I(ws), None, 0, n, .25, .7, None, 0, 300, S, r, 300, c), "null frame pointer"), # two rules
        ("multi", (ptrs, I(bad_h), I(ws), None, 0, n, .25, .7, None, 0, 300, S, r, 300, c), "frame height and width must be positive"),
        ("multi", (ptrs, I(hs), I(bad_w), None, 0, n, .25, .7, None, 0, 300, S, r, 300, c), "frame height and width must be positive"),
        ("multi", (ptrs, I(hs), I(ws), I(short), 0, n, .25, .7, None, 0, 300, S, r, 300, c), "row_stride_bytes smaller than a row"),
        ("multi", (ptrs, I(hs), I(ws), I(short), 0, n, .25, .7, None, 0, 2000, S, r, 300, c), "row_stride_bytes smaller than a row"),  # two rules
        ("infer", (f, 0, h, w, 0, .25, .7, None, 0, 300, S, r, 300, c), "n, height and width must be positive"),
        ("infer", (f, n, 0, w, 0, .25, .7, None, 0, 300, S, r, 300, c), "n, height and width must be positive"),
        ("infer", (f, n, h, -3, 0, .25, .7, None, 0, 300, S, r, 300, c), "n, height and width must be positive"),
        ("infer", (f, 0, h, w, 0, .25, .7, None, 0, 2000, S, r, 300, c), "n, height and width must be positive"),  # two rules
        ("device", (dev_ok, -1, h, w, .25, .7, None, 0, 300, S, r, 300, c), "n, height and width must be positive"),
        ("infer", (f, n, h, w, 0, .25, .7, None, 0, 1025, S, r, 300, c), "max_det must be <= 1024"),
        ("infer", (f, n, h, w, 0, .25, .7, None, 0, 2000, S, r, 0, c), "max_det must be <= 1024"),                 # two rules
        ("multi", (ptrs, I(hs), I(ws), None, 0, n, .25, .7, None, 0, 1025, S, r, 300, c), "max_det must be <= 1024"),
        ("infer", (f, n, h, w, 0, .25, .7, None, 0, 300, S, r, 0, c), "out_capacity_per_image must be >= 1"),
        ("infer", (f, n, h, w, 0, .25, .7, None, 0, 300, 100, r, -2, c), "out_capacity_per_image must be >= 1"),   # two rules
        ("infer", (f, n, h, w, 0, .25, .7, None, 0, 300, 100, r, 300, c), "imgsz must be a multiple of 32"),
        ("infer", (f, n, h, w, w * 3 - 1, .25, .7, None, 0, 300, 100, r, 300, c), "imgsz must be a multiple of 32"),   # two rules
        ("async", (dev_ok, n, h, w, .25, .7, None, 0, 300, 100, dev_ok, dev_ok, dev_ok), "imgsz must be a multiple of 32"),
        ("infer", (f, n, h, w, w * 3 - 1, .25, .7, None, 0, 300, S, r, 300, c), "row_stride_bytes smaller than a row"),
        ("infer", (f, n, h, w, 1, .25, .7, None, -1, 300, S, r, 300, c), "row_stride_bytes smaller than a row"),   # two rules
        ("infer", (f, n, h, w, 0, .25, .7, None, -1, 300, S, r, 300, c), "bad classes argument"),
        ("infer", (f, n, h, w, 0, .25, .7, None, 2, 300, S, r, 300, c), "bad classes argument"),
        ("infer", (f, n, h, w, 0, .25, .7, cl, -1, 300, S, r, 300, c), "bad classes argument"),
        ("multi", (ptrs, I(hs), I(ws), None, 0, n, .25, .7, None, 1, 300, S, r, 300, c), "bad classes argument"),
    ], (hs, ws, bad_h, bad_w, short, ptrs, hole, cl)


def test_refusals_in_order_and_the_next_call_is_sound(case):
    e = _eng(case, batch_chunk=4)
    fr, wants = case["frames"][RS][:2], _wants(case, RS, 2)
    rows, counts = e._out(2, 300)
    dev_ok = torch.zeros(2 * 300 * e.words, dtype=torch.int32, device="cuda")
    table, keep = _refusals(fr, rows, counts, dev_ok.data_ptr())
    fns = {"infer": e.lib.mi355_yolo_infer, "device": e.lib.mi355_yolo_infer_device, "async": e.lib.mi355_yolo_infer_device_async,
           "multi": e.lib.mi355_yolo_infer_multi}
    _check(e.infer(fr), wants, "before the refusals")
    for k, (fn, args, msg) in enumerate(table):
        rc = fns[fn](e.h, *args)
        assert (rc, e.err()) == (EINVAL, msg), f"refusal {k} ({fn}): got {rc}, {e.err()!r}; expected {msg!r}"
        assert (rows == SENTINEL).all() and (counts == -7).all(), f"refusal {k} wrote to the outputs"
        _check(e.infer(fr) if k % 2 else e.infer_multi(list(fr)), wants, f"after refusal {k}")
    # the raw_head entry points: their own checks in their own order
    ch, an = C.c_int(), C.c_int()
    q = lambda *a: e.lib.mi355_yolo_raw_head(e.h, *a)
    out = np.empty(1 << 16, np.float32)
    assert (q(fr.ctypes.data, 2, 48, 80, 0, S, out.ctypes.data, None, C.byref(an)), e.err()) == (EINVAL, "null argument")
    assert (q(fr.ctypes.data, 0, 48, 80, 0, 100, out.ctypes.data, C.byref(ch), C.byref(an)), e.err()) == (EINVAL, "n, height and width must be positive")
    assert (q(fr.ctypes.data, 2, 48, 80, 0, 100, out.ctypes.data, C.byref(ch), C.byref(an)), e.err()) == (EINVAL, "imgsz must be a multiple of 32")
    assert q(None, 2, 48, 80, 0, S, None, C.byref(ch), C.byref(an)) == 0                     # the shape query does not look at bgr ...
    assert (q(None, 2, 48, 80, 0, S, out.ctypes.data, C.byref(ch), C.byref(an)), e.err()) == (EINVAL, "null argument")       # ... the run does
    hs, ws, ptrs = keep[0], keep[1], keep[5]
    qm = lambda *a: e.lib.mi355_yolo_raw_head_multi(e.h, *a)
    assert (qm(ptrs, _i32(hs), _i32(ws), None, 0, 2, S, out.ctypes.data, C.byref(ch), None), e.err()) == (EINVAL, "null argument")
    assert (qm(ptrs, _i32(hs), _i32(ws), None, 0, 0, 100, None, C.byref(ch), C.byref(an)), e.err()) == (EINVAL, "n must be positive")
    assert (qm(keep[6], _i32(hs), _i32(ws), None, 0, 2, 100, None, C.byref(ch), C.byref(an)), e.err()) == (EINVAL, "null frame pointer")
    assert (qm(ptrs, _i32(hs), _i32(ws), None, 0, 2, 100, None, C.byref(ch), C.byref(an)), e.err()) == (EINVAL, "imgsz must be a multiple of 32")
    _check(e.infer(fr), wants, "after the raw_head refusals")
