"""The motion gate's host twin (``MotionGate(device=None)``, ``ops.motion_grid(device=-1)``: the routine of csrc/motion_grid.h in host
loops) against the numpy statement of tests/_motion_numpy.py: sums, flags, ``changed`` and ``moving`` exact over scripted sequences.
No GPU is touched."""
import numpy as np
import pytest

import _motion_cases as K
import _motion_numpy as M
from cvsd_amd import MotionGate, YUVFrame, ops
from tools import synth


def _gate(n, **kw):
    return MotionGate(n, device=None, **kw)


def _sums(frames, block):
    return ops.motion_grid(frames, block, device=-1)


@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("block", K.BLOCKS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scripted_sequence_matches_numpy(shape, block, layout):
    kw, ticks = K.scripted(shape[0], shape[1], block, layout)
    K.check_scripted(K.run(_gate, _sums, kw, ticks))


@pytest.mark.parametrize("level", [0.0, 1.3, 7.96875, 100.0])
def test_threshold_is_strict_at_other_levels(level):
    kw, ticks = K.scripted(97, 131, 16, "pitched", level=level)
    K.check_scripted(K.run(_gate, _sums, kw, ticks))


def _nv12(y, seed=0):
    h, w = y.shape
    return YUVFrame(y, uv=np.random.default_rng(seed).integers(0, 256, (h // 2, w), dtype=np.uint8), fmt="nv12")


def test_reset_min_blocks_zero_and_format_switch():
    a = K.scene(240, 320, 16, 5)
    y = np.ascontiguousarray(M.luma(a).astype(np.uint8))           # the same luma as a Y plane: only the format differs
    yuv = _nv12(y)
    i420 = YUVFrame(K.lay(y, "pitched"), u=np.zeros((120, 160), np.uint8), v=np.zeros((120, 160), np.uint8), fmt="i420")
    ticks = [[a], [a], [a], [yuv], [yuv], [i420], [a], [a], [None], [a], [a], [a]]
    out = K.run(_gate, _sums, dict(block=16, level=2.0, min_blocks=4, max_skip=None), ticks, resets={2: 0, 10: None})
    mv = [bool(o[0][0]) for o in out]
    # first frame; repeat; reset -> moves; BGR -> YUV moves though the luma is the same; repeat; NV12 -> I420 is the same luma: static;
    # YUV -> BGR moves; repeat; absent; repeat; reset of every camera -> moves; repeat
    assert mv == [True, False, True, True, False, False, True, False, False, False, True, False]
    assert [int(o[1][0]) for o in out][3] == 15 * 20                  # no reference: every block is flagged
    always = K.run(_gate, _sums, dict(block=8, level=2.0, min_blocks=0, max_skip=30), [[a, None]] * 3 + [[a, a]] * 9)
    assert all(o[0][0] for o in always) and [int(o[1][0]) for o in always][1:] == [0] * 11
    assert not any(o[0][1] for o in always[:3]) and all(o[1][1] == -1 for o in always[:3])


def test_max_skip_none_never_forces_and_drift_accumulates():
    a = K.scene(64, 64, 16, 9)
    # block (0, 0) drifts by 100 of luma sum per tick: below the threshold of 2 * 256 = 512 against the reference until tick 6
    ticks = [[K.bump(a, 16, 100 * t)] for t in range(12)]
    out = K.run(_gate, _sums, dict(block=16, level=2.0, min_blocks=1, max_skip=None), ticks)
    assert [bool(o[0][0]) for o in out] == [True] + [False] * 5 + [True] + [False] * 5


@pytest.mark.parametrize("shape", [(240, 320), (200, 300), (97, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_synthetic_clip_alternates_static_and_moving(shape):
    """tools/synth.synthetic_clip repeats its scene pairwise under a little noise: at the default options the second frame of a pair is
    static (no block changed) and the first of the next pair moves"""
    clip = synth.synthetic_clip(12, shape[0], shape[1], seed=3)
    out = K.run(_gate, _sums, dict(block=16, level=2.0, min_blocks=4, max_skip=30), [[f] for f in clip])
    ch = [int(o[1][0]) for o in out]
    mv = [bool(o[0][0]) for o in out]
    assert mv == [t % 2 == 0 for t in range(12)], (mv, ch)
    assert all(c == 0 for c in ch[1::2]) and all(c >= 4 for c in ch[2::2]), ch


def test_refusals():
    for kw in (dict(block=12), dict(block=0), dict(block=16.0), dict(level=-1), dict(level=256), dict(level=float("nan")), dict(level="x"),
               dict(min_blocks=-1), dict(min_blocks=1.5), dict(max_skip=-1), dict(max_skip=2.5)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            MotionGate(2, device=None, **kw)
    for n in (0, 65, -3, 1.0):
        with pytest.raises(ValueError, match="n_cameras"):
            MotionGate(n, device=None)
    g = MotionGate(2, device=None)
    a = K.scene(20, 20, 16, 0)
    with pytest.raises(ValueError, match="2 frames"):
        g.update([a])
    for bad in (a[:, :, 0], a.astype(np.float32), a[:, :, :2], np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            g.update([bad, None])
    for cam in (-1, 2):
        with pytest.raises(ValueError, match="camera"):
            g.mask(cam)
        with pytest.raises(ValueError, match="camera"):
            g.reset(cam)
    assert g.mask(0).shape == (0, 0)                                # nothing was touched by the refused calls
    mv, ch = g.update([a, None])
    assert mv.tolist() == [True, False] and ch.tolist() == [4, -1]
    # reversed rows and pixel-strided views are read through a dense copy
    mv, ch = g.update([np.ascontiguousarray(a[::-1])[::-1], a[:, ::2]])
    assert mv.tolist() == [False, True] and ch.tolist() == [0, 2]


def test_c_abi_refuses_bad_arguments_before_any_work():
    import ctypes as C
    from cvsd_amd import _lib
    lib = _lib.lib()
    h = C.c_void_p()
    mk = lambda **kw: _lib.MotionOpts(**{**dict(struct_size=C.sizeof(_lib.MotionOpts), block=16, level=2.0, min_blocks=4, max_skip=30), **kw})
    for n, o in ((0, mk()), (65, mk()), (2, mk(block=4)), (2, mk(level=300.0)), (2, mk(min_blocks=-2)), (2, mk(struct_size=4))):
        assert lib.mi355_motion_gate_create(-1, n, C.byref(o), C.byref(h)) == -1 and not h.value
    assert lib.mi355_motion_gate_create(-1, 1, None, C.byref(h)) == 0          # NULL options: the defaults
    a = K.scene(20, 20, 16, 0)
    mv, ch = (C.c_int * 1)(), (C.c_int * 1)()
    for kw in (dict(height=-20), dict(width=0), dict(row_stride=59), dict(bytes_per_pixel=2), dict(data=None)):
        f = _lib.MotionFrame(**{**dict(data=a.ctypes.data, height=20, width=20, row_stride=60, bytes_per_pixel=3), **kw})
        assert lib.mi355_motion_gate_update(h, (C.POINTER(_lib.MotionFrame) * 1)(C.pointer(f)), 0, mv, ch) == -1
    f = _lib.MotionFrame(data=a.ctypes.data, height=20, width=20, row_stride=60, bytes_per_pixel=3)
    assert lib.mi355_motion_gate_update(h, (C.POINTER(_lib.MotionFrame) * 1)(C.pointer(f)), 1, mv, ch) == -1      # device frames, host gate
    assert lib.mi355_motion_gate_update(h, (C.POINTER(_lib.MotionFrame) * 1)(C.pointer(f)), 0, mv, ch) == 0
    assert (mv[0], ch[0]) == (1, 4)                                 # still the first frame: the refused calls left no state
    assert lib.mi355_motion_gate_reset(h, 1) == -1 and lib.mi355_motion_gate_reset(h, -1) == 0
    lib.mi355_motion_gate_destroy(h)
    with pytest.raises(ValueError, match="block"):
        ops.motion_grid([a], block=5, device=-1)


def test_track_cameras_refuses_bad_motion_gate_arguments_without_a_gpu():
    """the argument is parsed before anything runs (a model object is not needed for that)"""
    from cvsd_amd.engine import YOLO
    parse = YOLO._motion_gate_spec
    assert parse(None, 4) is None
    assert parse(True, 4) == dict(block=16, level=2.0, min_blocks=4, max_skip=30)
    assert parse({"block": 8, "max_skip": None}, 4) == dict(block=8, level=2.0, min_blocks=4, max_skip=None)
    with pytest.raises(ValueError, match=r"\['blok', 'device'\]"):
        parse({"blok": 8, "device": 0}, 4)
    with pytest.raises(ValueError, match="level"):
        parse({"level": -2}, 4)
    with pytest.raises(ValueError, match="4 cameras"):
        parse(MotionGate(3, device=None), 4)
    with pytest.raises(TypeError):
        parse("yes", 4)
    g = MotionGate(4, device=None)
    assert parse(g, 4) is g
