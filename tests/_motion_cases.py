"""Scripted 12-tick sequences for the motion gate, shared by the host-twin tests (test_motion_gate.py) and the GPU tests
(test_gpu_motion_gate.py): every tick's moving / changed / flag grid and the sums grid are compared with the numpy statement
(_motion_numpy.py), exactly."""
import numpy as np

import _motion_numpy as M

SHAPES = [(1, 1), (2, 80), (7, 5), (97, 131), (240, 320), (50, 64)]     # 50x64: 16-byte aligned rows and a partial last strip at every block
BLOCKS = [8, 16, 32]
LAYOUTS = ["dense", "pitched", "pitch4", "odd"]


def lay(frame: np.ndarray, layout: str) -> np.ndarray:
    """the same pixels as a dense array, as a view of rows pitched wider than the frame, or as a view that starts at an odd byte"""
    if layout == "dense":
        return np.ascontiguousarray(frame)
    h, w = frame.shape[:2]
    tail = frame.shape[2:]
    row = w * int(np.prod(tail, dtype=np.int64))
    pitch = {"pitched": row + 13, "pitch4": (row + 3) // 4 * 4 + 4, "odd": row + 6}[layout]     # pitch4: rows 4-byte but not all 16-byte aligned
    lead = 1 + 16 * 3 if layout == "odd" else 0                    # odd: one byte past a 16-byte boundary, whatever the allocation's own
    buf = np.full(lead + h * pitch + 32, 0xA5, np.uint8)
    start = lead + (-buf.ctypes.data) % 16
    v = np.lib.stride_tricks.as_strided(buf[start:], shape=(h, w) + tail, strides=(pitch, row // w) + ((1,) if tail else ()))
    v[...] = frame
    assert not v.flags.c_contiguous or h == 1
    if layout == "odd":
        assert v.ctypes.data % 2 == 1
    return v


def scene(h, w, block, seed):
    """a random BGR frame whose block (0, 0) is flat gray 100: gray (v, v, v) has luma exactly v, so its sum can be moved by any amount"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    f[:block, :block] = 100
    return f


def bump(frame, block, amount):
    """block (0, 0)'s luma sum raised by exactly `amount`"""
    f = frame.copy()
    bh, bw = min(block, f.shape[0]), min(block, f.shape[1])
    p = bh * bw
    add = np.full(p, amount // p, np.int64)
    add[:amount % p] += 1
    f[:bh, :bw] = (100 + add).reshape(bh, bw, 1).astype(np.uint8)
    return f


def scripted(h, w, block, layout, level=2.0, seed=0):
    """-> (gate keywords, 12 ticks of [camera 0, camera 1]).  Camera 0: first frame, a repeat, block (0, 0) moved by exactly the threshold
    (not flagged: the test is a strict >) and by one more (flagged), a size change and back, an absent tick, then repeats until max_skip
    forces a refresh.  Camera 1: a small clip whose frames repeat pairwise, absent now and then."""
    a = scene(h, w, block, seed)
    p = min(block, h) * min(block, w)
    d = M.level_q(level) * p // 16
    other = scene(h + 3, w + 2, block, seed + 1)
    cam0 = [a, a, bump(a, block, d), bump(a, block, d + 1), a, other, a, None, a, a, a, a]
    rng = np.random.default_rng(seed + 2)
    base = [rng.integers(0, 256, (33, 47, 3), dtype=np.uint8) for _ in range(6)]
    cam1 = [None if t in (2, 7, 8) else base[t // 2] for t in range(12)]
    ticks = [[None if f0 is None else lay(f0, layout), f1] for f0, f1 in zip(cam0, cam1)]
    return dict(block=block, level=level, min_blocks=1, max_skip=3), ticks


def run(make_gate, sums_of, kw, ticks, resets=None):
    """Steps a gate made by make_gate(n, **kw) and the numpy Gate through `ticks`; resets = {tick: camera or None} applied before that
    tick.  -> the list of (moving, changed) per tick, after asserting that everything agrees."""
    n = len(ticks[0])
    gate, want = make_gate(n, **kw), M.Gate(n, **kw)
    out = []
    for t, frames in enumerate(ticks):
        if resets and t in resets:
            gate.reset(resets[t])
            want.reset(resets[t])
        mv, ch = gate.update(frames)
        wmv, wch = want.update(frames)
        assert mv.dtype == bool and ch.dtype == np.int32
        np.testing.assert_array_equal(ch, wch, err_msg=f"changed, tick {t}")
        np.testing.assert_array_equal(mv, wmv, err_msg=f"moving, tick {t}")
        for i in range(n):
            np.testing.assert_array_equal(gate.mask(i), want.masks[i], err_msg=f"mask of camera {i}, tick {t}")
        present = [i for i, f in enumerate(frames) if f is not None]
        if present:
            got = sums_of([frames[i] for i in present], kw["block"])
            for g, i in zip(got, present):
                assert g.dtype == np.uint32
                np.testing.assert_array_equal(g.astype(np.int64), want.sums[i], err_msg=f"sums of camera {i}, tick {t}")
        out.append((mv, ch))
    return out


def check_scripted(out):
    """what the script of `scripted` must have produced for camera 0 (min_blocks 1, max_skip 3)"""
    mv = [bool(o[0][0]) for o in out]
    ch = [int(o[1][0]) for o in out]
    assert mv == [True, False, False, True, True, True, True, False, False, False, False, True], mv
    assert ch[1] == 0 and ch[2] == 0 and ch[3] == 1 and ch[4] == 1 and ch[7] == -1 and ch[8:] == [0, 0, 0, 0], ch
