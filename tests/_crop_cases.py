"""The case table of person crops, shared by tests/test_crop_cases.py (the host twin against the checker) and
tests/test_gpu_crops.py (the kernel against the host twin), and ``raw_call``: ``mi355_crops`` on destinations of the test's own, every
crop in a pitched slot between guard bytes that must come back untouched."""
import ctypes as C

import numpy as np

from cvsd_amd import _lib

GUARD = 0xA5
SIZES = [(1, 1), (2, 3), (17, 9), (64, 32), (3, 2)]        # 3 w mod 4 = 3, 1, 3, 0, 2
FITS = ["stretch", "pad"]
FILLS = [0, 114]


def _frame(h: int, w: int, extra: int, seed: int) -> np.ndarray:
    """a random BGR frame [h, w, 3] whose rows are 3 w + extra bytes apart"""
    rng = np.random.default_rng(seed)
    store = rng.integers(0, 256, (h, 3 * w + extra), dtype=np.uint8)
    return store[:, :3 * w].reshape(h, w, 3)


_FRAMES = {}


def frames() -> dict:
    if not _FRAMES:
        _FRAMES.update({"37x53": _frame(37, 53, 7, 1), "16x16": _frame(16, 16, 4, 2), "1x9": _frame(1, 9, 0, 3), "9x1": _frame(9, 1, 5, 4)})
    return _FRAMES


# (x1, y1, x2, y2)
RECTS = {
    "37x53": [
        ("whole", (0, 0, 53, 37)), ("1x1", (5, 7, 6, 8)), ("1xN", (3, 10, 40, 11)), ("Nx1", (20, 2, 21, 30)),
        ("corner-tl", (0, 0, 8, 6)), ("corner-tr", (45, 0, 53, 6)), ("corner-bl", (0, 31, 8, 37)), ("corner-br", (45, 31, 53, 37)),
        ("right-bottom", (30, 20, 53, 37)), ("w4", (10, 5, 14, 12)), ("w5", (10, 5, 15, 12)), ("w6", (10, 5, 16, 12)), ("w7", (10, 5, 17, 12)),
        ("inner", (7, 5, 30, 20)), ("1x500-like", (2, 3, 51, 4)),
        ("empty-w", (10, 10, 10, 20)), ("empty-neg", (20, 20, 15, 25)), ("empty-corner", (53, 37, 53, 37)),
    ],
    "16x16": [("whole", (0, 0, 16, 16)), ("1x1-last", (15, 15, 16, 16)), ("half", (8, 0, 16, 16)), ("mid", (3, 4, 9, 15)), ("empty-h", (2, 7, 9, 7))],
    "1x9": [("whole", (0, 0, 9, 1)), ("1x1", (8, 0, 9, 1)), ("part", (2, 0, 7, 1))],
    "9x1": [("whole", (0, 0, 1, 9)), ("1x1", (0, 8, 1, 9)), ("part", (0, 2, 1, 7))],
}


def rects(name: str) -> np.ndarray:
    return np.array([r for _, r in RECTS[name]], np.int32).reshape(-1, 4)


def calls():
    """-> list of (id, frame names, [rects per frame], size, fit, fill): every frame with all its rectangles at every size, fit and fill;
    every non-empty rectangle at its own size (the copy path of a fixed size); and calls that mix frames with zero, one and many crops"""
    names = list(RECTS)
    out = [("native", names, [rects(n) for n in names], None, "stretch", 114)]
    for size in SIZES:
        for fit in FITS:
            for fill in FILLS:
                out.append((f"{size[0]}x{size[1]}-{fit}-{fill}", names, [rects(n) for n in names], size, fit, fill))
    for n in names:
        for rid, r in RECTS[n]:
            if r[2] > r[0] and r[3] > r[1]:
                for fit in FITS:
                    out.append((f"same-{n}-{rid}-{fit}", [n], [np.array([r], np.int32)], (r[3] - r[1], r[2] - r[0]), fit, 114))
    none = np.zeros((0, 4), np.int32)
    mixed = ["16x16", "37x53", "1x9", "37x53", "9x1"]
    mixed_r = [none, rects("37x53")[13:14], none, rects("37x53"), rects("9x1")]
    out.append(("mixed-native", mixed, mixed_r, None, "stretch", 114))
    out.append(("mixed-17x9-pad", mixed, mixed_r, (17, 9), "pad", 0))
    out.append(("mixed-64x32-stretch", mixed, mixed_r, (64, 32), "stretch", 114))
    out.append(("all-empty", ["16x16", "1x9"], [none, none], (17, 9), "stretch", 114))
    return out


def out_shape(rect, size):
    x1, y1, x2, y2 = (int(v) for v in rect)
    if size is not None:
        return int(size[0]), int(size[1])
    return (y2 - y1, x2 - x1) if x2 > x1 and y2 > y1 else (0, 0)


def raw_call(device, frame_list, rect_list, size, fit="stretch", fill=114, dst_extra=5, alloc=None, frame_desc=None, expect_rc=0,
             fit_code=None, spec_size=None):
    """``mi355_crops(device, ...)`` with destinations of the test's own: crop k lies at offset 3 (so mostly not dword-aligned) of a slot
    whose rows are 3 w + dst_extra bytes apart, slots separated by 64 guard bytes.  ``alloc(nbytes) -> (obj, address, to_numpy)`` places the
    buffer (default: host memory); ``frame_desc(frame) -> _lib.RenderFrame`` describes a frame (default: a host array by its strides).
    Returns the crops, after asserting that no byte outside them changed; with ``expect_rc != 0`` asserts the refusal and that NOTHING
    changed, and returns the message."""
    lib = _lib.lib()
    n = len(frame_list)
    rect_list = [np.ascontiguousarray(r, np.int32).reshape(-1, 4) for r in rect_list]
    slots, at = [], 64
    for r in rect_list:
        for k in range(len(r)):
            h, w = out_shape(r[k], size)
            pitch = 3 * w + dst_extra
            slots.append((at + 3, h, w, pitch))
            at += 3 + h * pitch + 64
    total = at
    on_device = alloc is not None
    if alloc is None:
        buf = np.full(total, GUARD, np.uint8)
        address, to_numpy = buf.ctypes.data, lambda: buf
    else:
        buf, address, to_numpy = alloc(total)
    if frame_desc is None:
        def frame_desc(f):
            return _lib.RenderFrame(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0], 0)
    fd = (_lib.RenderFrame * n)(*[frame_desc(f) for f in frame_list])
    ptrs = (C.c_void_p * n)(*[r.ctypes.data if len(r) else None for r in rect_list])
    counts = (C.c_int * n)(*[len(r) for r in rect_list])
    od = (_lib.RenderOut * max(len(slots), 1))(*[_lib.RenderOut(address + off, pitch, int(on_device)) for off, _, _, pitch in slots])
    spec = _lib.CropSpec(C.sizeof(_lib.CropSpec) if spec_size is None else spec_size, 0 if size is None else size[0],
                         0 if size is None else size[1], _lib.CROP_FIT[fit] if fit_code is None else fit_code, fill)
    rc = lib.mi355_crops(device, fd, n, ptrs, counts, C.byref(spec), od, None, None)
    got = to_numpy()
    if expect_rc:
        assert rc == expect_rc, (rc, lib.mi355_last_error())
        assert (got == GUARD).all(), "a refused call wrote to a destination"
        return lib.mi355_last_error().decode()
    assert rc == 0, lib.mi355_last_error()
    keep = np.ones(total, bool)
    crops = []
    for off, h, w, pitch in slots:
        rows = off + np.arange(h)[:, None] * pitch + np.arange(3 * w)[None, :]
        keep[rows.ravel()] = False
        crops.append(got[rows.ravel()].reshape(h, w, 3))
    assert (got[keep] == GUARD).all(), "a byte outside the crops' pixels was written"
    return crops


def flat(names):
    f = frames()
    return [f[n] for n in names]
