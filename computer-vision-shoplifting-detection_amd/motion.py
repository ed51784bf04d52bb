"""Motion gate: which cameras of a tick changed since their last detector pass -- a thin binding of
csrc/motion_kernels.hip (``mi355_motion_gate_*``).

Per camera a grid of block-luma sums is compared with the grid of the last frame that ran the detector; a camera whose grid moved in
fewer than ``min_blocks`` blocks is static, and ``YOLO.track_cameras(..., motion_gate=...)`` steps its tracker on the rows the detector
last produced for it instead of running the detector again.  Integer arithmetic throughout (include/mi355_yolo.h states it):
``device=k`` runs one HIP launch per tick for all cameras, ``device=None`` the same routine on the host; both give the same numbers.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .yuv import YUVFrame

BLOCKS = (8, 16, 32)
OPTIONS = ("block", "level", "min_blocks", "max_skip")


def check_options(block=16, level=2.0, min_blocks=4, max_skip=30) -> dict:
    """The gate's options, validated (a ``ValueError`` names the offending one) -> the keywords of :class:`MotionGate`."""
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or int(block) not in BLOCKS:
        raise ValueError(f"block must be 8, 16 or 32, not {block!r}")
    try:
        lv = float(level)
    except (TypeError, ValueError):
        raise ValueError(f"level must be a number in [0, 255], not {level!r}") from None
    if not 0.0 <= lv <= 255.0:                                    # NaN fails both comparisons
        raise ValueError(f"level must be in [0, 255], not {level!r}")
    if isinstance(min_blocks, bool) or not isinstance(min_blocks, (int, np.integer)) or int(min_blocks) < 0:
        raise ValueError(f"min_blocks must be an integer >= 0, not {min_blocks!r}")
    if max_skip is not None and (isinstance(max_skip, bool) or not isinstance(max_skip, (int, np.integer)) or int(max_skip) < 0):
        raise ValueError(f"max_skip must be an integer >= 0 or None, not {max_skip!r}")
    return {"block": int(block), "level": lv, "min_blocks": int(min_blocks), "max_skip": None if max_skip is None else int(max_skip)}


def _descriptor(f, keep: list) -> Tuple[_lib.MotionFrame, bool]:
    """One frame -> (mi355_motion_frame, lives on a GPU).  Host BGR arrays and uint8 CUDA tensors [H, W, 3] of any row pitch (a view such
    as ``frame[:, 5:]`` is read in place), ``YUVFrame``s by their Y plane.  ``keep`` collects what must stay alive for the call."""
    if isinstance(f, YUVFrame):
        y, bpp = f.y, 1
    else:
        y, bpp = f, 3
    on_dev = isinstance(y, torch.Tensor) and y.is_cuda
    if isinstance(y, torch.Tensor) and not on_dev:
        y = y.numpy()
    if not on_dev:
        y = np.asarray(y)
    if y.dtype != (torch.uint8 if on_dev else np.uint8) or y.ndim != (2 if bpp == 1 else 3) or (bpp == 3 and y.shape[2] != 3):
        raise ValueError("frames must be uint8 BGR [H, W, 3] arrays or CUDA tensors, YUVFrames, or None for an absent camera")
    h, w = int(y.shape[0]), int(y.shape[1])
    if h <= 0 or w <= 0:
        raise ValueError(f"a frame of {h}x{w} has no pixels")
    st = [int(s) for s in (y.stride() if on_dev else y.strides)]
    dense_px = st[1] == bpp and (bpp == 1 or st[2] == 1)
    if not (dense_px and (st[0] >= w * bpp or h == 1)):
        y = y.contiguous() if on_dev else np.ascontiguousarray(y)      # pixels not packed, rows overlapping or reversed: a dense copy
        st = [w * bpp]
    keep.append(y)
    d = _lib.MotionFrame(data=y.data_ptr() if on_dev else y.ctypes.data, height=h, width=w, row_stride=st[0] if h > 1 else w * bpp,
                         bytes_per_pixel=bpp)
    return d, on_dev


class MotionGate:
    """``MotionGate(n_cameras).update(frames) -> (moving bool[n], changed int32[n])``.

    ``block`` (8, 16 or 32 pixels), ``level`` (mean luma change of a block that flags it, in [0, 255]), ``min_blocks`` (flagged blocks
    that make a camera move; 0: every present camera moves), ``max_skip`` (static present ticks after which a camera is forced to
    move; None: never).  A camera moves on its first frame, after :meth:`reset`, and when its size or format (BGR / YUV) changes.  A moving
    camera's grid becomes its reference; a static camera keeps its reference, so slow drift adds up until it trips.  An absent camera
    (``None``) reports ``moving=False, changed=-1`` and its state stays as it is.

    ``device=k``: one launch per tick on GPU k (csrc/motion_kernels.hip); ``device=None``: the same routine on the host."""

    def __init__(self, n_cameras: int, block: int = 16, level: float = 2.0, min_blocks: int = 4, max_skip: Optional[int] = 30,
                 device: Optional[int] = 0):
        if isinstance(n_cameras, bool) or not isinstance(n_cameras, (int, np.integer)) or not 1 <= int(n_cameras) <= _lib.MOTION_MAX_CAMERAS:
            raise ValueError(f"n_cameras must be in [1, {_lib.MOTION_MAX_CAMERAS}], not {n_cameras!r}")
        self.options = check_options(block, level, min_blocks, max_skip)
        self.n, self.device = int(n_cameras), (None if device is None else int(device))
        self.block = self.options["block"]
        o = self.options
        opts = _lib.MotionOpts(struct_size=C.sizeof(_lib.MotionOpts), block=o["block"], level=o["level"], min_blocks=o["min_blocks"],
                               max_skip=-1 if o["max_skip"] is None else o["max_skip"])
        self._h = None
        h = C.c_void_p()
        _lib.check(_lib.lib().mi355_motion_gate_create(-1 if self.device is None else self.device, self.n, C.byref(opts), C.byref(h)))
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            try:
                _lib.lib().mi355_motion_gate_destroy(h)
            except Exception:
                pass

    def update(self, frames: Sequence) -> Tuple[np.ndarray, np.ndarray]:
        """One tick: ``frames[i]`` is camera i's frame or None.  Host BGR arrays (any row pitch), uint8 CUDA tensors, ``YUVFrame``s (host
        or device planes: the Y plane is the luma).  A GPU gate takes the present frames all on the host or all on its GPU; a host gate
        brings CUDA frames to the host first."""
        frames = list(frames)
        if len(frames) != self.n:
            raise ValueError(f"MotionGate({self.n}) takes a list of {self.n} frames (None = camera absent), got {len(frames)}")
        keep: list = []
        descs: List[Optional[_lib.MotionFrame]] = []
        where = set()
        for f in frames:
            if f is None:
                descs.append(None)
                continue
            if self.device is None:
                if isinstance(f, YUVFrame):
                    f = f.host()
                elif isinstance(f, torch.Tensor) and f.is_cuda:
                    f = f.cpu()
            d, on_dev = _descriptor(f, keep)
            if on_dev and keep[-1].device.index != self.device:
                raise ValueError("frames live on a different GPU than the gate")
            where.add(on_dev)
            descs.append(d)
        if len(where) > 1:
            raise ValueError("the present frames of a tick must be all host memory or all CUDA memory")
        on_dev = bool(where and where.pop())
        if on_dev:
            torch.cuda.current_stream(keep[0].device).synchronize()      # the gate reads on a stream of its own
        return self._update(descs, on_dev)

    def _update(self, descs, on_device: bool) -> Tuple[np.ndarray, np.ndarray]:
        ptrs = (C.POINTER(_lib.MotionFrame) * self.n)(*[C.pointer(d) if d is not None else None for d in descs])
        moving, changed = np.zeros(self.n, np.int32), np.full(self.n, -1, np.int32)
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        _lib.check(_lib.lib().mi355_motion_gate_update(self._h, ptrs, int(on_device), i32(moving), i32(changed)))
        return moving.astype(bool), changed

    def _update_device_bgr(self, ptrs, shapes) -> Tuple[np.ndarray, np.ndarray]:
        """``update`` on dense BGR frames known by raw device pointer (None = absent): the uploaded copies of the tick's motion
        compensation, whose pointers come back behind an event wait for that upload (``MultiGMC.pending_device_frames``)."""
        descs = [None if p is None else _lib.MotionFrame(data=int(p), height=int(s[0]), width=int(s[1]), row_stride=3 * int(s[1]), bytes_per_pixel=3)
                 for p, s in zip(ptrs, shapes)]
        return self._update(descs, True)

    def mask(self, camera: int) -> np.ndarray:
        """uint8 [gh, gw]: the blocks of ``camera`` flagged on its last present tick ([0, 0] before its first frame)."""
        if not 0 <= int(camera) < self.n:
            raise ValueError(f"camera {camera} out of range")
        gh, gw = C.c_int(), C.c_int()
        _lib.check(_lib.lib().mi355_motion_gate_mask(self._h, int(camera), None, 0, C.byref(gh), C.byref(gw)))
        out = np.zeros((gh.value, gw.value), np.uint8)
        if out.size:
            _lib.check(_lib.lib().mi355_motion_gate_mask(self._h, int(camera), out.ctypes.data, out.size, C.byref(gh), C.byref(gw)))
        return out

    def reset(self, camera: Optional[int] = None) -> None:
        """Forget the reference of ``camera`` (None: of every camera): its next frame moves."""
        if camera is not None and not 0 <= int(camera) < self.n:
            raise ValueError(f"camera {camera} out of range")
        _lib.check(_lib.lib().mi355_motion_gate_reset(self._h, -1 if camera is None else int(camera)))
