"""4:2:0 YUV frames as video decoders emit them (NV12, I420), handed to the engine by plane pointers.

The engine converts them to BGR on the GPU at ingest (csrc/yuv_kernels.hip): ``model(YUVFrame(...))`` returns what ``model(bgr)`` returns for
the BGR frame ``cv2.cvtColor(..., COLOR_YUV2BGR_NV12 / _I420)`` makes of the same planes.  Nothing here computes on the CPU.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib

FORMATS = {"nv12": _lib.PIX_NV12, "i420": _lib.PIX_I420}


def _is_cuda(p) -> bool:
    return isinstance(p, torch.Tensor) and p.is_cuda


class YUVFrame:
    """One NV12 or I420 frame.  ``y`` is the luma plane [H, W]; NV12 takes ``uv``, the interleaved chroma plane [H/2, W] (U,V,U,V...);
    I420 takes ``u`` and ``v``, [H/2, W/2] each.  Planes are uint8 numpy arrays, or CUDA tensors on the engine's GPU (a decoder's
    surfaces): 2-D, last stride 1, any row stride -- decoders pad rows and do not keep planes adjacent, so each plane is its own
    argument and nothing is copied here.  ``shape`` is (H, W); both must be even (the engine refuses the frame otherwise)."""

    def __init__(self, y, uv=None, u=None, v=None, fmt: str = "nv12"):
        fmt = str(fmt).lower()
        if fmt not in FORMATS:
            raise ValueError(f"fmt must be 'nv12' or 'i420', not {fmt!r}")
        self.fmt = fmt
        if y is None:
            raise ValueError("y: the luma plane is missing")
        if fmt == "nv12":
            if uv is None:
                raise ValueError("uv: an NV12 frame needs its interleaved chroma plane (uv=...)")
            if u is not None or v is not None:
                raise ValueError("u, v: an NV12 frame has one interleaved chroma plane (uv=...), not separate u and v")
            planes = {"y": y, "uv": uv}
        else:
            if u is None:
                raise ValueError("u: an I420 frame needs its U plane (u=...)")
            if v is None:
                raise ValueError("v: an I420 frame needs its V plane (v=...)")
            if uv is not None:
                raise ValueError("uv: an I420 frame has separate u and v planes, not an interleaved one")
            planes = {"y": y, "u": u, "v": v}
        self.on_device = _is_cuda(y)
        for name, p in list(planes.items()):
            if _is_cuda(p) != self.on_device:
                raise ValueError(f"{name}: the planes of a frame must be all host arrays or all CUDA tensors")
            if self.on_device:
                if p.dtype != torch.uint8 or p.ndim != 2 or (p.numel() and p.shape[1] > 1 and p.stride(1) != 1):
                    raise ValueError(f"{name}: planes must be 2-D uint8 with last stride 1")
            else:
                if isinstance(p, torch.Tensor):
                    p = p.numpy()
                p = np.asarray(p)
                if p.dtype != np.uint8 or p.ndim != 2 or (p.size and p.shape[1] > 1 and p.strides[1] != 1) or (p.size and p.strides[0] < 0):
                    raise ValueError(f"{name}: planes must be 2-D uint8 with last stride 1")
                planes[name] = p
        self.y = planes["y"]
        self.uv, self.u, self.v = planes.get("uv"), planes.get("u"), planes.get("v")
        h, w = int(self.y.shape[0]), int(self.y.shape[1])
        self.shape = (h, w)
        if h % 2 == 0 and w % 2 == 0:                         # odd sizes are the engine's to refuse
            want = (h // 2, w) if fmt == "nv12" else (h // 2, w // 2)
            for name in ("uv", "u", "v"):
                p = planes.get(name)
                if p is not None and tuple(p.shape) != want:
                    raise ValueError(f"{name}: a {fmt} frame of {h}x{w} has chroma planes of shape {want}, not {tuple(p.shape)}")

    @classmethod
    def from_packed(cls, arr, fmt: str = "nv12") -> "YUVFrame":
        """The usual single array [H*3/2, W]: the Y rows, then the chroma rows (NV12: H/2 rows of interleaved UV; I420: the U plane then the
        V plane, each H/2 x W/2 stored as H/4 rows of W bytes -- which needs H % 4 == 0; otherwise pass the planes)."""
        fmt = str(fmt).lower()
        if fmt not in FORMATS:
            raise ValueError(f"fmt must be 'nv12' or 'i420', not {fmt!r}")
        if arr.ndim != 2 or arr.shape[0] % 3:
            raise ValueError("arr: a packed 4:2:0 frame is a 2-D array of H*3/2 rows")
        h, w = int(arr.shape[0]) * 2 // 3, int(arr.shape[1])
        if fmt == "nv12":
            return cls(arr[:h], uv=arr[h:], fmt=fmt)
        if h % 4:
            raise ValueError(f"arr: a packed I420 frame needs H % 4 == 0 (H = {h}); pass the planes to YUVFrame(y, u=, v=, fmt='i420')")
        contiguous = arr.is_contiguous() if isinstance(arr, torch.Tensor) else arr.flags.c_contiguous
        if not contiguous or w % 2:
            raise ValueError("arr: a packed I420 frame must be contiguous with an even width")
        q = h // 4
        return cls(arr[:h], u=arr[h:h + q].reshape(h // 2, w // 2), v=arr[h + q:].reshape(h // 2, w // 2), fmt=fmt)

    def _planes(self):
        return [self.y, self.uv] if self.fmt == "nv12" else [self.y, self.u, self.v]

    def host(self) -> "YUVFrame":
        """The same frame with its planes in host memory (itself when they already are)."""
        if not self.on_device:
            return self
        p = [t.cpu().numpy() for t in self._planes()]
        return YUVFrame(p[0], uv=p[1], fmt="nv12") if self.fmt == "nv12" else YUVFrame(p[0], u=p[1], v=p[2], fmt="i420")

    def struct(self) -> _lib.YuvFrame:
        """mi355_yuv_frame of this frame; the planes must stay alive while the engine reads it."""
        ptr = (lambda p: p.data_ptr()) if self.on_device else (lambda p: p.ctypes.data)
        stride = (lambda p: int(p.stride(0))) if self.on_device else (lambda p: int(p.strides[0]))
        c = self.uv if self.fmt == "nv12" else self.u
        return _lib.YuvFrame(y=ptr(self.y), u=ptr(c), v=None if self.fmt == "nv12" else ptr(self.v), height=self.shape[0], width=self.shape[1],
                             y_stride=stride(self.y) if self.shape[0] > 1 else self.shape[1],
                             uv_stride=stride(c) if c.shape[0] > 1 else int(c.shape[1]), format=FORMATS[self.fmt], reserved=0)

    def to_bgr(self, device: int = 0) -> np.ndarray:
        """The BGR frame [H, W, 3] the engine makes of this one (``device=-1``: the kernel's host twin, no GPU)."""
        from .ops import yuv_to_bgr
        return yuv_to_bgr([self], device=device)[0]


def struct_array(frames: Sequence[YUVFrame]):
    return (_lib.YuvFrame * len(frames))(*[f.struct() for f in frames])


def as_frames(source) -> Optional[List[YUVFrame]]:
    """``source`` as a list of YUVFrames, None when it holds none; a list mixing them with anything else is a ValueError."""
    if isinstance(source, YUVFrame):
        return [source]
    if isinstance(source, (list, tuple)) and any(isinstance(f, YUVFrame) for f in source):
        if not all(isinstance(f, YUVFrame) for f in source):
            raise ValueError("source: a list must be all YUVFrames or none (convert BGR arrays and YUV frames in separate calls)")
        return list(source)
    return None
