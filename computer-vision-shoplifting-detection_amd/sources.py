"""Frames as the engine receives them: the BGR frame view, the batch kinds, the device wait, the source normaliser and the
detector arguments of a call.  Nothing here knows a model; ``engine.py`` and ``ops.py`` both build on it.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from .yuv import YUVFrame, as_frames, struct_array


# ---------------------------------------------------------------------------------------------- one BGR frame
class DeviceFrame:
    """A dense-or-pitched BGR uint8 frame on a GPU known by raw pointer (``ops.render``): the copy a motion-compensation step uploaded"""
    def __init__(self, ptr: int, h: int, w: int, pitch: Optional[int] = None):
        self.ptr, self.shape, self.pitch = int(ptr), (int(h), int(w), 3), int(pitch) if pitch else 3 * int(w)


class FrameView(NamedTuple):
    keep: object                # what must stay alive while the engine reads `ptr`: the frame itself, or the dense copy made of it
    ptr: int
    pitch: int                  # bytes from one row to the next
    hw: Tuple[int, int]
    on_device: bool


def bgr_view(f, empty_ok: bool = False, dense: bool = False) -> FrameView:
    """THE rule for one BGR frame: uint8 [H, W, 3] with strides (>= 3W, 3, 1) is read where it lies, by pointer and row pitch; anything
    else of that type and shape is read from a dense copy.  ``f``: a host array, a CPU or CUDA tensor, or a :class:`DeviceFrame`.
    ``empty_ok``: an array without elements has no meaningful strides and is passed on as it is (the render / JPEG entries refuse it
    by its size); without it such a frame takes the rule like any other and the engine refuses it.
    ``dense``: a pitched frame is copied too (the motion compensation of ``track_cameras`` takes C-contiguous frames)."""
    if isinstance(f, DeviceFrame):
        return FrameView(f, f.ptr, f.pitch, f.shape[:2], True)
    if isinstance(f, torch.Tensor) and f.is_cuda:
        if f.dtype != torch.uint8 or f.ndim != 3 or f.shape[-1] != 3:
            raise ValueError("tensor frames must be uint8 [H,W,3] BGR")
        if not f.is_contiguous() if dense else (f.stride(2) != 1 or f.stride(1) != 3 or f.stride(0) < 3 * f.shape[1]):
            f = f.contiguous()
        return FrameView(f, f.data_ptr(), f.stride(0), (int(f.shape[0]), int(f.shape[1])), True)
    f = f.numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
    if f.dtype != np.uint8 or f.ndim != 3 or f.shape[-1] != 3:
        raise ValueError("frames must be uint8 arrays of shape [H,W,3] (BGR, as cv2 delivers them)")
    if not (empty_ok and not f.size):
        if not f.flags.c_contiguous if dense else (f.strides[2] != 1 or f.strides[1] != 3 or f.strides[0] < 3 * f.shape[1]):
            f = np.ascontiguousarray(f)
    return FrameView(f, f.ctypes.data, f.strides[0], (int(f.shape[0]), int(f.shape[1])), False)


def one_or_many(frames):
    """-> (list of frames, whether ``frames`` was one frame): the entries that take "a frame or a list of them"; None stays None"""
    single = isinstance(frames, (np.ndarray, YUVFrame, torch.Tensor, DeviceFrame))
    return ([frames] if single else frames), single


def same_place(on_device) -> bool:
    """whether the frames of a list lie on a GPU; host and CUDA frames in one list are refused"""
    if any(on_device) and not all(on_device):
        raise ValueError("a list of frames must be all host arrays or all CUDA tensors")
    return bool(any(on_device))


# ---------------------------------------------------------------------------------------------- the batch kinds
# A dense batch is a plain np.ndarray or torch.Tensor [N, H, W, 3] and takes the rect letterbox.  The kinds below hand their frames
# over by pointer; they share n, shape, shapes, on_device and `raw`: True = raw device pointers that somebody else keeps alive and
# has ordered (nothing to check or wait for), False = Python objects kept alive here (`tensors()` are the CUDA ones among them).
class Ragged:
    """BGR frames of different (h, w) in one call (several cameras): host arrays or CUDA tensors on the engine's GPU, each passed to
    ``mi355_yolo_infer_multi`` by pointer with its own row stride.  The engine letterboxes them to the square ``imgsz x imgsz``
    canvas, as Ultralytics' ``BasePredictor.pre_transform`` does for a batch whose shapes differ."""
    raw = False

    def __init__(self, frames, on_device: bool):
        views = [bgr_view(f) for f in frames]
        same_place([v.on_device for v in views] + [bool(on_device)])         # ... and they lie where the caller says
        self.frames = [v.keep for v in views]                   # kept alive for the call: the engine reads them by pointer
        self._fill([v.ptr for v in views], [v.hw for v in views], [v.pitch for v in views], on_device)

    @classmethod
    def from_pointers(cls, ptrs, shapes) -> "Ragged":
        """Dense BGR uint8 frames of different (h, w) that already sit on the engine's GPU, known by raw pointer (YOLO.track_cameras:
        the copies the tick's motion compensation uploaded)."""
        self = cls.__new__(cls)
        self.raw, self.frames = True, ()
        self._fill(ptrs, shapes, [3 * int(w) for _, w in shapes], True)
        return self

    def _fill(self, ptrs, shapes, pitches, on_device):
        self.n, self.on_device = len(ptrs), bool(on_device)
        self.shape = (self.n,)
        self.shapes = [(int(h), int(w)) for h, w in shapes]
        self.heights = np.array([s[0] for s in self.shapes], np.int32)
        self.widths = np.array([s[1] for s in self.shapes], np.int32)
        self.row_strides = np.array(pitches, np.int32)
        self.ptrs = (C.c_void_p * self.n)(*[int(p) for p in ptrs])

    def args(self):
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        return self.ptrs, i32(self.heights), i32(self.widths), i32(self.row_strides), int(self.on_device), self.n

    def tensors(self):
        return self.frames if self.on_device else ()

    def render_frames(self) -> list:
        """the frames as ``ops.render`` takes them"""
        return [DeviceFrame(p, h, w) for p, (h, w) in zip(self.ptrs, self.shapes)] if self.raw else list(self.frames)


class DeviceFrames:
    """n dense BGR uint8 frames of one (h, w) that already sit on the engine's GPU, known by one raw pointer (YOLO.track: the copy the
    tracker's motion compensation uploaded).  A dense batch: ``shape`` is [n, h, w, 3] and the letterbox is the rect one."""
    raw, on_device = True, True

    def __init__(self, ptr: int, n: int, h: int, w: int):
        self.ptr, self.n, self.shape = int(ptr), int(n), (int(n), int(h), int(w), 3)
        self.shapes = [(int(h), int(w))] * int(n)

    def data_ptr(self) -> int:
        return self.ptr


class YuvBatch:
    """NV12 / I420 frames (:class:`YUVFrame`) of any sizes in one call, all on the host or all on the engine's GPU, passed to
    ``mi355_yolo_infer_yuv`` by plane pointers: the engine converts them to BGR on the GPU in front of the letterbox."""
    raw = False

    def __init__(self, frames):
        self.frames = list(frames)                              # kept alive for the call: the engine reads the planes by pointer
        on_dev = {f.on_device for f in self.frames}
        if len(on_dev) != 1:
            raise ValueError("a list of YUVFrames must be all host planes or all CUDA planes")
        self.on_device = on_dev.pop()
        self.n = len(self.frames)
        self.shape = (self.n,)
        self.shapes = [f.shape for f in self.frames]
        self.structs = struct_array(self.frames)

    def tensors(self):
        return [p for f in self.frames for p in f._planes()] if self.on_device else ()

    def render_frames(self) -> list:
        return list(self.frames)


def wait_for_torch(device) -> None:
    """Work torch has enqueued on its current stream of ``device`` must be complete before the engine reads its result: the engine
    runs on a stream of its own."""
    torch.cuda.current_stream(device).synchronize()


def ready(batch, device: int) -> None:
    """THE device rule, for every batch kind: torch CUDA memory must live on the engine's GPU ``device``, and the call waits for
    torch's current stream there.  Host memory and raw-pointer kinds have nothing to check or wait for."""
    if isinstance(batch, torch.Tensor):
        held = (batch,) if batch.is_cuda else ()
    elif isinstance(batch, np.ndarray) or batch.raw:
        return
    else:
        held = batch.tensors()
    if held:
        if any(t.device.index != device for t in held):
            raise ValueError("frames live on a different GPU than the engine")
        wait_for_torch(held[0].device)


# ---------------------------------------------------------------------------------------------- source -> batch
def as_batch(source, by_pointer: bool = False):
    """What ``predict`` takes -> (batch, originals or None).  Dense against by-pointer decides the letterbox (the rect canvas of the
    one shape against the square ``imgsz x imgsz`` canvas), so it decides the rows:
    ``by_pointer=False`` (a call without ``tile``): an array or 4-D tensor is a dense batch; a list of one shape is STACKED into one
    (``np.stack`` / ``torch.stack``: a copy); a list of several shapes is :class:`Ragged`.
    ``by_pointer=True`` (a tiled call): always :class:`Ragged`, never stacked -- the tiles are cut from the frames where they lie.
    YUVFrames are a :class:`YuvBatch` either way.
    Originals: a host array gives its frames as views, a host list the caller's own objects (``Results.orig_img is frame``), CUDA
    frames None."""
    yuv = as_frames(source)                                     # a list mixing YUVFrames with anything else: its ValueError
    if yuv is not None:
        return YuvBatch(yuv), None
    if isinstance(source, (torch.Tensor, np.ndarray)):
        tensor = isinstance(source, torch.Tensor)
        # kept asymmetry 1: a 3-D TENSOR is one frame to a tiled call and refused by an untiled one (a 3-D array is one frame to both)
        dims = (4,) if tensor and not by_pointer else (3, 4)
        if source.dtype != (torch.uint8 if tensor else np.uint8) or source.ndim not in dims or source.shape[-1] != 3:
            raise ValueError("tensor sources must be uint8 [N,H,W,3] BGR frames" if tensor else
                             "frames must be uint8 arrays of shape [H,W,3] (BGR, as cv2 delivers them)")
        if by_pointer:
            source = [source] if source.ndim == 3 else list(source)
        elif tensor:
            # kept asymmetry 2: an untiled CPU tensor stays a tensor without originals (it goes in as .numpy() at call time); a tiled
            # call takes its frames as the .numpy() views below, and those are its originals
            return source.contiguous(), None
        else:
            source = source[None] if source.ndim == 3 else source
            return np.ascontiguousarray(source), list(source)
    if not isinstance(source, (list, tuple)):
        raise TypeError(f"unsupported source type {type(source).__name__}: pass decoded BGR uint8 frames "
                        f"(frame decode stays on the host, as in the reference's cv2.VideoCapture loop)")
    if not source:
        raise ValueError("empty source")
    on_device = same_place([isinstance(f, torch.Tensor) and f.is_cuda for f in source])
    if by_pointer and not on_device:
        source = [f.numpy() if isinstance(f, torch.Tensor) else f for f in source]
    originals = None if on_device else list(source)
    if by_pointer or len({tuple(np.shape(f)) for f in source}) != 1:
        return Ragged(source, on_device), originals
    stacked = torch.stack(list(source)) if on_device else np.stack([np.asarray(f) for f in source])
    return as_batch(stacked)[0], originals


# ---------------------------------------------------------------------------------------------- the detector arguments of a call
IOU, MAX_DET, IMGSZ = 0.7, 300, 640                             # the defaults of predict / track / track_cameras / infer_async


class DetArgs(NamedTuple):
    """The detector arguments of one call, resolved; in the order the facade's internal calls take them."""
    conf: float
    iou: float
    classes: tuple              # (c_int array or None, count), as the C entries take the class filter
    max_det: int
    imgsz: int                  # one number: a (h, w) pair is folded to its larger side
    half: Optional[bool]        # None = what the model was constructed with
    feats: Optional[bool]


def class_filter(classes):
    """``classes=`` of a call (None, one class or a sequence of them) -> (c_int array or None, count); a resolved pair passes through"""
    if isinstance(classes, tuple) and len(classes) == 2 and (classes[0] is None or isinstance(classes[0], C.Array)):
        return classes
    if classes is None:
        return None, 0
    cl = [int(classes)] if np.isscalar(classes) else [int(c) for c in classes]
    return (C.c_int * len(cl))(*cl), len(cl)


def det_args(conf, iou=IOU, classes=None, max_det=MAX_DET, imgsz=IMGSZ, half=None, feats=None) -> DetArgs:
    """resolves what it is given once; ``det_args(*a) == a`` for a resolved ``a``"""
    return DetArgs(float(conf), float(iou), class_filter(classes), int(max_det),
                   int(max(imgsz)) if isinstance(imgsz, (list, tuple)) else int(imgsz), half, feats)


def det_args_from(conf, kwargs: dict) -> DetArgs:
    """the same from the keyword arguments of ``track`` / ``track_cameras`` (other keys are the caller's business)"""
    return det_args(conf, **{k: kwargs[k] for k in DetArgs._fields[1:] if k in kwargs})
