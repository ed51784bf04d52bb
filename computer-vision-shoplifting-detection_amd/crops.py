"""Person crops: which rectangle of a frame a box becomes, and what ``crops=`` of predict / track / track_cameras asks
for.  Pure numpy: nothing here touches a GPU, and the kernel of csrc/crop_kernels.hip (``ops.crop_resize``) sees nothing but integer
rectangles.

⚠︎UL: the geometry restates Ultralytics' ``utils/plotting.py:save_one_box`` from memory (xyxy2xywh, optional square, ``wh * gain + pad``,
xywh2xyxy, ``.long()``, clip_boxes) -- unpinned like the rest of the Ultralytics rules here; the known answers of
tests/test_crop_rects.py pin THIS statement of it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np


@dataclass(frozen=True)
class CropSpec:
    """What ``crops=`` cuts.  ``size``: None (native: every crop has its rectangle's size) or (h, w); ``fit``: "stretch"
    (``cv2.resize(crop, (w, h), INTER_LINEAR)``) or "pad" (LetterBox(auto=False) with ``fill``); ``gain`` / ``pad`` / ``square``:
    ``save_one_box``'s; ``source``: "frame" or "rendered" (needs ``render=``: the crops are cut from the drawn picture); ``out``:
    "numpy", or "cuda" -- with a fixed size one uint8 tensor [M, h, w, 3] per frame that never leaves the GPU."""
    size: Optional[Tuple[int, int]] = None
    fit: str = "stretch"
    fill: int = 114
    gain: float = 1.02
    pad: int = 10
    square: bool = False
    source: str = "frame"
    out: str = "numpy"

    def __post_init__(self):
        if self.size is not None:
            if len(tuple(self.size)) != 2 or any(int(s) != s or int(s) < 1 for s in self.size):
                raise ValueError(f"size must be None or (h, w) of positive integers, got {self.size!r}")
            object.__setattr__(self, "size", (int(self.size[0]), int(self.size[1])))
        if self.fit not in ("stretch", "pad"):
            raise ValueError(f"fit must be 'stretch' or 'pad', got {self.fit!r}")
        if not 0 <= int(self.fill) <= 255:
            raise ValueError("fill must be in 0 .. 255")
        if self.source not in ("frame", "rendered"):
            raise ValueError(f"source must be 'frame' or 'rendered', got {self.source!r}")
        if self.out not in ("numpy", "cuda"):
            raise ValueError(f"out must be 'numpy' or 'cuda', got {self.out!r}")


def as_spec(arg) -> Optional[CropSpec]:
    """``crops=`` of predict / track / track_cameras -> None (off) or a CropSpec"""
    if arg is None or arg is False:
        return None
    if arg is True:
        return CropSpec()
    if isinstance(arg, CropSpec):
        return arg
    if isinstance(arg, dict):
        return CropSpec(**arg)
    raise TypeError(f"crops must be None, True, a CropSpec or a dict of its fields, not {type(arg).__name__}")


def crop_rects(xyxy, shape, gain: float = 1.02, pad: int = 10, square: bool = False) -> np.ndarray:
    """Boxes float32 [M, 4] (x1, y1, x2, y2) of a frame of ``shape`` (h, w) -> int32 [M, 4] rectangles (x1, y1, x2, y2): crop i is
    ``frame[y1:y2, x1:x2]``.  ``save_one_box``'s steps in float32: centre and size, with ``square`` both sides the larger one,
    ``size * gain + pad``, back to corners, truncation toward zero, then x clipped to [0, w] and y to [0, h].  A rectangle with
    x2 <= x1 or y2 <= y1 is empty (a box that lies outside the frame)."""
    b = np.asarray(xyxy, np.float32).reshape(-1, 4)
    h, w = int(shape[0]), int(shape[1])
    two = np.float32(2)
    cx, cy = (b[:, 0] + b[:, 2]) / two, (b[:, 1] + b[:, 3]) / two
    bw, bh = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    if square:
        bw = bh = np.maximum(bw, bh)
    bw = bw * np.float32(gain) + np.float32(pad)
    bh = bh * np.float32(gain) + np.float32(pad)
    out = np.stack([cx - bw / two, cy - bh / two, cx + bw / two, cy + bh / two], axis=1).astype(np.float32)
    out = np.trunc(np.nan_to_num(out, nan=0.0, posinf=1e9, neginf=-1e9)).astype(np.int64)
    out[:, 0::2] = np.clip(out[:, 0::2], 0, w)
    out[:, 1::2] = np.clip(out[:, 1::2], 0, h)
    return out.astype(np.int32)


def crop_call_args(crops, encode, save_crop, render):
    """``crops=``, ``encode=``, ``save_crop=`` and ``render=`` of an entry point -> (CropSpec or None, the ``encode`` argument to go on
    with): ``save_crop=True`` is ``crops=True, encode="jpeg"`` when neither is given; ``source="rendered"`` needs ``render=``"""
    if save_crop and crops is None and encode is None:
        crops, encode = True, "jpeg"
    spec = as_spec(crops)
    if spec is not None and spec.source == "rendered" and (render is None or render is False):
        raise ValueError("crops: source='rendered' cuts the drawn picture and needs render=")
    return spec, encode
