"""``Results`` / ``Boxes`` / ``Keypoints`` containers with the Ultralytics surface the reference uses.

Mirrors ``ultralytics/engine/results.py`` as far as the hot path needs it:
``/root/reference/model.py:40`` reads ``results[0].boxes``; ``:45`` ``boxes.is_track``; ``:67`` iterates
``for box in boxes`` (1-row ``Boxes``); ``:60-64`` ``float(box.id)``, ``float(box.xywhn[0][k])``.
north_star adds ``.keypoints`` for pose models.  Backed by torch CPU tensors, like ``Results.cpu()``.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch


class _BaseTensor:
    def __init__(self, data, orig_shape: Tuple[int, int]):
        self.data = data
        self.orig_shape = orig_shape

    @property
    def shape(self):
        return self.data.shape

    def cpu(self):
        return self if isinstance(self.data, np.ndarray) else self.__class__(self.data.cpu(), self.orig_shape)

    def numpy(self):
        return self if isinstance(self.data, np.ndarray) else self.__class__(self.data.numpy(), self.orig_shape)

    def cuda(self):
        return self.__class__(torch.as_tensor(self.data).cuda(), self.orig_shape)

    def to(self, *args, **kwargs):
        return self.__class__(torch.as_tensor(self.data).to(*args, **kwargs), self.orig_shape)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        d = self.data
        if isinstance(d, torch.Tensor) and not d.is_cuda and isinstance(idx, (np.ndarray, list, torch.Tensor)):
            # row selection through a numpy view of the same memory: torch's CPU advanced-indexing kernel costs 10-60 MILLIseconds
            # for a [300, 17, 3] tensor once its OpenMP pool has many threads (measured: 54 ms at 8 threads against 10 us at 1),
            # which made `res[idx]` of the tracker callback the slowest step of a pose model's frame loop
            ix = idx.numpy() if isinstance(idx, torch.Tensor) else np.asarray(idx)
            return self.__class__(torch.from_numpy(np.ascontiguousarray(d.numpy()[ix])), self.orig_shape)
        return self.__class__(d[idx], self.orig_shape)


def _clone(x):
    return x.copy() if isinstance(x, np.ndarray) else x.clone()


def _empty_like(x):
    return np.empty_like(x) if isinstance(x, np.ndarray) else torch.empty_like(x)


def xyxy2xywh(x):
    """utils/ops.py:xyxy2xywh -> (cx, cy, w, h)"""
    y = _empty_like(x)
    y[..., 0] = (x[..., 0] + x[..., 2]) / 2
    y[..., 1] = (x[..., 1] + x[..., 3]) / 2
    y[..., 2] = x[..., 2] - x[..., 0]
    y[..., 3] = x[..., 3] - x[..., 1]
    return y


def clip_boxes(boxes, shape):
    """utils/ops.py:clip_boxes -- x1,x2 to [0, w], y1,y2 to [0, h] on the first four columns, in place; shape = (h, w)."""
    h, w = shape[:2]
    if isinstance(boxes, np.ndarray):
        boxes[..., [0, 2]] = boxes[..., [0, 2]].clip(0, w)
        boxes[..., [1, 3]] = boxes[..., [1, 3]].clip(0, h)
    else:
        boxes[..., 0].clamp_(0, w)
        boxes[..., 1].clamp_(0, h)
        boxes[..., 2].clamp_(0, w)
        boxes[..., 3].clamp_(0, h)
    return boxes


class Boxes(_BaseTensor):
    """data: [N, 6] = x1,y1,x2,y2,conf,cls   or   [N, 7] = x1,y1,x2,y2,track_id,conf,cls (tracking)."""

    def __init__(self, boxes, orig_shape):
        if boxes.ndim == 1:
            boxes = boxes[None, :]
        n = boxes.shape[-1]
        assert n in (6, 7), f"expected 6 or 7 values but got {n}"
        super().__init__(boxes, orig_shape)
        self.is_track = n == 7

    @property
    def xyxy(self):
        return self.data[:, :4]

    @property
    def conf(self):
        return self.data[:, -2]

    @property
    def cls(self):
        return self.data[:, -1]

    @property
    def id(self):
        return self.data[:, -3] if self.is_track else None

    @property
    def xywh(self):
        return xyxy2xywh(self.xyxy)

    @property
    def xyxyn(self):
        xyxy = _clone(self.xyxy)
        xyxy[..., [0, 2]] /= self.orig_shape[1]
        xyxy[..., [1, 3]] /= self.orig_shape[0]
        return xyxy

    @property
    def xywhn(self):
        xywh = xyxy2xywh(self.xyxy)
        xywh[..., [0, 2]] /= self.orig_shape[1]
        xywh[..., [1, 3]] /= self.orig_shape[0]
        return xywh


class Keypoints(_BaseTensor):
    """data: [N, K, 3] = x, y, conf (or [N, K, 2]).  Points with conf < 0.5 get x = y = 0 on construction."""

    def __init__(self, keypoints, orig_shape):
        if keypoints.ndim == 2:
            keypoints = keypoints[None, :]
        if keypoints.shape[2] == 3:
            if isinstance(keypoints, torch.Tensor) and not keypoints.is_cuda:
                k = keypoints.numpy()                         # same memory (see _BaseTensor.__getitem__ on torch's CPU indexing kernels)
                k[..., :2][k[..., 2] < 0.5] = 0
            else:
                mask = keypoints[..., 2] < 0.5
                keypoints[..., :2][mask] = 0
        super().__init__(keypoints, orig_shape)
        self.has_visible = self.data.shape[-1] == 3

    @property
    def xy(self):
        return self.data[..., :2]

    @property
    def xyn(self):
        xy = _clone(self.xy)
        xy[..., 0] /= self.orig_shape[1]
        xy[..., 1] /= self.orig_shape[0]
        return xy

    @property
    def conf(self):
        return self.data[..., 2] if self.has_visible else None


def _rows_of(seq, idx):
    """``Results.crops`` / ``crop_jpegs`` under the index a ``Results`` is subscripted with: a tensor is indexed as it is, a list by an
    integer (one row), a slice, a boolean mask or an index array"""
    if seq is None:
        return None
    if isinstance(seq, torch.Tensor):
        if isinstance(idx, (int, np.integer)):
            return seq[[int(idx)]]
        return seq[torch.as_tensor(idx, device=seq.device) if isinstance(idx, (np.ndarray, list, torch.Tensor)) else idx]
    ix = idx.numpy() if isinstance(idx, torch.Tensor) else idx
    if isinstance(ix, (int, np.integer)):
        return [seq[ix]]
    if isinstance(ix, slice):
        return seq[ix]
    ix = np.asarray(ix)
    return [seq[int(i)] for i in (np.nonzero(ix)[0] if ix.dtype == bool else ix)]


class Results:
    """One image's predictions (``list[Results]`` is what ``model(frame)`` / ``model.track(frame)`` return)."""

    def __init__(self, orig_img: Optional[np.ndarray], path: str, names: Dict[int, str], boxes=None, keypoints=None,
                 orig_shape: Optional[Tuple[int, int]] = None, speed: Optional[dict] = None, anchor_idx=None, feats=None,
                 tile_idx=None, tiles=None):
        self.orig_img = orig_img
        self.orig_shape = tuple(orig_shape) if orig_shape is not None else tuple(orig_img.shape[:2])
        self.boxes = Boxes(boxes, self.orig_shape) if boxes is not None else None
        self.keypoints = Keypoints(keypoints, self.orig_shape) if keypoints is not None else None
        self.masks = self.probs = self.obb = None
        self.speed = speed or {"preprocess": None, "inference": None, "postprocess": None}
        self.names = names
        self.path = path
        self.anchor_idx = anchor_idx      # engine extra: source anchor of every row (index-identity checks)
        # predict(feats=True): float32 [M, s], row i the appearance embedding of box i, read from the Detect head's input maps
        # (Ultralytics' Results.feats under with_reid / model: auto); None otherwise
        self.feats = feats
        # predict(tile=...): tiles = int32 [E, 4] rows x, y, w, h of the frame's entries (its tiles, row-major, then the frame itself when
        # full_frame is set); tile_idx = int32 [M], the entry every row came from (anchor_idx is then the anchor within that entry's
        # own canvas).  None for an untiled call.
        self.tile_idx = tile_idx
        self.tiles = tiles
        # track_cameras(motion_gate=...): {"moving", "changed", "skipped"} of this camera's tick; None for any other call
        self.motion = None
        # predict / track / track_cameras(render=...): uint8 [H, W, 3], the frame with this result drawn in, rendered on the GPU from the
        # call's device copy; None for any other call
        self.rendered = None
        self._render_device = 0
        # predict / track / track_cameras(encode=...): bytes, a baseline JFIF stream of the rendered picture (with render=) or of the
        # frame itself, encoded on the GPU; None for any other call
        self.jpeg = None
        # predict / track / track_cameras(crops=...): crop i is the picture of box i -- a list of uint8 arrays (or CUDA
        # tensors), or with a fixed size and out="cuda" one CUDA tensor [M, h, w, 3]; crop_jpegs (with encode=): a list of bytes, None
        # for the crop of an empty rectangle.  None for any other call
        self.crops = None
        self.crop_jpegs = None

    def plot(self, **spec) -> np.ndarray:
        """``results[0].plot()``: this result drawn into a COPY of its frame -> uint8 [H, W, 3] BGR, rendered on the GPU
        (``ops.render``).  Keywords are the fields of :class:`cvsd_amd.render.RenderSpec` (``boxes``, ``labels``, ``skeleton``,
        ``anonymize``, ``mosaic``, ``line_width``, ``kpt_radius``, ``kpt_conf``, ``color_by``).  ``orig_img`` is left unchanged."""
        from . import ops
        from .render import RenderSpec, primitives
        if self.orig_img is None:
            raise ValueError("this Results holds no image (its frames were on the GPU, or YUV planes): ask for the picture at call time, "
                             "predict / track / track_cameras(..., render=True), and read Results.rendered")
        return ops.render(np.asarray(self.orig_img), primitives(self, RenderSpec(**spec)), device=self._render_device)

    def save(self, filename) -> str:
        """Writes ``Results.jpeg`` -- the stream ``encode=`` of predict / track / track_cameras made on the GPU -- to ``filename``."""
        if self.jpeg is None:
            raise ValueError("this Results holds no JPEG stream: ask for one at call time, predict / track / track_cameras(..., encode='jpeg')")
        with open(filename, "wb") as fh:
            fh.write(self.jpeg)
        return str(filename)

    def save_crop(self, save_dir, file_name="im"):
        """``results[0].save_crop(dir)``: one JPEG per box, ``save_dir/<class name>/<file_name>.jpg``, ``<file_name>2.jpg``, ... (the
        layout of Ultralytics' ``save_one_box`` under ``increment_path``) -> the paths.  Writes ``crop_jpegs`` when the call made them
        (``crops=..., encode=...`` or ``save_crop=True``); otherwise cuts native crops out of ``orig_img`` and encodes them now, on the
        GPU the engine lives on.  The crop of an empty rectangle (a box outside the frame) has no file."""
        import os
        streams = self.crop_jpegs
        if streams is None:
            from . import ops
            from .crops import crop_rects
            if self.orig_img is None:
                raise ValueError("this Results holds no image (its frames were on the GPU, or YUV planes) and no crop streams: ask for them "
                                 "at call time, predict / track / track_cameras(..., save_crop=True)")
            streams = []
            if len(self):
                rects = crop_rects(self.boxes.xyxy.numpy() if isinstance(self.boxes.xyxy, torch.Tensor) else self.boxes.xyxy, self.orig_shape)
                cut = ops.crop_resize(np.asarray(self.orig_img), rects, device=self._render_device, out="cuda")
                live = [c for c in cut if c.numel()]
                enc = iter(ops.jpeg_encode(live, device=self._render_device) if live else [])
                streams = [next(enc) if c.numel() else None for c in cut]
        paths = []
        cls = self.boxes.cls.tolist() if len(self) else []
        for b, c in zip(streams, cls):
            if b is None:
                continue
            d = os.path.join(str(save_dir), str(self.names[int(c)]))
            os.makedirs(d, exist_ok=True)
            path, k = os.path.join(d, f"{file_name}.jpg"), 1
            while os.path.exists(path):
                k += 1
                path = os.path.join(d, f"{file_name}{k}.jpg")
            with open(path, "wb") as fh:
                fh.write(b)
            paths.append(path)
        return paths

    def __len__(self):
        return len(self.boxes) if self.boxes is not None else 0

    def __getitem__(self, idx):
        r = Results(self.orig_img, self.path, self.names, orig_shape=self.orig_shape, speed=self.speed)
        if self.boxes is not None:
            r.boxes = self.boxes[idx]
        if self.keypoints is not None:
            r.keypoints = self.keypoints[idx]
        if self.feats is not None:
            ix = idx.numpy() if isinstance(idx, torch.Tensor) else idx
            r.feats = self.feats[[ix]] if isinstance(ix, (int, np.integer)) else self.feats[ix]       # an integer keeps one row, as Boxes does
        if self.tile_idx is not None:
            ix = idx.numpy() if isinstance(idx, torch.Tensor) else idx
            r.tile_idx = self.tile_idx[[ix]] if isinstance(ix, (int, np.integer)) else self.tile_idx[ix]
        r.tiles = self.tiles
        r.motion = self.motion
        r.rendered, r._render_device, r.jpeg = self.rendered, self._render_device, self.jpeg
        r.crops, r.crop_jpegs = _rows_of(self.crops, idx), _rows_of(self.crop_jpegs, idx)      # aligned with the boxes, like feats
        return r

    def update(self, boxes=None):
        """engine/results.py:Results.update -- the tracker callback replaces the box tensor with track rows, clipped to
        the image like ``Boxes(ops.clip_boxes(boxes, self.orig_shape), self.orig_shape)`` (the rows are Kalman-state boxes
        and may overhang the frame; the reference's CSV reads ``xywhn`` of the clipped ones)."""
        if boxes is not None:
            self.boxes = Boxes(clip_boxes(boxes, self.orig_shape), self.orig_shape)

    def cpu(self):
        return self

    def numpy(self):
        r = Results(self.orig_img, self.path, self.names, orig_shape=self.orig_shape, speed=self.speed)
        r.boxes = self.boxes.numpy() if self.boxes is not None else None
        r.keypoints = self.keypoints.numpy() if self.keypoints is not None else None
        r.feats = self.feats
        r.tile_idx, r.tiles = self.tile_idx, self.tiles
        r.motion = self.motion
        r.rendered, r._render_device, r.jpeg = self.rendered, self._render_device, self.jpeg
        r.crops, r.crop_jpegs = self.crops, self.crop_jpegs
        return r
