"""Evidence frames: what to draw for a ``Results`` -- boxes, ``#id conf`` labels, COCO-17 skeletons and pixelated
people -- as the int32 primitive records the rasteriser of csrc/render_kernels.hip takes (``ops.render``).  Pure numpy: nothing here
touches a GPU, and the kernel sees nothing but rectangles, segments, discs and glyphs in integer pixels.

Defaults follow Ultralytics' ``Annotator`` where its rule is known (line width, limb list, both-joints gate, tracker boxes, label text).
PARITY UNPINNED: the exact pixels are this project's own rules (include/mi355_yolo.h) -- cv2 is not available to pin a single one to
``cv2.rectangle`` / ``cv2.line`` / ``cv2.putText``, and no test claims so."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

WORDS = 8                                            # MI355_RENDER_WORDS
MOSAIC, RECT, FILL, LINE, DISC, GLYPH = 1, 2, 3, 4, 5, 6
MAX_PRIMS = 16384                                    # MI355_RENDER_MAX_PRIMS
GLYPH_W, GLYPH_H, GLYPH_ADVANCE = 5, 7, 6            # font cell; characters advance by 6 font pixels
FONT_CHARS = "0123456789#.:%- "

# COCO-17 limbs, 0-based joint pairs (Ultralytics' Annotator.skeleton is the same list, 1-based)
SKELETON = ((15, 13), (13, 11), (16, 14), (14, 12), (11, 12), (5, 11), (6, 12), (5, 6), (5, 7), (6, 8), (7, 9), (8, 10), (1, 2), (0, 1),
            (0, 2), (1, 3), (2, 4), (3, 5), (4, 6))
HEAD_JOINTS = (0, 1, 2, 3, 4)                        # nose, eyes, ears
# "head": the bounding box of the visible head joints becomes a square around its centre whose side is HEAD_GROW times the box's larger
# side (at least HEAD_MIN_FRACTION of the person box's width): eyes and ears span the face's width, not the skull's height
HEAD_GROW = 2.0
HEAD_MIN_FRACTION = 0.25
# a fixed palette, B | G << 8 | R << 16, indexed by id % len or class % len
PALETTE = tuple(b | g << 8 | r << 16 for r, g, b in (
    (230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
    (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200), (128, 0, 0), (170, 255, 195),
    (128, 128, 0), (255, 215, 180), (0, 0, 128), (128, 128, 128)))
WHITE = 0xFFFFFF
_COORD = 1 << 20


@dataclass(frozen=True)
class RenderSpec:
    """What ``primitives`` draws.  ``anonymize``: None, "box" (the whole person box is pixelated) or "head"; ``mosaic``: the block side,
    4, 8, 16 or 32; ``line_width`` / ``kpt_radius``: None = Ultralytics' rule ``max(round((h + w) / 2 * 0.003), 2)`` (Python's round) and
    the line width; ``kpt_conf``: a joint is drawn when its confidence reaches it, a limb when both its joints do; ``color_by``: "id"
    (the class where there are no ids) or "class"."""
    boxes: bool = True
    labels: bool = True
    skeleton: bool = True
    anonymize: Optional[str] = None
    mosaic: int = 16
    line_width: Optional[int] = None
    kpt_radius: Optional[int] = None
    kpt_conf: float = 0.5
    color_by: str = "id"

    def __post_init__(self):
        if self.anonymize not in (None, "box", "head"):
            raise ValueError(f"anonymize must be None, 'box' or 'head', got {self.anonymize!r}")
        if self.mosaic not in (4, 8, 16, 32):
            raise ValueError(f"mosaic must be 4, 8, 16 or 32, got {self.mosaic!r}")
        if self.color_by not in ("id", "class"):
            raise ValueError(f"color_by must be 'id' or 'class', got {self.color_by!r}")
        if self.line_width is not None and not 1 <= int(self.line_width) <= 255:
            raise ValueError("line_width must be in 1 .. 255")
        if self.kpt_radius is not None and not 0 <= int(self.kpt_radius) <= 255:
            raise ValueError("kpt_radius must be in 0 .. 255")


def as_spec(arg) -> Optional[RenderSpec]:
    """``render=`` of predict / track / track_cameras -> None (off) or a RenderSpec"""
    if arg is None or arg is False:
        return None
    if arg is True:
        return RenderSpec()
    if isinstance(arg, RenderSpec):
        return arg
    if isinstance(arg, dict):
        return RenderSpec(**arg)
    raise TypeError(f"render must be None, True, a RenderSpec or a dict of its fields, not {type(arg).__name__}")


def line_width(h: int, w: int) -> int:
    return max(round((h + w) / 2 * 0.003), 2)


def _px(v) -> int:
    """a float coordinate -> the int32 pixel the kernel sees: floor(v + 0.5), kept inside the range the rasteriser accepts"""
    v = float(v)
    if not np.isfinite(v):
        return 0
    return int(min(max(np.floor(v + 0.5), -_COORD), _COORD))


def _px_array(a) -> list:
    """``_px`` of every element of an array, as nested lists of Python ints"""
    a = np.asarray(a, np.float64)
    return np.clip(np.floor(np.where(np.isfinite(a), a, 0.0) + 0.5), -_COORD, _COORD).astype(np.int64).tolist()


def label_text(track_id, conf) -> str:
    """``#id conf`` for a tracked box, ``conf`` alone otherwise; two decimals"""
    c = f"{float(conf):.2f}"
    return f"#{int(track_id)} {c}" if track_id is not None else c


def head_box(kpts, box, kpt_conf: float):
    """(x0, y0, x1, y1) floats of the region ``anonymize="head"`` pixelates: from the head joints that reach ``kpt_conf`` when at least
    two do, else (and for a detect model: kpts None) the top quarter of the box"""
    x1, y1, x2, y2 = (float(v) for v in box[:4])
    if kpts is not None:
        k = np.asarray(kpts, np.float64)[list(HEAD_JOINTS)]
        vis = k[:, 2] >= kpt_conf if k.shape[1] == 3 else np.ones(len(k), bool)
        if int(vis.sum()) >= 2:
            p = k[vis, :2]
            lo, hi = p.min(axis=0), p.max(axis=0)
            side = max(HEAD_GROW * float(max(hi[0] - lo[0], hi[1] - lo[1])), HEAD_MIN_FRACTION * (x2 - x1))
            cx, cy = (lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2
            return cx - side / 2, cy - side / 2, cx + side / 2, cy + side / 2
    return x1, y1, x2, y1 + (y2 - y1) / 4


def primitives(result, spec: Optional[RenderSpec] = None) -> np.ndarray:
    """-> int32 [P, 8] records {type, a, b, c, d, size, colour, 0} for one ``Results``, in painter's order: per box its mosaic, outline,
    limbs, joints, then its label (background and glyphs).  Boxes are the tracker's when the result carries ids."""
    spec = spec or RenderSpec()
    h, w = (int(v) for v in result.orig_shape)
    rows = []
    boxes = result.boxes
    n = len(boxes) if boxes is not None else 0
    if n == 0:
        return np.zeros((0, WORDS), np.int32)
    data = np.asarray(boxes.data, np.float64) if not hasattr(boxes.data, "numpy") else boxes.data.numpy().astype(np.float64)
    ids = data[:, 4] if boxes.is_track else None
    conf, cls = data[:, -2], data[:, -1]
    kp = None
    if result.keypoints is not None and len(result.keypoints) == n:
        kd = result.keypoints.data
        kp = np.asarray(kd.numpy() if hasattr(kd, "numpy") else kd, np.float64)
    lw = int(spec.line_width) if spec.line_width is not None else line_width(h, w)
    rad = int(spec.kpt_radius) if spec.kpt_radius is not None else lw
    scale = max(lw - 1, 1)                                       # label glyphs: one font pixel = scale x scale frame pixels
    bpx = _px_array(data[:, :4])                                 # every coordinate is rounded once, as arrays
    kpx = _px_array(kp[..., :2]) if kp is not None else None
    for i in range(n):
        key = int(ids[i]) if (ids is not None and spec.color_by == "id") else int(cls[i])
        colour = PALETTE[key % len(PALETTE)]
        x1, y1, x2, y2 = bpx[i]
        if spec.anonymize == "box":
            rows.append((MOSAIC, x1, y1, x2, y2, spec.mosaic, 0))
        elif spec.anonymize == "head":
            hb = head_box(kp[i] if kp is not None else None, data[i, :4], spec.kpt_conf)
            rows.append((MOSAIC, _px(hb[0]), _px(hb[1]), _px(hb[2]), _px(hb[3]), spec.mosaic, 0))
        if spec.boxes:
            rows.append((RECT, x1, y1, x2, y2, lw, colour))
        if spec.skeleton and kp is not None and kp.shape[1] == 17:
            k, kx = kp[i], kpx[i]
            vis = (k[:, 2] >= spec.kpt_conf).tolist() if k.shape[1] == 3 else [True] * len(k)
            for a, b in SKELETON:
                if vis[a] and vis[b]:
                    rows.append((LINE, kx[a][0], kx[a][1], kx[b][0], kx[b][1], lw, colour))
            for j in range(17):
                if vis[j]:
                    rows.append((DISC, kx[j][0], kx[j][1], 0, 0, rad, WHITE))
        if spec.labels:
            text = label_text(ids[i] if ids is not None else None, conf[i])
            tw, th, pad = (GLYPH_ADVANCE * len(text) - 1) * scale, GLYPH_H * scale, scale
            top = y1 - th - 2 * pad                               # above the box when it fits, else inside its top edge
            if top < 0:
                top = y1
            rows.append((FILL, x1, top, x1 + tw + 2 * pad - 1, top + th + 2 * pad - 1, 0, colour))
            for c, ch in enumerate(text):
                if ch != " ":
                    rows.append((GLYPH, x1 + pad + c * GLYPH_ADVANCE * scale, top + pad, ord(ch), 0, scale, WHITE))
    if len(rows) > MAX_PRIMS:
        raise ValueError(f"{len(rows)} primitives for one frame: at most {MAX_PRIMS} (MI355_RENDER_MAX_PRIMS) are drawn; nothing is dropped silently")
    out = np.zeros((len(rows), WORDS), np.int32)
    if rows:
        out[:, :7] = np.asarray(rows, np.int64)                  # every record has seven fields; the eighth word stays 0
    return out
