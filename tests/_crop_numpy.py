"""The sequential checker of person crops: what crop k of a call must be, made of the numpy slice of the frame and the
oracle's own functions -- ``oracle.yolo_oracle.resize_linear_u8`` (cv2.resize INTER_LINEAR, integer restatement) and
``letterbox(..., auto=False)``.  The one thing restated here is what the oracle does not have: ``fit="pad"`` clamps the inner size to at
least one pixel (a 1 x 500 crop into 64 x 64 would round to a side of 0), and paints ``fill`` where the oracle paints 114."""
import numpy as np

from oracle import yolo_oracle as O


def is_empty(rect) -> bool:
    x1, y1, x2, y2 = (int(v) for v in rect)
    return x2 <= x1 or y2 <= y1


def pad_geometry(ch: int, cw: int, size):
    """inner (h, w) and its (top, left) of ``fit="pad"``: the oracle's letterbox_geometry with the inner sides clamped to >= 1"""
    h, w = size
    (uw, uh), top, _, left, _ = O.letterbox_geometry(ch, cw, (h, w), auto=False)
    if uw >= 1 and uh >= 1:
        return (uh, uw), (top, left)
    uw, uh = max(uw, 1), max(uh, 1)
    dw, dh = (w - uw) / 2, (h - uh) / 2                       # letterbox_geometry's own two lines, for the clamped size
    return (uh, uw), (int(round(dh - 0.1)), int(round(dw - 0.1)))


def crop(frame: np.ndarray, rect, size=None, fit: str = "stretch", fill: int = 114) -> np.ndarray:
    x1, y1, x2, y2 = (int(v) for v in rect)
    if size is None:
        return np.zeros((0, 0, 3), np.uint8) if is_empty(rect) else frame[y1:y2, x1:x2].copy()
    h, w = size
    if is_empty(rect):
        return np.full((h, w, 3), fill, np.uint8)
    cut = frame[y1:y2, x1:x2].copy()
    if fit == "stretch":
        return O.resize_linear_u8(cut, w, h)
    assert fit == "pad"
    (ih, iw), (top, left) = pad_geometry(cut.shape[0], cut.shape[1], size)
    (uw, uh), _, _, _, _ = O.letterbox_geometry(cut.shape[0], cut.shape[1], (h, w), auto=False)
    if uw >= 1 and uh >= 1:
        out = O.letterbox(cut, (h, w), auto=False)             # the oracle's picture; only its 114 becomes `fill`
        assert out.shape == (h, w, 3)
        inner = out[top:top + ih, left:left + iw].copy()
    else:
        inner = O.resize_linear_u8(cut, iw, ih)
    res = np.full((h, w, 3), fill, np.uint8)
    res[top:top + ih, left:left + iw] = inner
    return res
