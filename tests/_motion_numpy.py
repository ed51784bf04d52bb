"""The motion gate as a plain numpy statement (include/mi355_yolo.h "motion gate"): pad, reshape, sum, then the state
rules.  Independent of the library: the tests check the kernel and its host twin against this."""
import numpy as np


def luma(frame) -> np.ndarray:
    """int64 [H, W]: BGR2GRAY's 14-bit fixed point for a BGR array [H, W, 3]; the Y plane for anything that has one (a YUVFrame)"""
    y = getattr(frame, "y", None)
    if y is not None:
        return np.asarray(y.cpu() if hasattr(y, "cpu") else y).astype(np.int64)
    f = np.asarray(frame.cpu() if hasattr(frame, "cpu") else frame).astype(np.int64)
    return (1868 * f[..., 0] + 9617 * f[..., 1] + 4899 * f[..., 2] + 8192) >> 14


def fmt_of(frame) -> int:
    return 1 if getattr(frame, "y", None) is not None else 3


def block_sums(plane: np.ndarray, block: int) -> np.ndarray:
    h, w = plane.shape
    gh, gw = -(-h // block), -(-w // block)
    p = np.zeros((gh * block, gw * block), np.int64)
    p[:h, :w] = plane
    return p.reshape(gh, block, gw, block).sum(axis=(1, 3))


def block_pixels(h: int, w: int, block: int) -> np.ndarray:
    return block_sums(np.ones((h, w), np.int64), block)


def level_q(level: float) -> int:
    return int(np.floor(16.0 * float(level) + 0.5))


class Gate:
    def __init__(self, n, block=16, level=2.0, min_blocks=4, max_skip=30):
        self.n, self.block, self.lq, self.min_blocks, self.max_skip = n, block, level_q(level), min_blocks, max_skip
        self.ref = [None] * n          # (key, sums) of the last moving frame
        self.key = [None] * n          # (h, w, format) of the previous present frame
        self.run = [0] * n
        self.masks = [np.zeros((0, 0), np.uint8) for _ in range(n)]
        self.sums = [None] * n         # the last present frame's grid

    def reset(self, camera=None):
        for i in range(self.n):
            if camera is None or i == camera:
                self.ref[i], self.run[i] = None, 0

    def update(self, frames):
        moving, changed = np.zeros(self.n, bool), np.full(self.n, -1, np.int32)
        for i, f in enumerate(frames):
            if f is None:
                continue
            l = luma(f)
            key = (l.shape[0], l.shape[1], fmt_of(f))
            if key != self.key[i]:
                self.ref[i] = None
            self.key[i] = key
            s = block_sums(l, self.block)
            if self.ref[i] is None:
                flags = np.ones(s.shape, np.uint8)
            else:
                flags = (16 * np.abs(s - self.ref[i]) > self.lq * block_pixels(l.shape[0], l.shape[1], self.block)).astype(np.uint8)
            c = int(flags.sum())
            mv = self.ref[i] is None or c >= self.min_blocks or (self.max_skip is not None and self.run[i] >= self.max_skip)
            self.masks[i], self.sums[i], changed[i], moving[i] = flags, s, c, mv
            if mv:
                self.ref[i], self.run[i] = s, 0
            else:
                self.run[i] += 1
        return moving, changed
