"""The case table of the JPEG encoder: small BGR frames that reach every rule -- edge extension on one or both sides,
one MCU and several, more than eight MCU rows (the RST index wraps), flat frames (DC only), noise (long codes, ZRL, many 0xFF bytes to
stuff), a smooth frame with a bright block (early EOB, runs of 16 and more), a block without a zero (no EOB), a pitched view.
Every input runs at both subsamplings and at qualities 1, 50, 85 and 100."""
import numpy as np

QUALITIES = (1, 50, 85, 100)
SUBSAMPLINGS = ("420", "444")


def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _gradient(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(2 * x + y) % 256, (x + 3 * y + 40) % 256, (255 - x - y) % 256], -1).astype(np.uint8)


def _smooth_bright(h, w):
    """a slow ramp with one bright 5 x 5 block: most blocks end after a few coefficients, the block's neighbours carry isolated high
    frequencies behind long runs of zeros"""
    y, x = np.mgrid[0:h, 0:w]
    f = np.stack([60 + x // 2 + y // 4, 90 + y // 2, 120 + x // 3], -1).astype(np.uint8)
    f[h // 2:h // 2 + 5, w // 2:w // 2 + 5] = (250, 252, 255)
    return f


def _pitched():
    base = _noise(15, 40, 7)
    base[:, :31] = np.maximum(_gradient(15, 31) // 2, base[:, :31] // 4)
    return base[:, :31]                      # rows 120 bytes apart, 93 of them pixels


def inputs():
    """-> [(name, frame, fidelity)]: fidelity = the case is smooth or structured, so its PSNR is compared with Pillow's"""
    return [
        ("1x1", _noise(1, 1, 1), False),
        ("1x40", _gradient(1, 40), True),
        ("40x1", _gradient(40, 1), True),
        ("8x8", _gradient(8, 8), True),
        ("16x16", _gradient(16, 16), True),
        ("17x17", _noise(17, 17, 2), False),
        ("33x70", _gradient(33, 70), True),
        ("pitched15x31", _pitched(), False),
        ("zeros16", np.zeros((16, 16, 3), np.uint8), True),
        ("ones16", np.full((16, 16, 3), 255, np.uint8), True),
        ("noise33x70", _noise(33, 70, 3), False),
        ("smooth_bright48x64", _smooth_bright(48, 64), True),
        ("rows72x8", _gradient(72, 8), True),              # nine MCU rows of 4:4:4
        ("rows144x8", _smooth_bright(144, 8), True),       # nine MCU rows of 4:2:0
        ("dense8x8", _noise(8, 8, 11), False),             # at quality 100 a block without a zero coefficient: no EOB
    ]


def cases():
    """-> [(id, frame, quality, subsampling, fidelity)]"""
    return [(f"{name}-{ss}-q{q}", frame, q, ss, fid) for name, frame, fid in inputs() for ss in SUBSAMPLINGS for q in QUALITIES]
