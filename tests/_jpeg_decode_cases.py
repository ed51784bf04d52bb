"""The case table of the JPEG decoder: small streams that reach every rule -- one MCU and several, sides that are no
multiple of the MCU, chroma planes of 1, 2 (replication) and 3 columns (the smallest plane the triangle filter runs on), odd chroma
heights, nine restart segments (the RST index wraps), flat / gradient / noise / smooth-with-a-bright-block content, all four layouts,
qualities 1, 50, 85 and 100, five ways Pillow writes a stream (standard tables, optimised tables, a restart marker every block, every
second block, every MCU row) and the project's own encoder (a restart segment per MCU row)."""
import functools
import io

import numpy as np
from PIL import Image

from _jpeg_cases import _gradient, _noise, _smooth_bright

QUALITIES = (1, 50, 85, 100)
LAYOUTS = ("444", "422", "420", "gray")
ENCODERS = {"std": {}, "opt": {"optimize": True}, "rb1": {"restart_marker_blocks": 1}, "rb2": {"restart_marker_blocks": 2},
            "rr1": {"restart_marker_rows": 1}}
RESTART_ENCODERS = ("rb1", "rb2", "rr1")


def _flat(h, w):
    return np.full((h, w, 3), (40, 130, 220), np.uint8)


def inputs():
    """-> [(name, BGR frame)] (h x w)"""
    return [
        ("1x1", _noise(1, 1, 1)), ("1x40", _gradient(1, 40)), ("40x1", _gradient(40, 1)), ("8x8", _noise(8, 8, 11)), ("16x16", _gradient(16, 16)),
        ("17x17", _noise(17, 17, 2)),
        ("9x4", _gradient(9, 4)), ("3x6", _noise(3, 6, 5)), ("6x3", _smooth_bright(6, 3)),      # chroma planes of 2, 3 and 2 columns
        ("20x5", _noise(20, 5, 6)),                                                             # 3 chroma columns
        ("33x70", _smooth_bright(33, 70)), ("35x18", _noise(35, 18, 4)),
        ("flat16x24", _flat(16, 24)),
        ("rows144x8", _smooth_bright(144, 8)), ("rows72x8", _gradient(72, 8)),                  # nine MCU rows of 4:2:0 / of 4:4:4
    ]


def pillow_encode(bgr, quality, layout, **opts) -> bytes:
    buf = io.BytesIO()
    if layout == "gray":
        g = ((bgr[..., 0].astype(np.int32) + bgr[..., 1] + bgr[..., 2]) // 3).astype(np.uint8)
        Image.fromarray(g, "L").save(buf, "JPEG", quality=quality, **opts)
    else:
        Image.fromarray(np.ascontiguousarray(bgr[..., ::-1]), "RGB").save(buf, "JPEG", quality=quality,
                                                                         subsampling={"444": 0, "422": 1, "420": 2}[layout], **opts)
    return buf.getvalue()


def pillow_decode(data) -> np.ndarray:
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), np.uint8)[..., ::-1])


def has_dri(data) -> bool:
    """a DRI marker segment with a non-zero interval in front of SOS"""
    p = 2
    while p + 4 <= len(data) and data[p] == 0xFF:
        m, L = data[p + 1], data[p + 2] << 8 | data[p + 3]
        if m == 0xDD:
            return (data[p + 4] << 8 | data[p + 5]) > 0
        if m == 0xDA:
            return False
        p += 2 + L
    return False


def case_ids():
    """-> [(id, name, layout, quality, encoder)]; encoder "own" is the project's"""
    out = [(f"{name}-{lay}-q{q}-{enc}", name, lay, q, enc) for name, _ in inputs() for lay in LAYOUTS for q in QUALITIES for enc in ENCODERS]
    out += [(f"{name}-{lay}-q{q}-own", name, lay, q, "own") for name in ("17x17", "33x70", "rows144x8", "rows72x8", "1x1") for lay in ("444", "420")
            for q in (50, 100)]
    return out


@functools.lru_cache(maxsize=None)
def _frames():
    return dict(inputs())


@functools.lru_cache(maxsize=None)
def stream(name, layout, quality, encoder) -> bytes:
    bgr = _frames()[name]
    if encoder == "own":
        from cvsd_amd import ops
        return ops.jpeg_encode(np.ascontiguousarray(bgr), quality=quality, subsampling=layout, device=-1)
    return pillow_encode(bgr, quality, layout, **ENCODERS[encoder])


def groups():
    """the table by (name, layout) -> [(id, quality, encoder)]: what one batched decode call takes"""
    g = {}
    for cid, name, lay, q, enc in case_ids():
        g.setdefault((name, lay), []).append((cid, q, enc))
    return g
