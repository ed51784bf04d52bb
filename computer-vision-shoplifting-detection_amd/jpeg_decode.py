"""Baseline JPEG frames as cameras and archives deliver them (MJPEG, snapshots, ``0001.jpg`` dumps), handed to the engine as compressed
bytes.

The engine decodes them to BGR on the GPU at ingest (csrc/jpeg_decode_kernels.hip): ``model(JPEGFrame(data))`` returns what ``model(bgr)``
returns for the BGR frame Pillow (libjpeg-turbo) decodes from the same bytes.  Only the header is read here, once, at construction.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional

import numpy as np

from . import _lib

SUBSAMPLING = {444: "444", 422: "422", 420: "420", 400: "gray"}


class JPEGFrame:
    """One baseline JPEG stream: ``data`` is bytes-like (``JPEGFrame.open(path)`` reads a file).  A stream the decoder does not take
    (progressive, 12-bit, CMYK, other sampling factors, several scans, arithmetic coding, a missing table or EOI ...) raises
    ``ValueError`` with the reason here, not at the call that would decode it.  ``shape`` is (H, W), ``subsampling`` "444", "422", "420"
    or "gray", ``restart_interval`` the DRI value in MCUs (0: none), ``segments`` the number of restart segments of the scan (what the
    GPU's lanes decode side by side; 1 without restart markers) and ``blocks`` the number of 8 x 8 coefficient blocks.  ``entropy``:
    this frame's own request for where its Huffman decoding runs -- "auto", "gpu", "host" or "sync" (``ops.jpeg_decode``) -- which goes
    before the decoding call's; ``None``: the call decides.  It travels with the frame through predict, track and track_cameras."""

    def __init__(self, data, entropy=None):
        if isinstance(data, JPEGFrame):
            entropy = data.entropy if entropy is None else entropy
            data = data.data
        if entropy is not None and entropy not in _lib.JPEG_ENTROPY:
            raise ValueError(f"entropy must be None, 'auto', 'gpu', 'host' or 'sync', got {entropy!r}")
        self.entropy = entropy
        if isinstance(data, (str, os.PathLike)):
            raise TypeError("JPEGFrame takes the stream's bytes; JPEGFrame.open(path) reads a file")
        self.data = bytes(data)
        self._buf = np.frombuffer(self.data, np.uint8)
        info = _lib.JpegStreamInfo()
        _lib.check(_lib.lib().mi355_jpeg_info(self._buf.ctypes.data if len(self.data) else None, len(self.data), C.byref(info)))
        self.shape = (int(info.height), int(info.width))
        self.components = int(info.components)
        self.subsampling = SUBSAMPLING[int(info.subsampling)]
        self.restart_interval = int(info.restart_interval)
        self.segments = int(info.segments)
        self.blocks = int(info.blocks)

    @classmethod
    def open(cls, path, entropy=None) -> "JPEGFrame":
        with open(path, "rb") as f:
            return cls(f.read(), entropy=entropy)

    def __len__(self) -> int:
        return len(self.data)

    def struct(self) -> _lib.JpegStream:
        """mi355_jpeg_stream of this frame; the frame must stay alive while the engine reads it."""
        return _lib.JpegStream(self._buf.ctypes.data, len(self.data), 0, _lib.JPEG_ENTROPY[self.entropy] if self.entropy and self.entropy != "auto" else 0)

    def to_bgr(self, device: int = 0) -> np.ndarray:
        """The BGR frame [H, W, 3] the engine makes of this one (``device=-1``: the kernels' host twin, no GPU)."""
        from .ops import jpeg_decode
        return jpeg_decode(self, device=device)


def has_frames(source) -> bool:
    """whether ``source`` is a JPEGFrame or a list that holds one"""
    return isinstance(source, JPEGFrame) or (isinstance(source, (list, tuple)) and any(isinstance(f, JPEGFrame) for f in source))


def split_mjpeg(data) -> List[bytes]:
    """The streams of a raw concatenated MJPEG file: cut at SOI / EOI outside entropy-coded data (marker segments are stepped over by
    their lengths, so a thumbnail's SOI inside an APPn segment cuts nothing).  Nothing is decoded.  Bytes between streams are dropped;
    an unfinished last stream is dropped too."""
    buf = bytes(data)
    out, n, p = [], len(buf), 0
    while True:
        p = buf.find(b"\xff\xd8", p)
        if p < 0:
            return out
        q, end = p + 2, -1
        while q + 4 <= n and buf[q] == 0xFF:
            m = buf[q + 1]
            if m == 0xFF:
                q += 1
                continue
            if m == 0xD9:
                end = q + 2
                break
            seg = (buf[q + 2] << 8) | buf[q + 3]
            q += 2 + seg
            if m == 0xDA:                                   # entropy-coded data: to the next marker that is neither stuffing nor RSTm
                while True:
                    q = buf.find(b"\xff", q)
                    if q < 0 or q + 1 >= n:
                        q = n
                        break
                    if buf[q + 1] == 0 or 0xD0 <= buf[q + 1] <= 0xD7:
                        q += 2
                        continue
                    break
        if end < 0:
            if q + 2 <= n and buf[q:q + 2] == b"\xff\xd9":
                end = q + 2
            else:
                p += 2
                continue
        out.append(buf[p:end])
        p = end


def decode_sources(source, device: int, handle=None, to_host: bool = False):
    """``source`` of predict / track / track_cameras with every JPEGFrame replaced by its decoded BGR frame -- all of them in ONE decode
    call: uint8 CUDA tensors [H, W, 3] on ``device`` that never visit the host, or (``to_host``) numpy arrays.  Anything else in the
    list, ``None`` included, stays where it is."""
    from .ops import jpeg_decode
    if isinstance(source, JPEGFrame):
        return jpeg_decode([source], device=device, handle=handle, as_tensor=not to_host)
    idx = [i for i, f in enumerate(source) if isinstance(f, JPEGFrame)]
    dec = jpeg_decode([source[i] for i in idx], device=device, handle=handle, as_tensor=not to_host)
    out = list(source)
    for i, d in zip(idx, dec):
        out[i] = d
    return out
