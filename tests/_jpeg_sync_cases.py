"""The inputs ``entropy="sync"`` adds to the case table of tests/_jpeg_decode_cases.py: scans long enough for several
subsequences and sequences.  ``noise48x64`` at quality 100 and 4:4:4 is a scan of about 12.6 KB with stuffed bytes; ``flat64x96`` has
blocks of a few bits, so many blocks end inside one subsequence; ``noise96x128`` at quality 100 and 4:4:4 is about 50 KB: two sequences
at the product constants (128 bytes x 256).  Each is crossed with the four layouts, qualities 50 and 100 and three ways Pillow writes a
stream: standard tables, optimised tables, a restart marker every MCU row."""
import functools
import struct

import _jpeg_decode_cases as K
import _jpeg_numpy as E
from _jpeg_cases import _noise, _smooth_bright

QUALITIES = (50, 100)
ENCODERS = ("std", "opt", "rr1")
SETTINGS = ((8, 4), (8, 64), (16, 16), (128, 256))            # (sub_bytes, seq_subs) of the hook; the last is the product's


@functools.lru_cache(maxsize=None)
def _frames():
    return {"noise48x64": _noise(48, 64, 3), "smooth64x96": _smooth_bright(64, 96), "flat64x96": K._flat(64, 96), "noise96x128": _noise(96, 128, 7)}


def case_ids():
    """-> [(id, name, layout, quality, encoder)] of the new inputs"""
    return [(f"{name}-{lay}-q{q}-{enc}", name, lay, q, enc) for name in _frames() for lay in K.LAYOUTS for q in QUALITIES for enc in ENCODERS]


@functools.lru_cache(maxsize=None)
def stream(name, layout, quality, encoder) -> bytes:
    if name in _frames():
        return K.pillow_encode(_frames()[name], quality, layout, **K.ENCODERS[encoder])
    return K.stream(name, layout, quality, encoder)


def groups(new_only=False):
    """(name, layout) -> [(id, quality, encoder)]: the existing table and the new inputs, what one batched decode call takes"""
    g = {}
    for cid, name, lay, q, enc in ([] if new_only else K.case_ids()) + case_ids():
        g.setdefault((name, lay), []).append((cid, q, enc))
    return g


# ---- the hand-derived stream ---------------------------------------------------------------------------------------------------------------
# Annex K.3 luminance codes used below: DC category 3 = 100, AC run 0 / size 1 = 00, EOB = 1010.
#   DC difference +5 (category 3): 100 101          6 bits
#   AC +1 (run 0, size 1):         00 1             3 bits
#   EOB:                           1010             4 bits
# Block 0 holds DC, two ACs and EOB: 16 bits.  Blocks 1 .. 11 hold DC, one AC and EOB: 13 bits each, block b from bit 16 + 13 (b - 1).
# 16 + 11 * 13 = 159 bits: 20 bytes with one padding 1-bit, no byte is FF (no three 1-bits in a row), so nothing is stuffed.
KNOWN_BITS = "100101" "001" "001" "1010" + ("100101" "001" "1010") * 11
# With sub_bytes = 8 the subsequences start at bits 0, 64 and 128.  The symbol boundaries of block b >= 1 lie at s = 16 + 13 (b - 1),
# s + 6 (k = 1), s + 9 (k = 2) and s + 13 (the next block).  Block 4: 55, 61, 64 -- the first boundary at or behind bit 64 is 64 itself:
# byte 8, bit 0, inside block 4 with k = 2.  Block 9: 120, 126, 129 -- the first at or behind 128 is 129: byte 16, bit 1, block 9, k = 2.
KNOWN_STATES = [(0, 0, 0, 0, 0, 0), (0, 8, 0, 0, 2, 4), (0, 16, 1, 0, 2, 9)]     # (segment, byte, bit, j, k, B)
KNOWN_COEFFICIENTS = [[5 * (b + 1), 1, 1 if b == 0 else 0] + [0] * 61 for b in range(12)]


def known_stream() -> bytes:
    """gray 8 x 96 (twelve blocks), the Annex K.3 luminance tables, every quantisation step 16, the scan KNOWN_BITS"""
    bits = KNOWN_BITS + "1" * (-len(KNOWN_BITS) % 8)
    scan = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    assert len(KNOWN_BITS) == 159 and len(scan) == 20 and 0xFF not in scan
    seg = lambda m, body: bytes([0xFF, m]) + struct.pack(">H", len(body) + 2) + body
    return (b"\xff\xd8" + seg(0xDB, bytes([0]) + bytes([16] * 64)) + seg(0xC0, struct.pack(">BHHB", 8, 8, 96, 1) + bytes([1, 0x11, 0]))
            + seg(0xC4, bytes([0x00]) + bytes(E.DC_BITS[0]) + bytes(E.DC_VAL)) + seg(0xC4, bytes([0x10]) + bytes(E.AC_BITS[0]) + bytes(E.AC_VAL[0]))
            + seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + scan + b"\xff\xd9")
