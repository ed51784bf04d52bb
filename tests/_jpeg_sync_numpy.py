"""The checker of ``entropy="sync"`` (csrc/jpeg_sync.h): ONE sequential bit walk in Python integers over the scan of a
well-formed stream, built on ``_jpeg_decode_numpy.parse``.  It records every symbol boundary as (byte, bit, j, k, B) -- the position in
the STUFFED stream relative to the segment's begin (the data byte that holds the next unread bit and the bit 0 .. 7 in it; never a
stuffing 00, so behind the last bit of an FF data byte it is (byte + 2, 0); behind the segment's end positions keep counting), the block
j within the MCU, the zigzag index k of the next coefficient (0: a DC symbol comes next) and the block B in progress.  A subsequence's
true entry state is the first boundary at or behind its start.  Nothing is speculated here and nothing is shared with the C++ code.
A segment's last subsequence can start behind the segment's last boundary -- on the stuffing zero of a final FF, or on a last byte that
holds padding bits only: no symbol of the true path begins there, its lane enters with B at the segment's block count and does
nothing.  Such a row is (segment, -1, -1, -1, -1, count).

    boundaries(data) -> per segment a list of (byte, bit, j, k, B)
    entry_states(data, sub_bytes) -> int64 [nsub, 6]: (segment, byte, bit, j, k, B) per subsequence
"""
import numpy as np

import _jpeg_decode_numpy as N


def _walk_segment(P, tabs, seg, blk0, nblk, bpm, ny):
    n = len(seg)
    idx, i = [], 0                                        # where every data byte lies in the stuffed segment
    while i < n:
        idx.append(i)
        i += 2 if seg[i] == 0xFF and i + 1 < n and seg[i + 1] == 0 else 1
    b = N._Bits(seg)

    def where():
        byte, bit = divmod(b.pos, 8)
        return (idx[byte] if byte < len(idx) else n + byte - len(idx)), bit

    out = [where() + (0, 0, blk0)]
    for blk in range(blk0, blk0 + nblk):
        j = (blk - blk0) % bpm
        c = 0 if j < ny else j - ny + 1
        sym = N._symbol(b, tabs[(0, P["td"][c])])
        assert sym is not None, "the checker takes well-formed streams"
        b.receive(sym)
        k = 1
        out.append(where() + (j, k, blk))
        while k < 64:
            sym = N._symbol(b, tabs[(1, P["ta"][c])])
            assert sym is not None
            r, sz = sym >> 4, sym & 15
            if sz == 0:
                if r != 15:
                    break
                k += 16
                assert k <= 64
            else:
                k += r
                assert k <= 63
                b.receive(sz)
                k += 1
            if k < 64:
                out.append(where() + (j, k, blk))
        out.append(where() + ((j + 1) % bpm, 0, blk + 1))  # the block has ended: EOB, or the coefficient or ZRL that reaches 64
    return out


def boundaries(data):
    P = N.parse(data)
    hs, vs, nc = P["hs"], P["vs"], P["ncomp"]
    mcus = -(-P["W"] // (8 * hs)) * -(-P["H"] // (8 * vs))
    ny = 1 if nc == 1 else hs * vs
    bpm = 1 if nc == 1 else ny + 2
    per = P["ri"] or mcus
    tabs = {k: N._Table(*v) for k, v in P["huff"].items()}
    out = []
    for s, (b0, b1) in enumerate(P["segments"]):
        nm = min(per, mcus - s * per)
        out.append(_walk_segment(P, tabs, P["data"][b0:b1], s * per * bpm, nm * bpm, bpm, ny))
    return P, out


def entry_states(data, sub_bytes):
    P, segs = boundaries(data)
    rows = []
    for s, ((b0, b1), bd) in enumerate(zip(P["segments"], segs)):
        nsub = max(1, -(-(b1 - b0) // sub_bytes))
        at = 0
        for i in range(nsub):
            while at < len(bd) and bd[at][0] < i * sub_bytes:
                at += 1
            rows.append((s,) + bd[at] if at < len(bd) else (s, -1, -1, -1, -1, bd[-1][4]))
    return np.array(rows, np.int64).reshape(-1, 6)


def stuffing_starts(data, sub_bytes):
    """how many subsequences start on a stuffing zero"""
    P = N.parse(data)
    n = 0
    for b0, b1 in P["segments"]:
        seg = P["data"][b0:b1]
        n += sum(1 for i in range(sub_bytes, len(seg), sub_bytes) if seg[i] == 0 and seg[i - 1] == 0xFF)
    return n
