"""A sequential JPEG decoder written from DESIGN.md 3.21 in Python integers: its own parser for the four layouts (4:4:4, 4:2:2, 4:2:0,
gray), bit-by-bit Huffman decoding (Annex F.2.2: mincode / maxcode / valptr, no look-ahead table), jpeg_idct_islow, fancy upsampling and
the colour conversion.  Nothing is shared with csrc/jpeg_decode.h.  Python integers do not overflow, so a block with extreme coefficients
is decoded exactly here; the host twin and the kernels must agree with it.

    decode(data) -> {"bgr": uint8 [H, W, 3], "coefficients": int16 [blocks, 64], "status": 0 | 1..4, ...}
"""
import numpy as np

OK, CODE_NOT_FOUND, RUN_PAST_BLOCK, SEGMENT_SHORT, SEGMENT_LONG = 0, 1, 2, 3, 4

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
          56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class Refused(ValueError):
    pass


def parse(data):
    """-> dict: H, W, ncomp, hs, vs, ri, q (per component, zigzag), huff {(class, id): (bits, vals)}, td / ta per component, segments
    [(begin, end)] of the entropy-coded bytes"""
    d = bytes(data)
    if d[:2] != b"\xff\xd8":
        raise Refused("no SOI")
    p, qt, huff, ri, sof = 2, {}, {}, 0, None
    while True:
        if p + 4 > len(d) or d[p] != 0xFF:
            raise Refused("no SOS")
        m = d[p + 1]
        if m == 0xFF:
            p += 1
            continue
        L = d[p + 2] << 8 | d[p + 3]
        s = d[p + 4:p + 2 + L]
        if m == 0xC0:
            if s[0] != 8:
                raise Refused("precision")
            H, W, nc = s[1] << 8 | s[2], s[3] << 8 | s[4], s[5]
            if nc not in (1, 3):
                raise Refused("components")
            sof = (H, W, [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(nc)])
        elif 0xC1 <= m <= 0xCF and m != 0xC4:
            raise Refused("SOF%d" % (m - 0xC0))
        elif m == 0xDB:
            i = 0
            while i < len(s):
                if s[i] >> 4:
                    raise Refused("16-bit DQT")
                qt[s[i] & 15] = list(s[i + 1:i + 65])
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(s):
                bits = list(s[i + 1:i + 17])
                n = sum(bits)
                huff[(s[i] >> 4, s[i] & 15)] = (bits, list(s[i + 17:i + 17 + n]))
                i += 17 + n
        elif m == 0xDD:
            ri = s[0] << 8 | s[1]
        elif m == 0xDA:
            if sof is None or s[0] != len(sof[2]):
                raise Refused("several scans")
            td = [s[2 + 2 * c] >> 4 for c in range(s[0])]
            ta = [s[2 + 2 * c] & 15 for c in range(s[0])]
            p += 2 + L
            break
        p += 2 + L
    H, W, comps = sof
    nc = len(comps)
    hs, vs = (1, 1) if nc == 1 else (comps[0][1], comps[0][2])
    if nc == 3 and ((hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any(c[1:3] != (1, 1) for c in comps[1:])):
        raise Refused("sampling")
    segs, begin, at, rst = [], p, p, 0
    while True:
        at = d.find(b"\xff", at)
        if at < 0 or at + 1 >= len(d):
            raise Refused("no EOI")
        m = d[at + 1]
        if m == 0:
            at += 2
        elif 0xD0 <= m <= 0xD7:
            if m != 0xD0 + rst % 8:
                raise Refused("RST out of sequence")
            segs.append((begin, at))
            rst, at = rst + 1, at + 2
            begin = at
        elif m == 0xD9:
            segs.append((begin, at))
            break
        else:
            raise Refused("marker in scan")
    return dict(H=H, W=W, ncomp=nc, hs=hs, vs=vs, ri=ri, q=[qt[c[3]] for c in comps], huff=huff, td=td, ta=ta, segments=segs, data=d)


class _Table:
    """Annex F.2.2.3: MINCODE, MAXCODE and VALPTR per code length"""

    def __init__(self, bits, vals):
        self.vals, self.mincode, self.maxcode, self.valptr = vals, [0] * 17, [-1] * 17, [0] * 17
        code = k = 0
        for l in range(1, 17):
            if bits[l - 1]:
                self.valptr[l], self.mincode[l] = k, code
                code += bits[l - 1]
                k += bits[l - 1]
                self.maxcode[l] = code - 1
            code <<= 1


class _Bits:
    """the unstuffed bits of one segment, one at a time; behind its end zero bits, which are counted"""

    def __init__(self, seg):
        out, i = [], 0
        while i < len(seg):
            out.append(seg[i])
            i += 2 if seg[i] == 0xFF and i + 1 < len(seg) and seg[i + 1] == 0 else 1
        self.bytes, self.pos, self.past = out, 0, 0

    def bit(self):
        byte, k = divmod(self.pos, 8)
        self.pos += 1
        if byte >= len(self.bytes):
            self.past += 1
            return 0
        return (self.bytes[byte] >> (7 - k)) & 1

    def receive(self, n):
        v = 0
        for _ in range(n):
            v = v << 1 | self.bit()
        return v


def _symbol(b, t):
    code = 0
    for l in range(1, 17):
        code = code << 1 | b.bit()
        if code <= t.maxcode[l]:
            return t.vals[t.valptr[l] + code - t.mincode[l]]
    return None


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def coefficients(P):
    """-> (int16 [blocks, 64], status)"""
    hs, vs, nc = P["hs"], P["vs"], P["ncomp"]
    mx, my = -(-P["W"] // (8 * hs)), -(-P["H"] // (8 * vs))
    ny = 1 if nc == 1 else hs * vs
    bpm = 1 if nc == 1 else ny + 2
    mcus = mx * my
    per = P["ri"] or mcus
    coef = np.zeros((mcus * bpm, 64), np.int16)
    tabs = {k: _Table(*v) for k, v in P["huff"].items()}
    if len(P["segments"]) != -(-mcus // per):
        raise Refused("segment count")
    for s, (b0, b1) in enumerate(P["segments"]):
        b = _Bits(P["data"][b0:b1])
        pred = [0, 0, 0]
        for m in range(s * per, min((s + 1) * per, mcus)):
            for j in range(bpm):
                c = 0 if j < ny else j - ny + 1
                sym = _symbol(b, tabs[(0, P["td"][c])])
                if sym is None:
                    return coef, CODE_NOT_FOUND
                pred[c] += _extend(b.receive(sym), sym)
                coef[m * bpm + j, 0] = ((pred[c] + 32768) % 65536) - 32768
                k = 1
                while k < 64:
                    sym = _symbol(b, tabs[(1, P["ta"][c])])
                    if sym is None:
                        return coef, CODE_NOT_FOUND
                    r, sz = sym >> 4, sym & 15
                    if sz == 0:
                        if r != 15:
                            break
                        k += 16
                        if k > 64:
                            return coef, RUN_PAST_BLOCK
                        continue
                    k += r
                    if k > 63:
                        return coef, RUN_PAST_BLOCK
                    coef[m * bpm + j, k] = _extend(b.receive(sz), sz)
                    k += 1
        if b.past:
            return coef, SEGMENT_SHORT
        if len(b.bytes) * 8 - b.pos >= 8:
            return coef, SEGMENT_LONG
    return coef, OK


def idct_1d(v, n):
    """one 8-point pass of jpeg_idct_islow on Python integers; n = 11 (columns) or 18 (rows)"""
    z1 = (v[2] + v[6]) * 4433
    t2, t3 = z1 - v[6] * 15137, z1 + v[2] * 6270
    t0, t1 = (v[0] + v[4]) << 13, (v[0] - v[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    h = 1 << (n - 1)
    return [(x + h) >> n for x in (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)]


def block_samples(zz, q):
    """64 coefficients (zigzag) and steps (zigzag) -> 8 x 8 samples as a list of rows"""
    blk = [0] * 64
    for k in range(64):
        blk[ZIGZAG[k]] = int(zz[k]) * int(q[k])
    for c in range(8):
        blk[c::8] = idct_1d(blk[c::8], 11)
    rows = []
    for r in range(8):
        rows.append([min(max(x + 128, 0), 255) for x in idct_1d(blk[8 * r:8 * r + 8], 18)])
    return rows


def _planes(P, coef):
    hs, vs, nc = P["hs"], P["vs"], P["ncomp"]
    mx, my = -(-P["W"] // (8 * hs)), -(-P["H"] // (8 * vs))
    ny = 1 if nc == 1 else hs * vs
    bpm = 1 if nc == 1 else ny + 2
    planes = [np.zeros((my * 8 * (vs if c == 0 else 1), mx * 8 * (hs if c == 0 else 1)), np.int64) for c in range(nc)]
    for m in range(mx * my):
        for j in range(bpm):
            if j < ny:
                c, x0, y0 = 0, ((m % mx) * hs + j % hs) * 8, ((m // mx) * vs + j // hs) * 8
            else:
                c, x0, y0 = j - ny + 1, (m % mx) * 8, (m // mx) * 8
            planes[c][y0:y0 + 8, x0:x0 + 8] = block_samples(coef[m * bpm + j], P["q"][c])
    return planes


def _upsample(p, P):
    """a chroma plane (padded) -> the H x W samples of the frame, as a list of rows"""
    H, W, hs, vs = P["H"], P["W"], P["hs"], P["vs"]
    if hs == 1:
        return [[int(p[y, x]) for x in range(W)] for y in range(H)]
    cw, ch = -(-W // 2), -(-H // vs)
    if cw <= 2:
        return [[int(p[y // vs, x // 2]) for x in range(W)] for y in range(H)]
    out = []
    for y in range(H):
        if vs == 1:
            r = [int(v) for v in p[y, :cw]]
            lo, hi, sh = 1, 2, 2
        else:
            near = y // 2
            far = min(near + 1, ch - 1) if y & 1 else max(near - 1, 0)
            r = [3 * int(a) + int(b) for a, b in zip(p[near, :cw], p[far, :cw])]
            lo, hi, sh = 8, 7, 4
        row = []
        for x in range(W):
            cx = x // 2
            if x & 1:
                row.append((3 * r[cx] + r[min(cx + 1, cw - 1)] + hi) >> sh)
            else:
                row.append((3 * r[cx] + r[max(cx - 1, 0)] + lo) >> sh)
        out.append(row)
    return out


def pixels(P, coef):
    planes = _planes(P, coef)
    H, W = P["H"], P["W"]
    out = np.zeros((H, W, 3), np.uint8)
    if P["ncomp"] == 1:
        out[:] = planes[0][:H, :W, None]
        return out
    cb, cr = _upsample(planes[1], P), _upsample(planes[2], P)
    clamp = lambda v: min(max(v, 0), 255)
    for y in range(H):
        for x in range(W):
            yy, b, r = int(planes[0][y, x]), cb[y][x] - 128, cr[y][x] - 128
            out[y, x] = (clamp(yy + ((116130 * b + 32768) >> 16)), clamp(yy + ((-22554 * b - 46802 * r + 32768) >> 16)),
                         clamp(yy + ((91881 * r + 32768) >> 16)))
    return out


def decode(data):
    P = parse(data)
    coef, status = coefficients(P)
    return {"bgr": pixels(P, coef) if status == OK else None, "coefficients": coef, "status": status, "ri": P["ri"],
            "segments": len(P["segments"]), "shape": (P["H"], P["W"])}
