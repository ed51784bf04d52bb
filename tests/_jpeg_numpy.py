"""A sequential checker of the JPEG encoder, written from the text of DESIGN.md 3.20 (not from csrc/jpeg_codec.h): Python integers, one
sample at a time, and a string of '0' / '1' for the entropy-coded data.  Also a small baseline parser: the markers, tables and per-block
coefficients of a stream.  Slow on purpose; the case table keeps the frames small."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# Annex K.1 / K.2 in natural (row-major) order, as the standard prints them
K1 = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K2 = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
# Annex K.3: BITS and HUFFVAL
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VAL = list(range(12))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
_TAIL = [r << 4 | s for r in range(16) for s in range(1, 11)]
AC_VAL = (
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1,
     0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2A],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19,
     0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A])
# both AC lists end with every remaining run/size symbol in ascending order
AC_VAL = tuple(head + [v for v in _TAIL if v not in head] for head in AC_VAL)


def quant_table(base, quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((b * s + 50) // 100, 1), 255) for b in base]


def huff_codes(bits, vals):
    """symbol -> (code, length): codes of one length count up, and double when the length grows (Annex C)"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def ycc(b, g, r):
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16, (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16,
            (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16)


def _pass(v, last):
    """one 8-point pass of the DCT of DESIGN.md 3.20"""
    n = 15 if last else 11
    h = 1 << (n - 1)
    t0, t7, t1, t6 = v[0] + v[7], v[0] - v[7], v[1] + v[6], v[1] - v[6]
    t2, t5, t3, t4 = v[2] + v[5], v[2] - v[5], v[3] + v[4], v[3] - v[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [0] * 8
    if last:
        o[0], o[4] = (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2
    else:
        o[0], o[4] = (t10 + t11) * 4, (t10 - t11) * 4
    z1 = (t12 + t13) * 4433
    o[2] = (z1 + t13 * 6270 + h) >> n
    o[6] = (z1 - t12 * 15137 + h) >> n
    z5 = (t4 + t5 + t6 + t7) * 9633
    a1, a2 = -(t4 + t7) * 7373, -(t5 + t6) * 20995
    a3, a4 = z5 - (t4 + t6) * 16069, z5 - (t5 + t7) * 3196
    o[7] = (t4 * 2446 + a1 + a3 + h) >> n
    o[5] = (t5 * 16819 + a2 + a4 + h) >> n
    o[3] = (t6 * 25172 + a2 + a3 + h) >> n
    o[1] = (t7 * 12299 + a1 + a4 + h) >> n
    return o


def fdct(block):
    """64 level-shifted samples, row-major -> 8 x the DCT coefficients, row-major"""
    b = list(block)
    for r in range(8):
        b[r * 8:r * 8 + 8] = _pass(b[r * 8:r * 8 + 8], False)
    for c in range(8):
        b[c::8] = _pass(b[c::8], True)
    return b


def quantise(c, q):
    r = (abs(c) + 4 * q) // (8 * q)
    return -r if c < 0 else r


def coefficients(img, quality=85, subsampling="420"):
    """-> int16 [blocks, 64]: quantised, zigzag order, blocks in scan order"""
    img = np.asarray(img)
    H, W = img.shape[:2]
    planes = [[[0] * W for _ in range(H)] for _ in range(3)]
    for y in range(H):
        for x in range(W):
            for c, v in enumerate(ycc(int(img[y, x, 0]), int(img[y, x, 1]), int(img[y, x, 2]))):
                planes[c][y][x] = v
    px = lambda c, x, y: planes[c][min(y, H - 1)][min(x, W - 1)]      # noqa: E731  the padded frame
    q = (quant_table(K1, quality), quant_table(K2, quality))
    sub = subsampling == "420"
    m = 16 if sub else 8
    out = []
    for my in range(-(-H // m)):
        for mx in range(-(-W // m)):
            blocks = []
            if sub:
                for j in range(4):
                    ox, oy = mx * 16 + (j & 1) * 8, my * 16 + (j >> 1) * 8
                    blocks.append((0, [px(0, ox + x, oy + y) - 128 for y in range(8) for x in range(8)]))
                for c in (1, 2):
                    blocks.append((1, [((px(c, mx * 16 + 2 * x, my * 16 + 2 * y) + px(c, mx * 16 + 2 * x + 1, my * 16 + 2 * y) +
                                         px(c, mx * 16 + 2 * x, my * 16 + 2 * y + 1) + px(c, mx * 16 + 2 * x + 1, my * 16 + 2 * y + 1) + 2) >> 2) - 128
                                       for y in range(8) for x in range(8)]))
            else:
                for c in range(3):
                    blocks.append((1 if c else 0, [px(c, mx * 8 + x, my * 8 + y) - 128 for y in range(8) for x in range(8)]))
            for tc, samples in blocks:
                d = fdct(samples)
                out.append([quantise(d[ZIGZAG[k]], q[tc][ZIGZAG[k]]) for k in range(64)])
    return np.array(out, np.int16).reshape(-1, 64)


def _bits(v, n):
    """the n magnitude bits of v: v itself, or v - 1 for a negative v, low n bits"""
    return format((v if v >= 0 else v - 1) & ((1 << n) - 1), "b").zfill(n) if n else ""


def _code(table, sym):
    c, length = table[sym]
    return format(c, "b").zfill(length)


def header(H, W, quality, subsampling):
    q = (quant_table(K1, quality), quant_table(K2, quality))
    mcus_x = -(-W // (16 if subsampling == "420" else 8))
    w16 = lambda v: bytes([v >> 8, v & 255])                      # noqa: E731
    o = b"\xff\xd8" + b"\xff\xe0" + w16(16) + b"JFIF\0" + b"\x01\x01" + b"\0" + w16(1) + w16(1) + b"\0\0"
    for i in range(2):
        o += b"\xff\xdb" + w16(67) + bytes([i]) + bytes(q[i][ZIGZAG[k]] for k in range(64))
    o += b"\xff\xc0" + w16(17) + b"\x08" + w16(H) + w16(W) + b"\x03" + bytes([1, 0x22 if subsampling == "420" else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for i in range(2):
        o += b"\xff\xc4" + w16(19 + 12) + bytes([i]) + bytes(DC_BITS[i]) + bytes(DC_VAL)
        o += b"\xff\xc4" + w16(19 + 162) + bytes([0x10 | i]) + bytes(AC_BITS[i]) + bytes(AC_VAL[i])
    o += b"\xff\xdd" + w16(4) + w16(mcus_x)
    o += b"\xff\xda" + w16(12) + bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return o


def encode(img, quality=85, subsampling="420"):
    img = np.asarray(img)
    H, W = img.shape[:2]
    coef = coefficients(img, quality, subsampling).tolist()
    dc = (huff_codes(DC_BITS[0], DC_VAL), huff_codes(DC_BITS[1], DC_VAL))
    ac = (huff_codes(AC_BITS[0], AC_VAL[0]), huff_codes(AC_BITS[1], AC_VAL[1]))
    m, comps = (16, [0, 0, 0, 0, 1, 2]) if subsampling == "420" else (8, [0, 1, 2])
    mcus_x, mcus_y = -(-W // m), -(-H // m)
    out = bytearray(header(H, W, quality, subsampling))
    it = iter(coef)
    for row in range(mcus_y):
        if row:
            out += bytes([0xFF, 0xD0 + (row - 1) % 8])
        pred, s = [0, 0, 0], ""
        for _ in range(mcus_x):
            for c in comps:
                zz, tc = next(it), 1 if c else 0
                d = zz[0] - pred[c]
                pred[c] = zz[0]
                n = abs(d).bit_length()
                s += _code(dc[tc], n) + _bits(d, n)
                run = 0
                for k in range(1, 64):
                    v = zz[k]
                    if v == 0:
                        run += 1
                        continue
                    while run >= 16:
                        s += _code(ac[tc], 0xF0)
                        run -= 16
                    n = abs(v).bit_length()
                    s += _code(ac[tc], run << 4 | n) + _bits(v, n)
                    run = 0
                if run:
                    s += _code(ac[tc], 0x00)
        s += "1" * (-len(s) % 8)
        for i in range(0, len(s), 8):
            b = int(s[i:i + 8], 2)
            out.append(b)
            if b == 0xFF:
                out.append(0)
    return bytes(out + b"\xff\xd9")


# ---- parser ---------------------------------------------------------------------------------------------------------------------------
def parse(data):
    """A baseline stream -> {"markers": [(marker, payload length)], "dqt": {id: 64 steps in zigzag order}, "dht": {(class, id): (bits, vals)},
    "sof": {...}, "dri": interval, "scan": bytes, "coefficients": int [blocks, 64] (zigzag order, DC absolute), "rst": the RSTm seen}"""
    assert data[:2] == b"\xff\xd8", "no SOI"
    info = {"markers": [(0xD8, 0)], "dqt": {}, "dht": {}, "dri": 0, "rst": []}
    i = 2
    while True:
        assert data[i] == 0xFF, f"no marker at {i}"
        mk, length = data[i + 1], data[i + 2] << 8 | data[i + 3]
        seg = data[i + 4:i + 2 + length]
        info["markers"].append((mk, length))
        if mk == 0xDB:
            assert len(seg) == 65 and seg[0] >> 4 == 0
            info["dqt"][seg[0] & 15] = list(seg[1:])
        elif mk == 0xC4:
            bits = list(seg[1:17])
            assert len(seg) == 17 + sum(bits)
            info["dht"][(seg[0] >> 4, seg[0] & 15)] = (bits, list(seg[17:]))
        elif mk == 0xC0:
            info["sof"] = {"precision": seg[0], "height": seg[1] << 8 | seg[2], "width": seg[3] << 8 | seg[4],
                           "components": [(seg[6 + 3 * k], seg[7 + 3 * k], seg[8 + 3 * k]) for k in range(seg[5])]}
        elif mk == 0xDD:
            info["dri"] = seg[0] << 8 | seg[1]
        elif mk == 0xE0:
            info["app0"] = bytes(seg)
        elif mk == 0xDA:
            info["sos"] = bytes(seg)
            i += 2 + length
            break
        i += 2 + length
    assert data[-2:] == b"\xff\xd9", "no EOI"
    info["scan"] = data[i:-2]
    info["markers"].append((0xD9, 0))
    # split at RSTm, unstuff, decode
    sof = info["sof"]
    sub = sof["components"][0][1] == 0x22
    m, comps = (16, [0, 0, 0, 0, 1, 2]) if sub else (8, [0, 1, 2])
    mcus_x, mcus_y = -(-sof["width"] // m), -(-sof["height"] // m)
    dec = {}
    for key, (bits, vals) in info["dht"].items():
        dec[key] = {(length, code): sym for sym, (code, length) in huff_codes(bits, vals).items()}
    segs, cur, k, scan = [], bytearray(), 0, info["scan"]
    while k < len(scan):
        if scan[k] == 0xFF:
            assert k + 1 < len(scan), "a lone 0xFF ends the scan"
            if scan[k + 1] == 0:
                cur.append(0xFF)
            else:
                assert 0xD0 <= scan[k + 1] <= 0xD7, f"marker {scan[k + 1]:02x} inside the scan"
                info["rst"].append(scan[k + 1] - 0xD0)
                segs.append(bytes(cur))
                cur = bytearray()
            k += 2
        else:
            cur.append(scan[k])
            k += 1
    segs.append(bytes(cur))
    info["segments"] = segs
    interval = info["dri"] or mcus_x * mcus_y
    coef, mcu = [], 0
    for seg in segs:
        s = "".join(format(b, "08b") for b in seg)
        pos, pred = 0, [0, 0, 0]

        def sym(table):
            nonlocal pos
            code, length = 0, 0
            while True:
                assert pos < len(s), "the segment ends inside a code"
                code, length, pos = code << 1 | (s[pos] == "1"), length + 1, pos + 1
                if (length, code) in table:
                    return table[(length, code)]
                assert length < 16, "no such code"

        def val(n):
            nonlocal pos
            if n == 0:
                return 0
            v = int(s[pos:pos + n], 2)
            pos += n
            return v if v >> (n - 1) else v - (1 << n) + 1

        for _ in range(min(interval, mcus_x * mcus_y - mcu)):
            for c in comps:
                tc = 1 if c else 0
                zz = [0] * 64
                pred[c] += val(sym(dec[(0, tc)]))
                zz[0] = pred[c]
                kk = 1
                while kk < 64:
                    rs = sym(dec[(1, tc)])
                    if rs == 0:
                        break
                    if rs == 0xF0:
                        kk += 16
                        continue
                    kk += rs >> 4
                    assert kk < 64, "a run leaves the block"
                    zz[kk] = val(rs & 15)
                    kk += 1
                coef.append(zz)
            mcu += 1
        assert len(s) - pos < 8 and set(s[pos:]) <= {"1"}, "a segment must end with fewer than 8 one-bits of padding"
    assert mcu == mcus_x * mcus_y
    info["coefficients"] = np.array(coef, np.int64).reshape(-1, 64)
    return info
