"""The JPEG decoder's rules on the CPU (csrc/jpeg_decode.h): the sequential checker tests/_jpeg_decode_numpy.py against
Pillow (libjpeg-turbo), byte for byte, on every case of tests/_jpeg_decode_cases.py; the host twin (``device=-1``) against the checker
for pixels and coefficients; a hand-derived known answer; a hand-built stream with extreme coefficients; the round trip through the
project's encoder; every refused form; corrupt entropy-coded data; and the shared routine under AddressSanitizer / UBSan in a
stand-alone program.  Integer arithmetic: nothing here has a tolerance."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import _jpeg_decode_cases as K
import _jpeg_decode_numpy as N
import _jpeg_numpy as E
from cvsd_amd import JPEGFrame, ops

GROUPS = K.groups()
GROUP_IDS = [f"{g[0]}-{g[1]}" for g in GROUPS]
_checked = {}


def checker(data):
    if data not in _checked:
        _checked[data] = N.decode(data)
    return _checked[data]


# ---- the table --------------------------------------------------------------------------------------------------------------------------
def test_the_table_is_what_it_says():
    ids = K.case_ids()
    assert len(ids) == len({i[0] for i in ids}) == 15 * 4 * 4 * 5 + 20
    seen = set()
    for _, name, lay, q, enc in ids:
        d = K.stream(name, lay, q, enc)
        f = JPEGFrame(d)
        assert f.subsampling == lay and f.shape == K._frames()[name].shape[:2]
        if enc in K.RESTART_ENCODERS or enc == "own":
            assert K.has_dri(d) and f.restart_interval > 0, (name, lay, enc)
        else:
            assert not K.has_dri(d) and f.restart_interval == 0 and f.segments == 1
        seen.add(f.segments)
    assert {1, 2, 9}.issubset(seen) and max(seen) > 9            # nine and more segments: the RST index wraps


@pytest.mark.parametrize("group", list(GROUPS), ids=GROUP_IDS)
def test_checker_equals_pillow(group):
    for cid, q, enc in GROUPS[group]:
        d = K.stream(group[0], group[1], q, enc)
        got = checker(d)
        assert got["status"] == N.OK, cid
        assert np.array_equal(got["bgr"], K.pillow_decode(d)), cid


@pytest.mark.parametrize("group", list(GROUPS), ids=GROUP_IDS)
def test_host_twin_equals_checker(group):
    streams = [K.stream(group[0], group[1], q, enc) for _, q, enc in GROUPS[group]]
    pix = ops.jpeg_decode(streams, device=-1)
    coef = ops.jpeg_decode_coefficients(streams, device=-1)
    for (cid, _, _), d, p, c in zip(GROUPS[group], streams, pix, coef):
        want = checker(d)
        assert p.dtype == np.uint8 and np.array_equal(p, want["bgr"]), cid
        assert c.dtype == np.int16 and c.shape == want["coefficients"].shape and np.array_equal(c, want["coefficients"]), cid
        if group[1] in ("420", "444"):
            assert np.array_equal(c, E.parse(d)["coefficients"]), cid
        f = JPEGFrame(d)
        assert (f.segments, f.restart_interval, f.blocks) == (want["segments"], want["ri"], len(c))


def test_mixed_list_pitched_out_and_frame_methods(tmp_path):
    picks = [("33x70", "420", 85, "std"), ("17x17", "444", 100, "opt"), ("20x5", "422", 50, "rb2"), ("35x18", "gray", 1, "rr1"),
             ("rows72x8", "444", 50, "own"), ("1x1", "420", 85, "rb1")]
    streams = [K.stream(*p) for p in picks]
    single = [ops.jpeg_decode(d, device=-1) for d in streams]
    for s, g in zip(single, ops.jpeg_decode([JPEGFrame(d) for d in streams], device=-1, entropy="host")):
        assert np.array_equal(s, g)
    bufs = [np.full((s.shape[0] + 2, s.shape[1] + 3, 3), 0x5A, np.uint8) for s in single]
    views = [b[1:-1, 2:-1] for b in bufs]
    assert ops.jpeg_decode(streams, device=-1, out=views)[0] is views[0]
    for b, v, s in zip(bufs, views, single):
        assert np.array_equal(v, s)
        v[:] = 0x5A
        assert (b == 0x5A).all(), "bytes outside the destination were written"
    path = tmp_path / "a.jpg"
    path.write_bytes(streams[0])
    f = JPEGFrame.open(path)
    assert f.shape == (33, 70) and f.subsampling == "420" and len(f) == len(streams[0]) and np.array_equal(f.to_bgr(device=-1), single[0])
    for bad in (dict(entropy="lanes"), dict(as_tensor=True), dict(out=[views[0]])):
        with pytest.raises(ValueError):
            ops.jpeg_decode(streams, device=-1, **bad)
    with pytest.raises(ValueError, match="out"):
        ops.jpeg_decode(streams[0], device=-1, out=np.zeros((33, 70, 3), np.float32))
    with pytest.raises(TypeError):
        JPEGFrame(str(path))


# ---- hand-built streams ------------------------------------------------------------------------------------------------------------------
class _Writer:
    def __init__(self):
        self.bits = []

    def put(self, code, length):
        self.bits += [(code >> (length - 1 - i)) & 1 for i in range(length)]

    def bytes(self):
        b = self.bits + [1] * (-len(self.bits) % 8)
        out = bytearray()
        for i in range(0, len(b), 8):
            v = int("".join(map(str, b[i:i + 8])), 2)
            out.append(v)
            if v == 0xFF:
                out.append(0)
        return bytes(out)


DC0, AC0 = E.huff_codes(E.DC_BITS[0], E.DC_VAL), E.huff_codes(E.AC_BITS[0], E.AC_VAL[0])


def _mag(w, v):
    n = abs(v).bit_length()
    if n:
        w.put((v if v > 0 else v - 1) & ((1 << n) - 1), n)


def gray_stream(H, W, step, blocks=None, raw=None):
    """A gray baseline stream with the Annex K.3 luminance tables and every quantisation step = ``step``.  ``blocks``: per block a list
    of 64 coefficients in zigzag order (DC absolute).  ``raw``: a function that writes the entropy-coded bits itself."""
    w = _Writer()
    if raw is not None:
        raw(w)
    else:
        pred = 0
        for zz in blocks:
            d = zz[0] - pred
            pred = zz[0]
            w.put(*DC0[abs(d).bit_length()])
            _mag(w, d)
            run = 0
            for v in zz[1:]:
                if v == 0:
                    run += 1
                    continue
                while run >= 16:
                    w.put(*AC0[0xF0])
                    run -= 16
                w.put(*AC0[run << 4 | abs(v).bit_length()])
                _mag(w, v)
                run = 0
            if run:
                w.put(*AC0[0])
    seg = lambda m, body: bytes([0xFF, m]) + struct.pack(">H", len(body) + 2) + body
    return (b"\xff\xd8" + seg(0xDB, bytes([0]) + bytes([step] * 64)) + seg(0xC0, struct.pack(">BHHB", 8, H, W, 1) + bytes([1, 0x11, 0]))
            + seg(0xC4, bytes([0x00]) + bytes(E.DC_BITS[0]) + bytes(E.DC_VAL)) + seg(0xC4, bytes([0x10]) + bytes(E.AC_BITS[0]) + bytes(E.AC_VAL[0]))
            + seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + w.bytes() + b"\xff\xd9")


def test_known_answer_one_dc_coefficient():
    """Gray 8 x 8, one coefficient: DC = 5 with step 16, so the dequantised DC is 80.  Column pass (descale 11) of column 0, whose only
    input is v0 = 80: t0 = t1 = 80 << 13, every other term 0, so all eight outputs are (80 * 8192 + 1024) >> 11 = 320 (= 80 << 2: the two
    bits the pass keeps); the other columns are 0.  Row pass (descale 18) of a row (320, 0, ..., 0): every output is
    (320 * 8192 + 131072) >> 18 = 2752512 >> 18 = 10 (the real 10.5 = 84 / 8 rounded down by the shift: ((80 + 4) >> 3)).  Sample =
    10 + 128 = 138, and gray gives B = G = R."""
    d = gray_stream(8, 8, 16, [[5] + [0] * 63])
    want = np.full((8, 8, 3), ((80 + 4) >> 3) + 128, np.uint8)
    assert want[0, 0, 0] == 138
    assert np.array_equal(ops.jpeg_decode(d, device=-1), want)
    assert np.array_equal(checker(d)["bgr"], want) and np.array_equal(K.pillow_decode(d), want)
    assert np.array_equal(ops.jpeg_decode_coefficients(d, device=-1), np.array([[5] + [0] * 63], np.int16))


def test_extreme_coefficients_need_64_bits():
    """sixteen blocks whose DC climbs by 2047 a block to 32752 and falls back below -32000 (differences of category 11), every AC
    coefficient +-1023, step 255: 32-bit sums overflow in both passes; the checker's Python integers do not"""
    rng = np.random.default_rng(3)
    blocks, dc = [], 0
    for i in range(48):
        dc += 2047 if i < 16 else -2047 if dc > -32000 else 0
        ac = [int(s) * 1023 for s in rng.choice((-1, 1), 63)]
        if i % 3 == 1:
            ac = [1023] * 63
        if i % 3 == 2:
            ac = [a if k % 5 == 0 else 0 for k, a in enumerate(ac)]
        blocks.append([dc] + ac)
    assert max(b[0] for b in blocks) == 32752 and min(b[0] for b in blocks) < -32000
    d = gray_stream(16, 192, 255, blocks)
    want = checker(d)
    assert want["status"] == N.OK and np.array_equal(want["coefficients"], np.array(blocks, np.int16))
    assert np.array_equal(ops.jpeg_decode_coefficients(d, device=-1), want["coefficients"])
    got = ops.jpeg_decode(d, device=-1)
    assert np.array_equal(got, want["bgr"])
    assert 0 < (got == 0).sum() and 0 < (got == 255).sum()
    # on both sides of the bound up to which a block takes the 32-bit path: sums of |coef * step| of 4094, 4095 and 4096
    for tail in (1, 2, 3):
        for sign in (1, -1):
            d = gray_stream(8, 8, 1, [[2047 * sign, -1023 * sign, 1023, tail * sign] + [0] * 60])
            assert np.array_equal(ops.jpeg_decode(d, device=-1), checker(d)["bgr"]), (tail, sign)
            d = gray_stream(8, 8, 2, [[1023 * sign, 1023] + [0] * 61 + [tail * sign]])
            assert np.array_equal(ops.jpeg_decode(d, device=-1), checker(d)["bgr"]), (tail, sign)


@pytest.mark.parametrize("ss", ["420", "444"])
def test_round_trip_through_the_projects_encoder(ss):
    for name, frame in K.inputs():
        for q in (1, 60, 100):
            d = ops.jpeg_encode(np.ascontiguousarray(frame), quality=q, subsampling=ss, device=-1)
            assert np.array_equal(ops.jpeg_decode(d, device=-1), K.pillow_decode(d)), (name, q)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _segments(d):
    """-> [(marker, start, end)] of the marker segments in front of the scan"""
    out, p = [], 2
    while True:
        m, L = d[p + 1], d[p + 2] << 8 | d[p + 3]
        out.append((m, p, p + 2 + L))
        p += 2 + L
        if m == 0xDA:
            return out


def _patched(d, marker, offset, value):
    b = bytearray(d)
    _, s, _ = next(x for x in _segments(d) if x[0] == marker)
    b[s + offset] = value
    return bytes(b)


def _refused():
    import io
    from PIL import Image
    base = K.stream("33x70", "420", 85, "std")
    rst = K.stream("33x70", "420", 85, "rr1")
    segs = _segments(base)
    sos = next(x for x in segs if x[0] == 0xDA)
    dht = [x for x in segs if x[0] == 0xC4]
    buf = io.BytesIO()
    Image.fromarray(K._frames()["33x70"][..., ::-1].copy()).save(buf, "JPEG", progressive=True)
    prog = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 4), np.uint8), "CMYK").save(buf, "JPEG")
    cmyk = buf.getvalue()
    mid = sos[2] + (len(base) - sos[2]) // 2
    while base[mid - 1] == 0xFF or base[mid] == 0:
        mid += 1
    first_rst = rst.index(b"\xff\xd0", _segments(rst)[-1][2])
    return {
        "SOF1": (_patched(base, 0xC0, 1, 0xC1), "SOF1"),
        "SOF2": (prog, "SOF2"),
        "SOF9 arithmetic": (_patched(base, 0xC0, 1, 0xC9), "arithmetic"),
        "12-bit": (_patched(base, 0xC0, 4, 12), "12-bit"),
        "4 components": (cmyk, "4 components"),
        "sampling 4x1": (_patched(base, 0xC0, 11, 0x41), "sampling factors"),
        "sampling 1x2": (_patched(base, 0xC0, 11, 0x12), "sampling factors"),
        "chroma 2x1": (_patched(base, 0xC0, 14, 0x21), "sampling factors"),
        "several scans": (base[:sos[1]] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + base[sos[2]:], "several scans"),
        "DNL": (base[:sos[1]] + b"\xff\xdc\x00\x04\x00\x21" + base[sos[1]:], "DNL"),
        "missing Huffman table": (base[:dht[-1][1]] + base[dht[-1][2]:], "missing AC Huffman table"),
        "missing quantisation table": (_patched(base, 0xC0, 15, 3), "missing quantisation table"),
        "no EOI": (base[:-2], "no EOI"),
        "marker inside the scan": (base[:mid] + b"\xff\xe0" + base[mid:], "inside the scan"),
        "RST out of sequence": (rst[:first_rst + 1] + b"\xd3" + rst[first_rst + 2:], "out of sequence"),
        "RST without DRI": (base[:mid] + b"\xff\xd0" + base[mid:], "restart"),
        "not a JPEG": (b"\x89PNG" + base[4:], "SOI"),
    }


@pytest.mark.parametrize("name", list(_refused()))
def test_refused_streams(name):
    data, reason = _refused()[name]
    with pytest.raises(ValueError, match=reason):
        JPEGFrame(data)
    good = K.stream("17x17", "444", 85, "std")
    outs = [np.full((17, 17, 3), 0x5A, np.uint8), np.full((33, 70, 3), 0x5A, np.uint8)]
    with pytest.raises(ValueError, match=r"streams\[1\].*" + reason):
        ops.jpeg_decode([good, data], device=-1, out=outs)
    assert all((o == 0x5A).all() for o in outs), "a destination was written although a stream of the call is refused"


# ---- corrupt entropy-coded data ---------------------------------------------------------------------------------------------------------------
def _corrupt():
    base = K.stream("33x70", "420", 85, "std")
    sos_end = _segments(base)[-1][2]
    out = {"truncated segment": (base[:-40] + b"\xff\xd9", None),
           "bytes left over": (base[:-2] + b"\x12\x34\x56\xff\xd9", N.SEGMENT_LONG)}
    rng = np.random.default_rng(8)
    flips = 0
    while flips < 6:
        at, bit = int(rng.integers(sos_end, len(base) - 2)), int(rng.integers(0, 8))
        v = base[at] ^ (1 << bit)
        if base[at] in (0, 0xFF) or v in (0, 0xFF) or base[at - 1] == 0xFF:
            continue
        out[f"flipped bit {flips}"] = (base[:at] + bytes([v]) + base[at + 1:], None)
        flips += 1

    def run_past(w):
        w.put(*DC0[0])
        for _ in range(4):                                   # k = 1 -> 17 -> 33 -> 49 -> 65: the fourth run leaves the block
            w.put(*AC0[0xF1])
            w.put(1, 1)

    def zrl_past(w):
        w.put(*DC0[0])
        for _ in range(4):                                   # k = 1 -> 17 -> 33 -> 49 -> 65
            w.put(*AC0[0xF0])
        w.put(*AC0[0])

    def unknown(w):
        w.put(*DC0[0])
        w.put(0xFFFF, 16)                                    # sixteen 1-bits: the code the Annex K tables leave unused
        w.put(0, 16)

    out["run past 63"] = (gray_stream(8, 8, 16, raw=run_past), N.RUN_PAST_BLOCK)
    out["ZRL past 63"] = (gray_stream(8, 8, 16, raw=zrl_past), N.RUN_PAST_BLOCK)
    out["unknown 16-bit code"] = (gray_stream(8, 8, 16, raw=unknown), N.CODE_NOT_FOUND)
    out["segment short"] = (gray_stream(8, 16, 16, [[5] + [0] * 63]), N.SEGMENT_SHORT)
    return out


@pytest.mark.parametrize("name", list(_corrupt()))
def test_corrupt_entropy_data_on_the_host_twin(name):
    data, status = _corrupt()[name]
    want = checker(data)
    if status is not None:
        assert want["status"] == status
    f = JPEGFrame(data)                                       # the header is fine: nothing is refused at construction
    good = [K.stream("17x17", "444", 85, "std"), K.stream("20x5", "422", 50, "rb2")]
    outs = [np.full((17, 17, 3), 0x5A, np.uint8), np.full(f.shape + (3,), 0x5A, np.uint8), np.full((20, 5, 3), 0x5A, np.uint8)]
    if want["status"] == N.OK:                                # a flipped bit can leave a stream that still decodes: then to the checker's pixels
        ops.jpeg_decode([good[0], data, good[1]], device=-1, out=outs)
        assert np.array_equal(outs[1], want["bgr"])
    else:
        with pytest.raises(ValueError, match=r"streams\[1\]: corrupt entropy-coded data"):
            ops.jpeg_decode([good[0], data, good[1]], device=-1, out=outs)
        assert (outs[1] == 0x5A).all()
        from cvsd_amd import _lib
        import ctypes as C
        fr = [JPEGFrame(good[0]), f, JPEGFrame(good[1])]
        st = (C.c_int * 3)()
        od = (_lib.RenderOut * 3)(*[_lib.RenderOut(o.ctypes.data, o.strides[0], 0) for o in outs])
        assert _lib.lib().mi355_jpeg_decode(-1, (_lib.JpegStream * 3)(*[x.struct() for x in fr]), 3, 0, od, st, None, None) == -1
        assert list(st) == [0, want["status"], 0]
    assert np.array_equal(outs[0], checker(good[0])["bgr"]) and np.array_equal(outs[2], checker(good[1])["bgr"])


# ---- the shared routine under sanitizers, stand-alone ------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "computer-vision-shoplifting-detection_amd", "csrc")


def test_host_routine_under_sanitizers(tmp_path):
    """tools/jpeg_decode_host_drive.cpp and csrc/jpeg_decode_host.cpp, built without HIP and with -fsanitize=address,undefined, run
    mi355_jpeg_info / mi355_jpeg_decode(-1) / mi355_op_jpeg_decode_coefficients(-1) over the case table, every single-byte truncation of
    three small streams and seeded bit flips, every stream and destination in a heap block of exactly its size"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([cxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the AddressSanitizer / UBSan runtime is not on this machine")
    corpus = [K.stream(name, lay, q, enc) for _, name, lay, q, enc in K.case_ids()]
    corpus += [d for d, _ in _corrupt().values()] + [d for d, _ in _refused().values()]
    small = [K.stream("9x4", "420", 50, "opt"), K.stream("17x17", "422", 85, "rb2"), K.stream("8x8", "gray", 100, "std")]
    for d in small:
        corpus += [d[:k] for k in range(len(d))]
    rng = np.random.default_rng(21)
    for i in range(600):
        d = bytearray(small[i % 3] if i % 2 else K.stream("33x70", "420", 85, "rr1"))
        for _ in range(1 + i % 4):
            d[int(rng.integers(2, len(d)))] ^= 1 << int(rng.integers(0, 8))
        corpus.append(bytes(d))
    path = tmp_path / "corpus.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(corpus)))
        for d in corpus:
            f.write(struct.pack("<I", len(d)) + d)
    exe = tmp_path / "jpeg_decode_host_drive"
    r = subprocess.run([cxx, *flags, "-DMI355_JPEG_DECODE_STANDALONE", "-I", CSRC, os.path.join(ROOT, "tools", "jpeg_decode_host_drive.cpp"),
                        os.path.join(CSRC, "jpeg_decode_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "jpeg_decode_host_drive ok" in r.stdout and f"{len(corpus)} streams" in r.stdout, r.stdout
    decoded = int(r.stdout.split("decoded ")[1].split(",")[0])
    assert decoded >= len(K.case_ids())
