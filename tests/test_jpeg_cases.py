"""The JPEG encoder's host twin (``ops.jpeg_encode(..., device=-1)``: the routines of csrc/jpeg_codec.h in host loops) against the
sequential checker of tests/_jpeg_numpy.py, byte for byte over the case table; the stream's structure; a hand-derived known answer; and
three outside references: Pillow's quantisation tables, Pillow's decoder, and a float64 DCT (scipy).  No GPU is touched.

Fidelity against Pillow's own encoder, measured on this table (decode(ours) and decode(Pillow's stream at the same quality and
subsampling), PSNR against the source): at 4:4:4 the two are equal to 0.00 dB in every case -- colour conversion, DCT and quantisation
give libjpeg's numbers.  At 4:2:0 Pillow is ahead on the integer-slope gradients at high quality: 4.59 dB at worst ("1x40", quality
100: 47.34 against 51.93 dB), 2.87 dB the same frame at 85, 2.07 dB "33x70" at 100, under 0.05 dB on the smooth_bright and rows cases.
The cause is the stated chroma rule, (a + b + c + d + 2) >> 2, which rounds every half up, where libjpeg alternates the bias between 1
and 2: on a gradient whose four-sample sums are odd half the time that is a quarter-level offset in Cb and Cr, which is the whole error
budget at quality 100 (an MSE of 1.2 against 0.4), and a frame one pixel high doubles it (its rows are repeated, so every sum is
2 (a + b)).  MAX_GAP_DB is the worst figure plus 0.1."""
import ctypes as C
import io

import numpy as np
import pytest
from PIL import Image

import _jpeg_cases as K
import _jpeg_numpy as J
from cvsd_amd import _lib, ops

CASES = K.cases()
IDS = [c[0] for c in CASES]
MAX_GAP_DB = 4.59 + 0.1
ORDER = [0xD8, 0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA, 0xD9]


@pytest.fixture(scope="module")
def streams():
    """the host twin's stream of every case, one call per quality and subsampling over all inputs"""
    out = {}
    frames = [f for _, f, _ in K.inputs()]
    for ss in K.SUBSAMPLINGS:
        for q in K.QUALITIES:
            for (name, _, _), b in zip(K.inputs(), ops.jpeg_encode(frames, quality=q, subsampling=ss, device=-1)):
                out[f"{name}-{ss}-q{q}"] = b
    return out


def _decode(b):
    im = Image.open(io.BytesIO(b))
    im.load()
    return im


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / max(float(((a.astype(np.float64) - b) ** 2).mean()), 1e-10))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_twin_matches_checker(streams, case):
    cid, frame, q, ss, _ = case
    keep = frame.copy()
    got, want = streams[cid], J.encode(np.ascontiguousarray(frame), q, ss)
    assert np.array_equal(frame, keep)
    assert isinstance(got, bytes) and len(got) == len(want), (len(got), len(want))
    bad = [i for i in range(len(got)) if got[i] != want[i]]
    assert not bad, f"{len(bad)} bytes differ, first at {bad[0]}: got {got[bad[0]]:02x}, want {want[bad[0]]:02x}"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_marker_walk_and_pillow_decode(streams, case):
    cid, frame, q, ss, _ = case
    h, w = frame.shape[:2]
    info = J.parse(streams[cid])
    assert [m for m, _ in info["markers"]] == ORDER
    assert [n for _, n in info["markers"]] == [0, 16, 67, 67, 17, 31, 181, 31, 181, 4, 12, 0]
    assert info["app0"] == b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"
    assert info["sof"] == {"precision": 8, "height": h, "width": w, "components": [(1, 0x22 if ss == "420" else 0x11, 0), (2, 0x11, 1), (3, 0x11, 1)]}
    m = 16 if ss == "420" else 8
    assert info["dri"] == -(-w // m)
    rows = -(-h // m)
    assert info["rst"] == [r % 8 for r in range(rows - 1)] and len(info["segments"]) == rows
    assert sorted(info["dht"]) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert info["sos"] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert np.array_equal(info["coefficients"], J.coefficients(np.ascontiguousarray(frame), q, ss))
    im = _decode(streams[cid])
    assert im.size == (w, h) and im.mode == "RGB"


def test_case_table_reaches_the_rules(streams):
    """ZRL, blocks without EOB, stuffed bytes and a wrapping RST index all occur: a table without them would check nothing"""
    dense = J.parse(streams["dense8x8-444-q100"])["coefficients"]
    assert (dense[:, 63] != 0).any() and (dense[0] != 0).all(), "no block without a zero: the no-EOB path is not reached"
    assert b"\xff\x00" in J.parse(streams["noise33x70-444-q100"])["scan"]
    assert 9 in [len(J.parse(streams[f"rows{n}-{ss}-q50"])["segments"]) for n, ss in (("72x8", "444"), ("144x8", "420"))]
    assert J.parse(streams["rows144x8-420-q85"])["rst"] == [0, 1, 2, 3, 4, 5, 6, 7]
    assert J.parse(streams["rows144x8-444-q85"])["rst"] == [0, 1, 2, 3, 4, 5, 6, 7] * 2 + [0]
    zz = J.parse(streams["smooth_bright48x64-420-q100"])["coefficients"]
    gaps = [np.diff(np.flatnonzero(np.r_[1, b[1:]])).max(initial=0) for b in zz]     # distance between neighbouring non-zero coefficients
    assert max(gaps) > 32, "no run of 32 zeros before a coefficient: two ZRL in a row are not reached"
    assert max(np.diff(np.flatnonzero(np.r_[1, b[1:]])).max(initial=0) for b in J.parse(streams["noise33x70-444-q1"])["coefficients"]) > 48
    zz = J.parse(streams["smooth_bright48x64-444-q85"])["coefficients"]
    assert (np.abs(zz[:, 8:]).sum(axis=1) == 0).any(), "no block that ends after a few coefficients"


def test_known_answer_grey_block():
    """8 x 8 of BGR (128, 128, 128) at 4:4:4: Y = Cb = Cr = 128, every coefficient 0.  Per block DC difference 0 and EOB: luminance
    00 + 1010, chrominance 00 + 00 twice -> 001010 0000 0000, padded with two 1-bits: 0010 1000 0000 0011 = 28 03, then EOI."""
    b = ops.jpeg_encode(np.full((8, 8, 3), 128, np.uint8), quality=85, subsampling="444", device=-1)
    assert b[-4:] == bytes([0x28, 0x03, 0xFF, 0xD9]) and J.parse(b)["scan"] == bytes([0x28, 0x03])
    assert np.array_equal(np.asarray(_decode(b)), np.full((8, 8, 3), 128, np.uint8))


@pytest.mark.parametrize("q", [1, 25, 50, 75, 85, 95, 100])
def test_quant_tables_equal_pillows(q, tmp_path):
    f = K.inputs()[4][1]
    p = tmp_path / "pil.jpg"
    Image.fromarray(f).save(p, "JPEG", quality=q)
    theirs = Image.open(p).quantization                        # natural order
    ours = _decode(ops.jpeg_encode(f, quality=q, device=-1)).quantization
    assert sorted(ours) == [0, 1] and all(list(ours[i]) == list(theirs[i]) for i in (0, 1))
    info = J.parse(ops.jpeg_encode(f, quality=q, device=-1))
    for i, base in ((0, J.K1), (1, J.K2)):
        assert [info["dqt"][i][k] for k in range(64)] == [list(theirs[i])[J.ZIGZAG[k]] for k in range(64)] == \
               [J.quant_table(base, q)[J.ZIGZAG[k]] for k in range(64)]


@pytest.mark.parametrize("ss", K.SUBSAMPLINGS)
def test_coefficients_within_one_of_a_float_dct(ss):
    """the integer DCT against scipy's float64 DCT of the same level-shifted samples, same quantisation steps: never more than 1 apart
    (the share of coefficients that differ at all is recorded in DESIGN.md 3.20)"""
    from scipy.fft import dctn
    differ = total = 0
    for name, frame, _ in K.inputs():
        frame = np.ascontiguousarray(frame)
        for q in K.QUALITIES:
            got = ops.jpeg_coefficients(frame, quality=q, subsampling=ss, device=-1)
            assert got.dtype == np.int16 and np.array_equal(got, J.coefficients(frame, q, ss)), (name, q)
            h, w = frame.shape[:2]
            m = 16 if ss == "420" else 8
            H, W = -(-h // m) * m, -(-w // m) * m
            pad = frame[np.minimum(np.arange(H), h - 1)][:, np.minimum(np.arange(W), w - 1)].astype(np.int64)
            ycc = np.stack(J.ycc(pad[..., 0], pad[..., 1], pad[..., 2]))
            steps = [np.array(J.quant_table(b, q))[J.ZIGZAG] for b in (J.K1, J.K2)]
            want = []
            for my in range(H // m):
                for mx in range(W // m):
                    tile = ycc[:, my * m:(my + 1) * m, mx * m:(mx + 1) * m]
                    if ss == "420":
                        c = (tile[1:, 0::2, 0::2] + tile[1:, 0::2, 1::2] + tile[1:, 1::2, 0::2] + tile[1:, 1::2, 1::2] + 2) >> 2
                        blocks = [(0, tile[0, y:y + 8, x:x + 8]) for y in (0, 8) for x in (0, 8)] + [(1, c[0]), (1, c[1])]
                    else:
                        blocks = [(0, tile[0]), (1, tile[1]), (1, tile[2])]
                    for tc, b in blocks:
                        d = dctn(b.astype(np.float64) - 128.0, norm="ortho").reshape(64)[J.ZIGZAG] / steps[tc]
                        want.append(np.sign(d) * np.floor(np.abs(d) + 0.5))
            want = np.array(want)
            assert want.shape == got.shape
            assert np.abs(got - want).max() <= 1, (name, q, float(np.abs(got - want).max()))
            differ += int((got != want).sum())
            total += got.size
    print(f"{ss}: {differ} of {total} coefficients differ from the float64 DCT's ({100.0 * differ / total:.3f} %)")


def test_fidelity_against_pillows_encoder(streams):
    worst = (0.0, None)
    for cid, frame, q, ss, fid in CASES:
        if not fid:
            continue
        rgb = np.ascontiguousarray(frame[..., ::-1])
        ours = _psnr(np.asarray(_decode(streams[cid])), rgb)
        buf = io.BytesIO()
        Image.fromarray(rgb).save(buf, "JPEG", quality=q, subsampling={"420": 2, "444": 0}[ss])
        theirs = _psnr(np.asarray(_decode(buf.getvalue())), rgb)
        print(f"{cid}: ours {ours:.2f} dB, Pillow {theirs:.2f} dB, {len(streams[cid])} and {len(buf.getvalue())} bytes")
        if theirs - ours > worst[0]:
            worst = (theirs - ours, cid)
    print("worst gap", worst)
    assert worst[0] <= MAX_GAP_DB, worst


def test_pitched_view_and_mixed_sizes_in_one_call():
    big = np.random.default_rng(4).integers(0, 256, (40, 100, 3), dtype=np.uint8)
    view = big[3:36, 7:77]
    small = K.inputs()[0][1]
    got = ops.jpeg_encode([view, small, big], quality=70, subsampling="420", device=-1)
    assert got[0] == ops.jpeg_encode(np.ascontiguousarray(view), quality=70, device=-1) == J.encode(np.ascontiguousarray(view), 70, "420")
    assert got[1] == ops.jpeg_encode(small, quality=70, device=-1) and got[2] == ops.jpeg_encode(big, quality=70, device=-1)


def test_bad_arguments_are_refused_before_any_write():
    f = K.inputs()[4][1]
    lib = _lib.lib()
    cap = int(lib.mi355_jpeg_bound(16, 16, 420))
    assert cap == 640 + 6 * 416 + 2 + 2 and lib.mi355_jpeg_bound(0, 16, 420) == 0 and lib.mi355_jpeg_bound(16, 16, 422) == 0
    assert lib.mi355_jpeg_bound(1080, 1920, 420) == 640 + 68 * 120 * 6 * 416 + 2 * 68 + 2
    buf = np.full(cap + 64, 0xA5, np.uint8)

    def call(h, w, q, ss, capacity=cap, pitch=None):
        fr = (_lib.RenderFrame * 1)(_lib.RenderFrame(f.ctypes.data, h, w, pitch or 3 * 16, 0))
        out = (_lib.JpegOut * 1)(_lib.JpegOut(buf.ctypes.data + 32, capacity, -7))
        rc = lib.mi355_jpeg_encode(-1, fr, 1, q, ss, out, None, None)
        return rc, lib.mi355_last_error().decode(), out[0].length

    for args, word in (((16, 16, 0, 420), "quality"), ((16, 16, 101, 420), "quality"), ((16, 16, 85, 422), "subsampling"),
                       ((0, 16, 85, 420), "height"), ((16, 0, 85, 420), "width"), ((65536, 16, 85, 420), "height"),
                       ((16, 65536, 85, 420), "width"), ((16, 16, 85, 420, cap - 1), "capacity"), ((16, 16, 85, 420, cap, 47), "row_stride")):
        rc, msg, length = call(*args)
        assert rc == -1 and word in msg, (args, rc, msg)
        assert length == -7 and (buf == 0xA5).all(), f"{args}: written before the refusal"
    rc, _, length = call(16, 16, 85, 420)
    assert rc == 0 and (buf[:32] == 0xA5).all() and (buf[32 + length:] == 0xA5).all() and bytes(buf[32:32 + length]) == ops.jpeg_encode(f, device=-1)
    for kw in (dict(quality=0), dict(quality=101), dict(subsampling="422")):
        with pytest.raises(ValueError):
            ops.jpeg_encode(f, device=-1, **kw)
    with pytest.raises(ValueError):
        ops.jpeg_encode(np.zeros((0, 4, 3), np.uint8), device=-1)


def test_results_save_and_spec(tmp_path):
    from cvsd_amd import JpegSpec, Results
    from cvsd_amd.jpeg import as_spec
    assert as_spec(None) is None and as_spec("jpeg") == JpegSpec(85, "420", False) and as_spec({"quality": 60}).quality == 60
    for bad in (dict(quality=0), dict(quality=101), dict(quality=85.5), dict(subsampling="422")):
        with pytest.raises(ValueError):
            JpegSpec(**bad)
    with pytest.raises(TypeError):
        as_spec("png")
    r = Results(None, "image0.jpg", {0: "person"}, orig_shape=(8, 8))
    with pytest.raises(ValueError, match="encode="):
        r.save(tmp_path / "none.jpg")
    r.jpeg = ops.jpeg_encode(np.full((8, 8, 3), 128, np.uint8), device=-1)
    p = r.save(tmp_path / "evidence.jpg")
    assert open(p, "rb").read() == r.jpeg and Image.open(p).size == (8, 8)
