"""``entropy="sync"`` on the CPU (csrc/jpeg_sync.h): the host twin of the self-synchronising parallel Huffman decoder --
the kernels' rounds executed synchronously -- against the sequential routine (``entropy="host"``) and Pillow on every case of the table
and on the longer inputs of tests/_jpeg_sync_cases.py; the hook's entry states and block indices against the one sequential bit walk
of tests/_jpeg_sync_numpy.py at four (sub_bytes, seq_subs) settings; that the inputs really take several local and global rounds and a
start on a stuffing zero; corrupt and refused streams; per-frame requests in one call; a hand-derived known answer; and the twin under
AddressSanitizer / UBSan in a stand-alone program.  Integer arithmetic: nothing here has a tolerance."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import _jpeg_decode_cases as K
import _jpeg_decode_numpy as N
import _jpeg_sync_cases as S
import _jpeg_sync_numpy as Y
import test_jpeg_decode_cases as D
from cvsd_amd import JPEGFrame, _lib, ops

GROUPS = S.groups()
NEW = S.case_ids()
_states = {}


def states(data, sub_bytes):
    if (data, sub_bytes) not in _states:
        _states[(data, sub_bytes)] = Y.entry_states(data, sub_bytes)
    return _states[(data, sub_bytes)]


def test_the_new_inputs_are_what_they_say():
    assert len(NEW) == 4 * 4 * 2 * 3 and len(GROUPS) == len(K.groups()) + 16
    d = S.stream("noise48x64", "444", 100, "std")
    P = N.parse(d)
    (b0, b1), = P["segments"]
    assert 12000 < b1 - b0 < 13500 and d[b0:b1].count(b"\xff\x00") >= 50
    d = S.stream("noise96x128", "444", 100, "std")
    (b0, b1), = N.parse(d)["segments"]
    assert b1 - b0 > 128 * 256
    assert JPEGFrame(S.stream("noise96x128", "420", 50, "rr1")).segments == 6


# ---- 1. the twin against the sequential routine and Pillow -------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS), ids=lambda g: f"{g[0]}-{g[1]}")
def test_sync_twin_equals_the_sequential_routine_and_pillow(group):
    streams = [S.stream(group[0], group[1], q, enc) for _, q, enc in GROUPS[group]]
    info = []
    pix = ops.jpeg_decode(streams, device=-1, entropy="sync", timing=info)
    assert info[0]["entropy"] == ["sync"] * len(streams)
    coef = ops.jpeg_decode_coefficients(streams, device=-1, entropy="sync")
    want = ops.jpeg_decode_coefficients(streams, device=-1, entropy="host")
    for (cid, _, _), d, p, c, w in zip(GROUPS[group], streams, pix, coef, want):
        assert c.dtype == np.int16 and np.array_equal(c, w), cid
        assert np.array_equal(p, K.pillow_decode(d)), cid


# ---- 2. the hook: coefficients, entry states and block indices -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NEW, ids=[c[0] for c in NEW])
def test_hook_states_equal_the_checker(case):
    d = S.stream(*case[1:])
    want = ops.jpeg_decode_coefficients(d, device=-1, entropy="host")
    for sub, seq in S.SETTINGS:
        got = ops.jpeg_sync(d, -1, sub, seq)
        ref = states(d, sub)
        assert got["status"] == 0 and np.array_equal(got["coefficients"], want), (sub, seq)
        assert got["stats"]["nsub"] == len(ref) and got["states"].shape == ref.shape, (sub, seq)
        idle = ref[:, 1] < 0                                  # behind the segment's last boundary: only "B is at the count" is defined
        assert idle.sum() <= JPEGFrame(d).segments and (got["states"][idle, 0] == ref[idle, 0]).all() and (got["states"][idle, 5] >= ref[idle, 5]).all()
        bad = np.flatnonzero((got["states"] != ref).any(axis=1) & ~idle)
        assert bad.size == 0, (sub, seq, int(bad[0]), got["states"][bad[0]].tolist(), ref[bad[0]].tolist())


def test_hook_arguments():
    d = S.stream("flat64x96", "420", 50, "std")
    for bad in ((4, 4), (12, 4), (8, 1), (8, 257)):
        with pytest.raises(ValueError):
            ops.jpeg_sync(d, -1, *bad)
    with pytest.raises(ValueError):
        ops.jpeg_sync([d, d], -1, 8, 4)
    for bad in ("lanes", "parallel", 3):
        with pytest.raises(ValueError):
            ops.jpeg_decode(d, device=-1, entropy=bad)
        with pytest.raises(ValueError):
            ops.jpeg_decode_coefficients(d, device=-1, entropy=bad)
        with pytest.raises(ValueError):
            JPEGFrame(d, entropy=bad)
    f = JPEGFrame(d)
    sd = (_lib.JpegStream * 1)(_lib.JpegStream(f._buf.ctypes.data, len(d), 0, 7))
    out = np.zeros((64, 96, 3), np.uint8)
    od = (_lib.RenderOut * 1)(_lib.RenderOut(out.ctypes.data, out.strides[0], 0))
    assert _lib.lib().mi355_jpeg_decode(-1, sd, 1, 0, od, None, None, None) == -1 and not out.any()
    assert _lib.lib().mi355_jpeg_decode(-1, sd, 1, 4, od, None, None, None) == -1


# ---- 3. the hard paths are really taken -----------------------------------------------------------------------------------------------------
def test_the_inputs_take_several_rounds_and_a_stuffed_start():
    d = S.stream("noise48x64", "444", 100, "std")
    for sub, seq in ((8, 64), (16, 16)):
        st = ops.jpeg_sync(d, -1, sub, seq)["stats"]
        assert st["rounds_local"] >= 2 and st["rounds_global"] >= 2, (sub, seq, st)
        assert st["nseq"] == -(-st["nsub"] // seq)
    assert Y.stuffing_starts(d, 8) >= 1
    first = states(d, 8)
    starts = np.arange(len(first)) * 8
    assert (first[:, 1] >= starts).all()
    st = ops.jpeg_sync(S.stream("noise96x128", "444", 100, "std"), -1, 128, 256)["stats"]
    assert st["nseq"] >= 2, st


# ---- 4. corrupt and refused streams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D._corrupt()))
def test_corrupt_streams_on_the_sync_twin(name):
    data, _ = D._corrupt()[name]
    f = JPEGFrame(data)
    good = [K.stream("17x17", "444", 85, "std"), K.stream("20x5", "422", 50, "rb2")]
    fr = [JPEGFrame(good[0]), f, JPEGFrame(good[1])]
    status = {}
    for entropy in ("host", "sync"):
        outs = [np.full((17, 17, 3), 0x5A, np.uint8), np.full(f.shape + (3,), 0x5A, np.uint8), np.full((20, 5, 3), 0x5A, np.uint8)]
        st = (C.c_int * 3)()
        od = (_lib.RenderOut * 3)(*[_lib.RenderOut(o.ctypes.data, o.strides[0], 0) for o in outs])
        rc = _lib.lib().mi355_jpeg_decode(-1, (_lib.JpegStream * 3)(*[x.struct() for x in fr]), 3, _lib.JPEG_ENTROPY[entropy], od, st, None, None)
        status[entropy] = (rc, list(st))
        assert np.array_equal(outs[0], K.pillow_decode(good[0])) and np.array_equal(outs[2], K.pillow_decode(good[1]))
        if st[1]:
            assert rc == -1 and (outs[1] == 0x5A).all()
        else:
            assert rc == 0 and np.array_equal(outs[1], ops.jpeg_decode(data, device=-1, entropy="host"))
    assert status["sync"] == status["host"], status
    for sub, seq in ((8, 4), (128, 256)):
        assert ops.jpeg_sync(data, -1, sub, seq)["status"] == status["host"][1][1]
    if status["host"][1][1]:
        with pytest.raises(ValueError, match=r"streams\[1\]: corrupt entropy-coded data"):
            ops.jpeg_decode([good[0], data, good[1]], device=-1, entropy="sync")


@pytest.mark.parametrize("name", list(D._refused()))
def test_refused_streams_on_the_sync_twin(name):
    data, reason = D._refused()[name]
    good = K.stream("17x17", "444", 85, "std")
    f = JPEGFrame(good, entropy="sync")
    outs = [np.full((17, 17, 3), 0x5A, np.uint8), np.full((33, 70, 3), 0x5A, np.uint8)]
    with pytest.raises(ValueError, match=r"streams\[1\].*" + reason):
        ops.jpeg_decode([good, data], device=-1, out=outs, entropy="sync")
    buf = np.frombuffer(data, np.uint8)
    sd = (_lib.JpegStream * 2)(f.struct(), _lib.JpegStream(buf.ctypes.data, len(data), 0, 3))
    od = (_lib.RenderOut * 2)(*[_lib.RenderOut(o.ctypes.data, o.strides[0], 0) for o in outs])
    assert _lib.lib().mi355_jpeg_decode(-1, sd, 2, 3, od, None, None, None) == -1
    assert all((o == 0x5A).all() for o in outs), "a destination was written although a stream of the call is refused"
    with pytest.raises(ValueError, match=reason):
        ops.jpeg_sync(data, -1, 8, 4)


# ---- 5. per-frame requests in one call ----------------------------------------------------------------------------------------------------------
def test_mixed_requests_in_one_call():
    picks = [("noise48x64", "444", 100, "std", "sync"), ("33x70", "420", 85, "rr1", "gpu"), ("flat64x96", "422", 50, "opt", "host"),
             ("smooth64x96", "gray", 100, "rr1", "sync"), ("17x17", "444", 100, "opt", None), ("noise96x128", "420", 50, "std", "sync")]
    frames = [JPEGFrame(S.stream(*p[:4]), entropy=p[4]) for p in picks]
    single = [ops.jpeg_decode(f.data, device=-1) for f in frames]
    info = []
    got = ops.jpeg_decode(frames, device=-1, timing=info)
    assert info[0]["entropy"] == ["sync", "host", "host", "sync", "host", "sync"]      # the twin has no lanes: "gpu" runs on the host
    for g, s in zip(got, single):
        assert np.array_equal(g, s)
    coef = ops.jpeg_decode_coefficients(frames, device=-1, entropy="sync")
    for c, f in zip(coef, frames):
        assert np.array_equal(c, ops.jpeg_decode_coefficients(f.data, device=-1, entropy="host"))
    again = JPEGFrame(frames[0])
    assert again.entropy == "sync" and JPEGFrame(frames[0], entropy="host").entropy == "host" and JPEGFrame(frames[4]).entropy is None
    assert frames[0].struct().entropy == 3 and frames[4].struct().entropy == 0 and JPEGFrame(frames[0].data, entropy="auto").struct().entropy == 0


def test_captures_pass_the_request_through(tmp_path):
    from cvsd_amd.preprocess_driver import ImageDirCapture, MjpegCapture
    a, b = S.stream("flat64x96", "420", 50, "std"), S.stream("smooth64x96", "444", 50, "std")
    (tmp_path / "clip").mkdir()
    (tmp_path / "clip" / "0001.jpg").write_bytes(a)
    (tmp_path / "clip.mjpeg").write_bytes(a + b)
    for cap, n in ((ImageDirCapture(str(tmp_path / "clip"), decode=False, entropy="sync"), 1), (MjpegCapture(str(tmp_path / "clip.mjpeg"), entropy="sync"), 2)):
        for _ in range(n):
            ok, f = cap.read()
            assert ok and isinstance(f, JPEGFrame) and f.entropy == "sync"
            info = []
            ops.jpeg_decode(f, device=-1, timing=info)
            assert info[0]["entropy"] == ["sync"]
    ok, f = MjpegCapture(str(tmp_path / "clip.mjpeg")).read()
    assert ok and f.entropy is None


# ---- 6. a hand-derived known answer ----------------------------------------------------------------------------------------------------------
def test_known_answer_states_of_a_hand_built_stream():
    """tests/_jpeg_sync_cases.py derives the three entry states at sub_bytes = 8 bit by bit"""
    d = S.known_stream()
    want = np.array(S.KNOWN_COEFFICIENTS, np.int16)
    assert np.array_equal(ops.jpeg_decode_coefficients(d, device=-1, entropy="host"), want)
    for seq in (2, 256):
        got = ops.jpeg_sync(d, -1, 8, seq)
        assert got["status"] == 0 and np.array_equal(got["coefficients"], want)
        assert got["states"].tolist() == [list(s) for s in S.KNOWN_STATES]
        assert (got["stats"]["nsub"], got["stats"]["nseq"]) == (3, 2 if seq == 2 else 1)
    assert Y.entry_states(d, 8).tolist() == [list(s) for s in S.KNOWN_STATES]
    assert np.array_equal(ops.jpeg_decode(d, device=-1, entropy="sync"), K.pillow_decode(d))


# ---- 7. the twin under sanitizers, stand-alone -------------------------------------------------------------------------------------------------
def test_sync_twin_under_sanitizers(tmp_path):
    """tools/jpeg_sync_host_drive.cpp and csrc/jpeg_decode_host.cpp, built without HIP and with -fsanitize=address,undefined, run
    mi355_jpeg_decode(-1, ..., SYNC) and the hook at sub_bytes 8 and 128 over the case table with the new inputs, every single-byte
    truncation of three small streams, seeded bit flips and the corrupt and refused streams; every buffer in a heap block of exactly
    its size; the statuses must be the sequential routine's"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run([cxx, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the AddressSanitizer / UBSan runtime is not on this machine")
    corpus = [K.stream(name, lay, q, enc) for _, name, lay, q, enc in K.case_ids()] + [S.stream(*c[1:]) for c in NEW] + [S.known_stream()]
    corpus += [d for d, _ in D._corrupt().values()] + [d for d, _ in D._refused().values()]
    small = [K.stream("9x4", "420", 50, "opt"), K.stream("17x17", "422", 85, "rb2"), K.stream("8x8", "gray", 100, "std")]
    for d in small:
        corpus += [d[:k] for k in range(len(d))]
    rng = np.random.default_rng(22)
    flip = small + [K.stream("33x70", "420", 85, "rr1"), K.stream("33x70", "444", 100, "std"), S.stream("noise48x64", "420", 50, "std")]
    for i in range(900):
        d = bytearray(flip[i % len(flip)])
        for _ in range(1 + i % 4):
            d[int(rng.integers(2, len(d)))] ^= 1 << int(rng.integers(0, 8))
        corpus.append(bytes(d))
    path = tmp_path / "corpus.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(corpus)))
        for d in corpus:
            f.write(struct.pack("<I", len(d)) + d)
    exe = tmp_path / "jpeg_sync_host_drive"
    r = subprocess.run([cxx, *flags, "-DMI355_JPEG_DECODE_STANDALONE", "-I", D.CSRC, os.path.join(D.ROOT, "tools", "jpeg_sync_host_drive.cpp"),
                        os.path.join(D.CSRC, "jpeg_decode_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "jpeg_sync_host_drive ok" in r.stdout and f"{len(corpus)} streams" in r.stdout, r.stdout
    decoded = int(r.stdout.split("decoded ")[1].split(",")[0])
    corrupt = int(r.stdout.split("corrupt ")[1].split()[0])
    assert decoded >= len(K.case_ids()) + len(NEW) and corrupt >= 100
