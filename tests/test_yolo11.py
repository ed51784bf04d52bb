"""YOLO11 without a GPU: the program against the public model cards, its well-formedness with the new op types, the .mi355w v2
image (round trip, loader validation through the host-only memory planner), the converter on fabricated YOLO11 pickles, the
v8 / v5u images pinned byte for byte, and the graph checked against an independent torch restatement (tests/_yolo11_torch.py)."""
import hashlib
import os
import struct
import sys

import numpy as np
import pytest

from cvsd_amd.graph import (OP_ATTN, OP_CONV, OP_DWCONV, OP_SPPF_POOL, OP_STEM, OP_UPSAMPLE, build_program,
                            merge_sibling_convs, parse_model_name)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# Ultralytics YOLO11 model cards: (params M, GFLOPs at 640).  The pose cards are the yolo11-pose.yaml builds, whose Detect part
# is sized for nc: 80 (the COCO-pose checkpoints themselves carry nc = 1 and are ~0.03 M / 0.2 GFLOPs smaller).
CARDS = {"yolo11n": (2.6, 6.5), "yolo11s": (9.4, 21.5), "yolo11m": (20.1, 68.0), "yolo11l": (25.3, 86.9), "yolo11x": (56.9, 194.9),
         "yolo11n-pose": (2.9, 7.6), "yolo11s-pose": (9.9, 23.2), "yolo11m-pose": (20.9, 71.7)}


@pytest.mark.parametrize("name", sorted(CARDS))
def test_param_count_and_gflops_match_model_card(name):
    fam, scale, task = parse_model_name(name)
    prog = build_program(fam, scale, task, nc=80)
    params, gflops = CARDS[name]
    assert abs(prog.param_count() / 1e6 - params) < 0.05, prog.param_count()
    assert abs(2 * prog.macs() / 1e9 - gflops) < 0.06, 2 * prog.macs() / 1e9


def test_exact_fused_counts():
    assert build_program("v11", "n").param_count() == 2616248
    assert build_program("v11", "s").param_count() == 9443760


def test_parse_model_names():
    assert parse_model_name("yolo11n.pt") == ("v11", "n", "detect")
    assert parse_model_name("yolo11x-pose") == ("v11", "x", "pose")
    assert parse_model_name("yolov8n") == ("v8", "n", "detect")
    for bad in ("yolov11n", "yolo11q", "yolo12n"):
        with pytest.raises(ValueError):
            parse_model_name(bad)


@pytest.mark.parametrize("name", ["yolo11n", "yolo11m-pose", "yolo11x"])
@pytest.mark.parametrize("merged", [False, True])
def test_program_is_well_formed(name, merged):
    prog = build_program(*parse_model_name(name))
    if merged:
        prog = merge_sibling_convs(prog)[0]
    written = {}
    n_dw = n_attn = 0
    for op in prog.ops:
        if op.type in (OP_CONV, OP_UPSAMPLE, OP_SPPF_POOL, OP_DWCONV, OP_ATTN):
            for c in range(op.src.choff, op.src.choff + op.src.c):
                assert (op.src.buf, c) in written, (name, op)
        if op.res is not None:
            assert all((op.res.buf, c) in written for c in range(op.res.choff, op.res.choff + op.dst.c))
        n_out = 3 * op.src.c if op.type == OP_SPPF_POOL else op.dst.c
        assert op.dst.choff % 4 == 0 and op.dst.choff + n_out <= prog.buffers[op.dst.buf][0]
        for c in range(op.dst.choff, op.dst.choff + n_out):
            assert (op.dst.buf, c) not in written, "channel written twice"
            written[(op.dst.buf, c)] = True
        if op.type in (OP_CONV, OP_STEM, OP_DWCONV):
            cv = prog.convs[op.conv]
            assert cv.cout == op.dst.c and (op.type == OP_STEM or cv.cin == op.src.c)
            assert (cv.groups == cv.cin) == (op.type == OP_DWCONV)
        if op.type == OP_DWCONV:
            n_dw += 1
            assert op.src.c == op.dst.c and op.k == 3 and op.s == 1
            assert prog.buffers[op.src.buf][1] == prog.buffers[op.dst.buf][1]
        if op.type == OP_ATTN:
            n_attn += 1
            assert (op.k, op.s) == (32, 64) and op.src.c == op.heads * 128 and op.dst.c == op.heads * 64
            assert prog.buffers[op.src.buf][1] == 32
    depth = {"n": 1, "m": 1, "x": 2}[name[6]]
    assert n_attn == depth and n_dw == depth + 6               # pe per PSABlock + two DWConv per head level
    assert len(prog.levels) == 3 and [lv.stride for lv in prog.levels] == [8, 16, 32]


def test_v8_and_v5u_programs_are_unchanged():
    """no new op type and no permuted / grouped conv in the families that existed before"""
    for fam in ("v8", "v5u"):
        for scale in "nsmlx":
            prog = build_program(fam, scale)
            assert all(op.type in (OP_STEM, OP_CONV, OP_UPSAMPLE, OP_SPPF_POOL) for op in prog.ops)
            assert all(c.groups == 1 and c.rows is None and c.sd_name is None for c in prog.convs)


# sha256 of the seed-0 synthetic images, computed on the commit before YOLO11 support (shipped plans/ are keyed by image hash)
PINNED = {"yolov8n": "481b968a25e5289bdf0015ba5a9fb8f0387b1ba0979ae55d6277f52bfc35c93f",
          "yolov5mu": "6cae011959dde39420df9cde1f2629cdff1ad7f33569d917d5b449b3a4158521"}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_v8_and_v5u_images_are_byte_identical(name):
    from cvsd_amd import weights
    from tools import synth
    _, sd = synth.synthetic_checkpoint(name, seed=0)
    blob = weights.build_from_state_dict(name, sd)
    assert struct.unpack_from("<I", blob, 8)[0] == 1
    assert hashlib.sha256(blob).hexdigest() == PINNED[name]


@pytest.fixture(scope="module")
def y11n():
    from tools import synth
    return synth.synthetic_checkpoint("yolo11n", seed=0)


def test_mi355w_round_trip(y11n):
    from cvsd_amd import weights
    prog0, sd = y11n
    blob = weights.build_from_state_dict("yolo11n", sd)
    assert struct.unpack_from("<I", blob, 8)[0] == 2
    prog, fused, meta = weights.from_bytes(blob)
    assert prog.family == "v11" and meta["model"] == "yolo11n"
    want_prog, want_fused = merge_sibling_convs(prog0, weights.fuse_state_dict(prog0, sd))
    assert [(o.type, o.k, o.s, o.act, o.heads) for o in prog.ops] == [(o.type, o.k, o.s, o.act, o.heads) for o in want_prog.ops]
    for a, b in zip(prog.convs, want_prog.convs):
        assert (a.name, a.cin, a.cout, a.k, a.groups, a.has_bn) == (b.name, b.cin, b.cout, b.k, b.groups, b.has_bn)
        np.testing.assert_array_equal(fused[a.name][0], want_fused[b.name][0])
        np.testing.assert_array_equal(fused[a.name][1], want_fused[b.name][1])
    assert any(not c.has_bn and c.act == 0 for c in prog.convs) and any(c.has_bn and c.act == 0 for c in prog.convs)
    assert weights.to_bytes(prog, fused, meta) == blob


def test_fused_rows_follow_the_permutation(y11n):
    """qkv rows [q heads | k heads | v heads] and C2PSA.cv1 rows [b | a] are the checkpoint's rows, moved"""
    from cvsd_amd import weights
    prog, sd = y11n
    fused = weights.fuse_state_dict(prog, sd)
    qkv = next(c for c in prog.convs if c.name.endswith("attn.qkv"))
    w, b = fused[qkv.name]
    raw = weights.fuse_conv_bn(sd[qkv.name + ".conv.weight"], *(sd[f"{qkv.name}.bn.{k}"] for k in ("weight", "bias", "running_mean", "running_var")))
    nh = qkv.cin // 64
    assert np.array_equal(w[:32], raw[0][:32]) and np.array_equal(w[32:64], raw[0][128:160])         # q of heads 0 and 1
    assert np.array_equal(w[nh * 32:nh * 32 + 32], raw[0][32:64])                                       # k of head 0
    assert np.array_equal(w[nh * 64:nh * 64 + 64], raw[0][64:128]) and np.array_equal(b[nh * 64:], raw[1][np.r_[64:128, 192:256]])


def _ops():
    from cvsd_amd import ops
    return ops


def test_memory_plan_accepts_a_v11_image(y11n):
    ops = _ops()
    from cvsd_amd import weights
    blob = weights.build_from_state_dict("yolo11n", y11n[1])
    off, size, arena, plain = ops.memory_plan(blob, 8, 640, 640)
    assert 0 < arena < plain


def _patched(blob, op_index, field, value):
    """the image with field `field` of op record `op_index` replaced (weights.py: header, buffer table, 16-int op records)"""
    b = bytearray(blob)
    nb = struct.unpack_from("<I", b, 8 + 8 + 28)[0]
    fixed = 8 + 8 + 28 + 16 + 8 + 8
    struct.pack_into("<i", b, fixed + 8 * nb + 64 * op_index + 4 * field, value)
    return bytes(b)


def test_loader_validates_the_new_ops(y11n):
    ops = _ops()
    from cvsd_amd import weights
    blob = weights.build_from_state_dict("yolo11n", y11n[1])
    prog = weights.from_bytes(blob)[0]
    ia = next(i for i, o in enumerate(prog.ops) if o.type == OP_ATTN)
    idw = next(i for i, o in enumerate(prog.ops) if o.type == OP_DWCONV)
    v1 = bytearray(blob)
    struct.pack_into("<I", v1, 8, 1)                                  # a version-1 reader must not see these ops
    bad = [bytes(v1), _patched(blob, ia, 1, 16), _patched(blob, ia, 14, 3), _patched(blob, idw, 14, 7), _patched(blob, idw, 2, 2)]
    for b in bad:
        with pytest.raises(Exception):
            ops.memory_plan(b, 1, 640, 640)


def _fabricate_names(tmp_path, name, full_sd=None):
    """a YOLO11-shaped pickle: every key of the program's state dict; tiny tensors except the stem (its width is the scale)"""
    from test_convert import _fabricate
    prog = build_program(*parse_model_name(name))
    if full_sd is None:
        sd = {}
        for c in prog.convs:
            if c.has_bn:
                for k in ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var"):
                    sd[f"{c.name}.{k}"] = np.zeros((1,), np.float32)
            else:
                sd[f"{c.name}.weight"] = np.zeros((1,), np.float32)
                sd[f"{c.name}.bias"] = np.zeros((1,), np.float32)
        sd["model.0.conv.weight"] = np.zeros((prog.convs[0].cout, 3, 3, 3), np.float32)
        sd["model.23.dfl.conv.weight"] = np.arange(16, dtype=np.float32).reshape(1, 16, 1, 1)
    else:
        sd = full_sd
    p = str(tmp_path / f"{name}.pt")
    _fabricate(p, sd, {0: "person"}, half=True)
    return p, sd


@pytest.mark.parametrize("name", ["yolo11n", "yolo11s", "yolo11m", "yolo11l", "yolo11x",
                                  "yolo11n-pose", "yolo11s-pose", "yolo11m-pose", "yolo11l-pose", "yolo11x-pose"])
def test_convert_infers_every_yolo11_name(tmp_path, name):
    from cvsd_amd import convert
    p, _ = _fabricate_names(tmp_path, name)
    sd, info = convert.read_checkpoint(p)
    assert convert.infer_model_name(sd, info) == name


def test_convert_refuses_segmentation_yolo11(tmp_path):
    from cvsd_amd import convert
    p, sd = _fabricate_names(tmp_path, "yolo11n")
    sd = dict(sd)
    sd["model.23.proto.cv1.conv.weight"] = np.zeros((1,), np.float32)
    p, _ = _fabricate_names(tmp_path, "yolo11n", full_sd=sd)
    got, info = convert.read_checkpoint(p)
    with pytest.raises(ValueError, match="segmentation"):
        convert.infer_model_name(got, info)


def test_convert_yolo11_checkpoint_end_to_end(tmp_path, y11n):
    from cvsd_amd import convert, weights
    p, _ = _fabricate_names(tmp_path, "yolo11n", full_sd=y11n[1])
    blob = convert.convert_pt(p)
    prog, fused, meta = weights.from_bytes(blob)
    assert prog.family == "v11" and prog.nc == 80 and meta["names"] == {"0": "person"}


@pytest.mark.parametrize("h,w", [(640, 640), (480, 640)])
def test_torch_restatement_agrees_with_the_float64_program(y11n, h, w):
    """the graph check: an independent fp32 torch YOLO11 and a float64 run of the product's program agree at the fp32 noise level"""
    import _yolo11_torch as T
    from tools import precision as P, synth
    prog, sd = y11n
    frames = synth.synthetic_frames(1, h, w, seed=5)
    ref = P.f64_head("yolo11n", sd, frames, 640)
    got = T.head("yolo11n", sd, frames, 640)
    assert got.shape == ref.shape
    e = P.group_errors(got, ref, prog.nc)
    assert e["box"]["mean"] < 5e-3 and e["box"]["max"] < 1.0 and e["score"]["max"] < 1e-2, e
    assert T.Yolo11Torch("yolo11n", sd).count_params() == prog.param_count()
