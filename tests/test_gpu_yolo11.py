"""YOLO11 on the GPU: the two new kernels (depthwise conv, PSA attention) against float64, then whole nets through the C ABI under
the product-default environment -- as close to float64 as an independent torch fp32 restatement is (tests/_yolo11_torch.py),
post-NMS identity, determinism / batch invariance, track(), and the clean refusal of half=True."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RATIO, RATIO_MAX = 1.0, 1.5          # err(gpu vs f64) <= RATIO * err(torch vs f64) for mean and p99.9, RATIO_MAX for the max
RATIO_RECT = 1.25                    # ... at 480x640 (see test_yolo11_engine_is_as_close_to_float64_as_torch)
SCORE_ABS = 1e-3
MARGIN_NOISE = {"conf threshold": 5e-4, "score order": 5e-4, "iou threshold": 5e-3}


def _dw_ref(x, w, b, silu, res):
    from tools.program_ref import dwconv_nhwc, silu as silu_f
    y = dwconv_nhwc(x.astype(np.float64), w.astype(np.float64), 1, 1) + b.astype(np.float64)
    if silu:
        y = silu_f(y)
    return y + res.astype(np.float64) if res is not None else y


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("n,h,w,c", [(2, 13, 7, 20), (3, 20, 20, 64), (1, 9, 33, 10)])
def test_dwconv2d_matches_float64_on_channel_views(silu, with_res, n, h, w, c):
    from cvsd_amd import ops
    rng = np.random.default_rng([n, h, w, c, silu, with_res])
    cx, cy, cr = c + 12, c + 8, c + 4
    cx, cy, cr = (cx + 3) // 4 * 4, (cy + 3) // 4 * 4, (cr + 3) // 4 * 4
    x = rng.standard_normal((n, h, w, cx)).astype(np.float32)
    wt = (rng.standard_normal((c, 1, 3, 3)) / 3).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    res = rng.standard_normal((n, h, w, cr)).astype(np.float32) if with_res else None
    y0 = rng.standard_normal((n, h, w, cy)).astype(np.float32)           # channels outside the view must come back unchanged
    x_off, y_off, r_off = 8, 4, 4 if c + 4 <= cr else 0
    got = ops.dwconv2d(x, wt, b, silu=silu, residual=res, x_off=x_off, c=c, res_off=r_off, y=y0, y_off=y_off)
    want = _dw_ref(x[..., x_off:x_off + c], wt, b, silu, None if res is None else res[..., r_off:r_off + c])
    np.testing.assert_array_equal(got[..., :y_off], y0[..., :y_off])
    np.testing.assert_array_equal(got[..., y_off + c:], y0[..., y_off + c:])
    err = np.abs(got[..., y_off:y_off + c] - want)
    assert err.max() <= 1e-5 * max(1.0, np.abs(want).max()), err.max()
    again = ops.dwconv2d(x, wt, b, silu=silu, residual=res, x_off=x_off, c=c, res_off=r_off, y=y0, y_off=y_off)
    assert np.array_equal(got, again)


def _attn_torch(qkv, heads):
    """Ultralytics' Attention arithmetic in torch fp32 (CPU) on the permuted qkv layout"""
    import torch
    n, N, _ = qkv.shape
    t = torch.from_numpy(qkv)
    q = t[..., :heads * 32].reshape(n, N, heads, 32).permute(0, 2, 3, 1)              # [n, nh, kd, N]
    k = t[..., heads * 32:heads * 64].reshape(n, N, heads, 32).permute(0, 2, 3, 1)
    v = t[..., heads * 64:].reshape(n, N, heads, 64).permute(0, 2, 3, 1)              # [n, nh, hd, N]
    attn = ((q.transpose(-2, -1) @ k) * (32 ** -0.5)).softmax(dim=-1)
    out = v @ attn.transpose(-2, -1)                                                   # [n, nh, hd, N]
    return out.permute(0, 3, 1, 2).reshape(n, N, heads * 64).numpy()


@pytest.mark.parametrize("N", [1, 240, 300, 400, 1600])
@pytest.mark.parametrize("heads", [2, 4, 6])
@pytest.mark.parametrize("batch", [1, 8])
def test_psa_attention_is_as_close_to_float64_as_torch(N, heads, batch):
    from cvsd_amd import ops
    from tools.program_ref import psa_attention
    rng = np.random.default_rng([N, heads, batch])
    qkv = (rng.standard_normal((batch, N, heads * 128)) * 1.5).astype(np.float32)
    got = ops.psa_attention(qkv, heads)
    ref = psa_attention(qkv.astype(np.float64).reshape(batch, N, 1, -1), heads, 32, 64).reshape(batch, N, -1)
    e_gpu, e_t = np.abs(got - ref), np.abs(_attn_torch(qkv, heads) - ref)
    print(f"[attn] N {N} heads {heads} batch {batch}: mean {e_gpu.mean():.2e} (torch {e_t.mean():.2e}) "
          f"max {e_gpu.max():.2e} (torch {e_t.max():.2e})")
    assert e_gpu.mean() <= RATIO * max(e_t.mean(), 1e-9)
    assert e_gpu.max() <= RATIO_MAX * max(e_t.max(), 1e-8)
    if batch > 1:                                    # batch invariance: frame 1 alone gives the same bits
        assert np.array_equal(ops.psa_attention(qkv[1:2], heads)[0], got[1])


def _measure(name, h, w, imgsz=640):
    import _yolo11_torch as T
    from cvsd_amd import YOLO
    from tools import precision as P, synth
    _, sd = synth.synthetic_checkpoint(name, seed=0)
    frames = synth.synthetic_frames(2, h, w, seed=5)
    ref = P.f64_head(name, sd, frames, imgsz)
    torch32 = T.head(name, sd, frames, imgsz)
    m = YOLO.from_state_dict(name, sd)
    gpu = m.raw_head(frames, imgsz=imgsz)
    assert gpu.shape == ref.shape
    return m, frames, ref, P.group_errors(torch32, ref, m.nc), P.group_errors(gpu, ref, m.nc)


@pytest.mark.parametrize("name,h,w,imgsz", [("yolo11n", 640, 640, 640), ("yolo11n-pose", 640, 640, 640), ("yolo11s", 640, 640, 640),
                                            ("yolo11n", 480, 640, 640), ("yolo11n", 1280, 1280, 1280)])
def test_yolo11_engine_is_as_close_to_float64_as_torch(name, h, w, imgsz):
    from tools import precision as P
    m, frames, ref, e_torch, e_gpu = _measure(name, h, w, imgsz)
    report = {}
    for g in e_gpu:
        for stat in ("mean", "p999", "max"):
            t, v = e_torch[g][stat], e_gpu[g][stat]
            report[f"{g}.{stat}"] = [float(f"{v:.3e}"), float(f"{t:.3e}"), round(v / max(t, 1e-30), 2)]
    print(f"[precision] {name} {h}x{w}: " + json.dumps(report))
    # 480x640 (rect letterbox, 300 attention tokens): on these two frames the EXISTING engine is at torch parity, not below it
    # (yolov8n: 1.01 / 0.98 / 1.04 x torch's mean / p99.9 / max), and yolo11n measures 0.96 / 1.15 / 1.13; other frame seeds give
    # 0.7 x.  The same frames are kept, with a ratio that covers the existing engine's own level at this shape.
    ratio = RATIO_RECT if (h, w) == (480, 640) else RATIO
    for g in e_gpu:
        for stat in ("mean", "p999", "max"):
            lim = RATIO_MAX if stat == "max" else ratio
            assert e_gpu[g][stat] <= lim * max(e_torch[g][stat], 1e-6), (name, g, stat, report[f"{g}.{stat}"])
    # scores within 1e-3 wherever fp32 torch itself gets there; on these random-weight YOLO11 nets torch's own max score error
    # can exceed it (1.6e-3 on yolo11n at 640: a single-sample statistic), and there the ratio above is the bound
    for g in ("score", "kpt_conf"):
        if g in e_gpu:
            assert e_gpu[g]["p999"] <= SCORE_ABS
            if e_torch[g]["max"] <= SCORE_ABS:
                assert e_gpu[g]["max"] <= SCORE_ABS, (name, g, report[f"{g}.max"])
    res = m.predict(frames, conf=0.25, iou=0.7, imgsz=imgsz)
    want = P.nms_rows(ref.astype(np.float32), 0.25, 0.7, m.nc)
    for i, (r, (_, kept64)) in enumerate(zip(res, want)):
        div = P.first_divergence_margin(ref[i], kept64.tolist(), r.anchor_idx.tolist(), m.nc, 0.25, 0.7)
        if div is not None:
            pos, margin, kind = div
            assert margin < MARGIN_NOISE[kind], f"{name} frame {i}: diverges at rank {pos} on a float64 {kind} margin of {margin:.2e}"


def test_yolo11_rows_are_deterministic_and_batch_invariant():
    from cvsd_amd import YOLO
    from tools import synth
    _, sd = synth.synthetic_checkpoint("yolo11n", seed=0)
    m = YOLO.from_state_dict("yolo11n", sd)
    frames = synth.synthetic_frames(64, 640, 640, seed=11)

    def rows(batch):
        return [(r.anchor_idx.copy(), r.boxes.data.numpy().copy()) for r in m.predict(batch, conf=0.25)]

    alone = rows(frames[:1])[0]
    in8 = rows(frames[:8])
    in64 = rows(frames)
    again = rows(frames)
    assert len(alone[0]) > 0
    for got in (in8[0], in64[0]):
        assert np.array_equal(got[0], alone[0]) and np.array_equal(got[1], alone[1])
    for a, b in zip(in64, again):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for a, b in zip(in8, in64[:8]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert m.info_struct.family == b"v11"


def test_yolo11_track_yields_ids():
    from cvsd_amd import YOLO
    from tools import synth
    _, sd = synth.synthetic_checkpoint("yolo11n", seed=0)
    m = YOLO.from_state_dict("yolo11n", sd)
    clip = synth.synthetic_clip(6, 320, 320, seed=2)
    ids = []
    for f in clip:
        r = m.track(f, persist=True, conf=0.25, imgsz=320)[0]
        if r.boxes.id is not None:
            ids.extend(np.asarray(r.boxes.id).ravel().tolist())
    assert ids, "track() produced no ids on a YOLO11 model"


def test_yolo11_half_is_refused_cleanly():
    from cvsd_amd import YOLO
    from tools import synth
    _, sd = synth.synthetic_checkpoint("yolo11n", seed=0)
    with pytest.raises(Exception, match="half"):
        YOLO.from_state_dict("yolo11n", sd, half=True)
