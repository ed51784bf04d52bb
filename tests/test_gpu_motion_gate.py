"""The motion gate on the GPU (csrc/motion_kernels.hip) against the numpy statement of tests/_motion_numpy.py, exactly; the forms a frame
may arrive in against each other; and ``YOLO.track_cameras(..., motion_gate=...)`` against the composition a user writes without it --
a MotionGate of their own on the host frames, ``model.predict`` on the moving frames, one ``BYTETracker(gmc_device=0)`` per camera fed
fresh or cached rows: bit for bit."""
import numpy as np
import pytest
import torch

import _motion_cases as K
import _motion_numpy as M
import test_gpu_track_cameras as T
from cvsd_amd import MotionGate, YUVFrame, ops

pytestmark = pytest.mark.gpu


def _gate(n, **kw):
    return MotionGate(n, device=0, **kw)


def _sums(frames, block):
    return ops.motion_grid(frames, block, device=0)


@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("block", K.BLOCKS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scripted_sequence_matches_numpy(shape, block, layout):
    kw, ticks = K.scripted(shape[0], shape[1], block, layout)
    K.check_scripted(K.run(_gate, _sums, kw, ticks))


def test_many_cameras_of_many_sizes_in_one_launch():
    """64 cameras, sizes from 1x1 to 130x270 (more than one strip, more than 16 and more than 64 groups per row), some absent"""
    rng = np.random.default_rng(1)
    sizes = [(1 + (7 * i) % 130, 1 + (37 * i) % 270) for i in range(64)]
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    ticks = []
    for t in range(4):
        cur = [None if (i + t) % 9 == 0 else (f if t < 2 else np.roll(f, 3, axis=1)) for i, f in enumerate(frames)]
        ticks.append(cur)
    out = K.run(_gate, _sums, dict(block=16, level=2.0, min_blocks=1, max_skip=30), ticks)
    assert any(not m and c == 0 for m, c in zip(out[1][0], out[1][1])) and out[2][0].sum() > 32


def _yuv(y, fmt, device=None, pitched=False):
    h, w = y.shape
    rng = np.random.default_rng(7)
    planes = {"uv": rng.integers(0, 256, (h // 2, w), dtype=np.uint8)} if fmt == "nv12" else \
             {"u": rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8), "v": rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)}
    yp = K.lay(y, "pitched") if pitched else y
    if device is not None:
        dev = torch.device("cuda", device)
        if pitched:
            parent = torch.zeros((h, w + 48), dtype=torch.uint8, device=dev)
            parent[:, 5:5 + w] = torch.from_numpy(np.ascontiguousarray(y)).to(dev)
            yp = parent[:, 5:5 + w]                                  # a decoder surface: pitched, and here starting at an odd byte
        else:
            yp = torch.from_numpy(np.ascontiguousarray(y)).to(dev)
        planes = {k: torch.from_numpy(v).to(dev) for k, v in planes.items()}
    return YUVFrame(yp, fmt=fmt, **planes)


@pytest.mark.parametrize("shape", [(98, 130, 16), (240, 320, 8), (50, 64, 32)], ids=lambda s: f"{s[0]}x{s[1]}-{s[2]}")
def test_input_forms_agree(shape):
    """one clip in every form a frame may arrive in: the same moving / changed / masks / sums as the numpy statement, hence as each other"""
    h, w, block = shape
    clip = [K.scene(h, w, block, 11 + k // 2) for k in range(6)]
    clip = [clip[0], clip[0], clip[2], clip[2], K.bump(clip[2], block, 3 * min(block, h) * min(block, w)), clip[4]]     # 3 > level 2
    dev = torch.device("cuda", 0)

    def cuda_view(f):
        parent = torch.zeros((h, w + 7, 3), dtype=torch.uint8, device=dev)
        parent[:, 5:5 + w] = torch.from_numpy(f).to(dev)
        return parent[:, 5:5 + w]
    forms = {
        "host": lambda f: f, "pitched": lambda f: K.lay(f, "pitched"), "odd": lambda f: K.lay(f, "odd"),
        "cuda": lambda f: torch.from_numpy(f).to(dev), "cuda_view": cuda_view,
    }
    kw = dict(block=block, level=2.0, min_blocks=1, max_skip=30)
    outs = {name: K.run(_gate, _sums, kw, [[fn(f)] for f in clip]) for name, fn in forms.items()}
    lum = [M.luma(f).astype(np.uint8) for f in clip]
    for fmt in ("nv12", "i420"):
        for where in (None, 0):
            for pitched in (False, True):
                outs[f"{fmt}-{where}-{pitched}"] = K.run(_gate, _sums, kw, [[_yuv(y, fmt, where, pitched)] for y in lum])
    flat = {k: [(bool(m[0]), int(c[0])) for m, c in v] for k, v in outs.items()}
    assert len({tuple(v) for v in flat.values()}) == 1, flat         # BGR luma == the Y planes made from it: every form tells one story
    assert [m for m, _ in flat["host"]] == [True, False, True, False, True, True]
    g = _gate(2)
    with pytest.raises(ValueError, match="all host memory or all CUDA"):
        g.update([clip[0], torch.from_numpy(clip[0]).to(dev)])
    assert g.mask(0).shape == (0, 0)


# ------------------------------------------------------------------------------------------------------------ track_cameras
def _ticks(sizes, n=12):
    """n ticks of four cameras; camera 2 is absent on three of them.  The absences are placed so that every list the detector sees -- gated,
    ungated or in the composition -- is all four cameras or cameras 0, 1, 3, the lists test_gpu_track_cameras.py runs as well: the first pass
    over a new list of shapes costs seconds, whichever test makes it."""
    clips = T._clips(n, sizes)
    out = []
    for t in range(n):
        frames = [c[t] for c in clips]
        if t in (4, 5, 9):                                            # a whole pair of the pairwise-repeating clip, and a repeat alone
            frames[2] = None
        out.append(frames)
    return out


def _composition_tick(model, gate, cache, trackers, frames, reid):
    """what a user writes without motion_gate=: their own gate on the host frames, predict on the moving frames, one tracker per camera"""
    moving, changed = gate.update(frames)
    present = [i for i, f in enumerate(frames) if f is not None]
    run = [i for i in present if moving[i]]
    if run:
        for r, i in zip(model.predict([frames[i] for i in run], conf=0.1, **({"feats": True} if reid else {})), run):
            cache[i] = r
    out = [None] * len(frames)
    for i in present:
        r = cache[i]
        tracks = trackers[i].update(r.boxes.data.numpy(), frames[i], **({"feats": r.feats} if reid else {}))
        if len(tracks):
            r = r[tracks[:, -1].astype(int)]
            r.update(boxes=torch.as_tensor(tracks[:, :-1], dtype=torch.float32))
        out[i] = r
    return out, moving, changed, run


_MODELS = {}


def _models(name):
    """three model objects per checkpoint, shared by the layouts: a call with persist=False starts their cameras (and gate) afresh"""
    if name not in _MODELS:
        _MODELS[name] = (T._model(name), T._model(name), T._model(name))
    return _MODELS[name]


@pytest.mark.parametrize("layout", ["mixed", "equal"])
@pytest.mark.parametrize("name", ["yolov8n", "yolov8n-pose"])
def test_gated_track_cameras(name, layout, monkeypatch):
    from cvsd_amd.tracker import BYTETracker
    reid = name == "yolov8n" and layout == "mixed"                  # one case runs the appearance matching
    tk = {"tracker": {"with_reid": True}} if reid else {}
    ticks = _ticks(T.MIXED if layout == "mixed" else T.EQUAL)
    plain, always, gated = _models(name)
    calls = []
    real = gated._predict_batch
    monkeypatch.setattr(gated, "_predict_batch", lambda batch, *a, **k: (calls.append(int(batch.shape[0])), real(batch, *a, **k))[1])
    gate, cache = MotionGate(4, device=None), [None] * 4
    trackers = [BYTETracker(gmc_device=0, **({"with_reid": True} if reid else {})) for _ in range(4)]
    ids, skipped_ticks = [], 0
    for t, frames in enumerate(ticks):
        want = plain.track_cameras(frames, persist=t > 0, **tk)
        # min_blocks = 0: every present camera moves -- the ungated call bit for bit
        got = always.track_cameras(frames, persist=t > 0, motion_gate={"min_blocks": 0}, **tk)
        ids += T._same_results(got, want)
        assert all(g.motion == {"moving": True, "changed": g.motion["changed"], "skipped": False} for g in got if g is not None)
        assert all(w.motion is None for w in want if w is not None)
        # the default gate: the composition
        n_calls = len(calls)
        got = gated.track_cameras(frames, persist=t > 0, motion_gate=True, **tk)
        want, moving, changed, run = _composition_tick(plain, gate, cache, trackers, frames, reid)
        ids += T._same_results(got, want)
        assert calls[n_calls:] == ([len(run)] if run else [])         # one detector call over the moving cameras, none when all are static
        skipped_ticks += not run and any(f is not None for f in frames)
        for i, (g, f) in enumerate(zip(got, frames)):
            if g is not None:
                assert g.motion == {"moving": bool(moving[i]), "changed": int(changed[i]), "skipped": not moving[i]}
                assert g.orig_img is f                                # a static camera's result carries this tick's frame
    assert skipped_ticks >= 3 and ids                                # the clips repeat pairwise: ticks without any detector pass did occur
    assert min(ids) == 1


def test_ungated_call_after_gated_ones_is_a_fresh_models(monkeypatch):
    ticks = _ticks(T.MIXED, 8)
    a, b = T._model("yolov8n-pose"), T._model("yolov8n-pose")
    for frames in ticks[:4]:
        a.track_cameras(frames, persist=True, motion_gate=True)
    ids = []
    for t, frames in enumerate(ticks[4:]):
        ids += T._same_results(a.track_cameras(frames, persist=t > 0), b.track_cameras(frames, persist=t > 0))
    assert ids
    # ... and persist=False restarts the gate with the trackers: the first tick moves again although the frame repeats
    r = a.track_cameras(ticks[7], persist=True, motion_gate=True)
    r = a.track_cameras(ticks[7], persist=True, motion_gate=True)
    assert all(not x.motion["moving"] and x.motion["skipped"] for x in r if x is not None)
    r = a.track_cameras(ticks[7], persist=False, motion_gate=True)
    assert all(x.motion["moving"] and not x.motion["skipped"] for x in r if x is not None)
    with pytest.raises(ValueError, match="blok"):
        a.track_cameras(ticks[7], persist=True, motion_gate={"blok": 8})
    with pytest.raises(ValueError, match="3 cameras"):
        a.track_cameras(ticks[7], persist=True, motion_gate=MotionGate(3, device=None))
    # a gate of the caller's, on the host: the same decisions
    mine = MotionGate(4, device=None)
    r1 = a.track_cameras(ticks[2], persist=False, motion_gate=mine)
    r2 = a.track_cameras(ticks[3], persist=True, motion_gate=mine)
    assert all(x.motion["moving"] for x in r1 if x is not None) and all(x.motion["skipped"] for x in r2 if x is not None)


def test_rows_do_not_depend_on_sharing_the_uploaded_frames(monkeypatch):
    ticks = _ticks(T.MIXED, 10)
    outs = []
    for share in ("1", "0"):
        monkeypatch.setenv("MI355_TRACK_SHARED_FRAME", share)
        model = T._model("yolov8n")
        outs.append([model.track_cameras(frames, persist=True, motion_gate=True) for frames in ticks])
    ids = []
    for got, want in zip(*outs):
        ids += T._same_results(got, want)
        assert [g.motion for g in got if g is not None] == [w.motion for w in want if w is not None]
    assert ids and any(g.motion["skipped"] for got in outs[0] for g in got if g is not None)
