"""The fused Shopformer kernel on the GPU against the reference's outputs stored in tests/golden/shopformer_fixture*.npz (reads only
the repository).  Yardstick of the accuracy test: mean |gpu - float64 reference| <= 1.25 x mean |reference fp32 - float64| + 1e-6."""
import numpy as np
import pytest
import torch

import _shopformer_numpy as R
from _shopformer_sweep_cases import check_elements
from _shopformer_c_forms import old_c_forms_equal_forward

pytestmark = pytest.mark.gpu
CONFIGS = ["default", "kp18_t24", "h32_l4"]
KEYS = (("tokens", "tokens"), ("reconstructed_tokens", "recon"), ("normality_score", "score"))


@pytest.fixture(scope="module")
def fix():
    return R.load_fixture()


@pytest.fixture(scope="module")
def models(fix):
    from cvsd_amd import Shopformer
    out = {}
    for name in CONFIGS:
        cfg, sd, x = R.fixture_model(fix, name)
        out[name] = (Shopformer.from_state_dict(sd, cfg, device=0), x)
    return out


def _within(got, fix, name, tag=""):
    for key, ref in KEYS:
        f64, f32 = fix[f"{name}.{tag}{ref}_f64"], fix[f"{name}.{tag}{ref}_f32"]
        e_gpu, e_ref = float(np.abs(got[key] - f64).mean()), float(np.abs(f32 - f64).mean())
        print(f"{name} {tag}{key}: gpu mean err {e_gpu:.3e}, reference fp32 mean err {e_ref:.3e}, ratio {e_gpu / e_ref:.3f}")
        assert got[key].shape == f64.shape
        assert e_gpu <= 1.25 * e_ref + 1e-6, (key, e_gpu, e_ref)


def _every_element(got, fix, name, x, tag="", img64=None):
    """each output, element by element, against the float64 numpy evaluation of the SAME fp32 weight image (``img64``, computed here
    when not given), in units of the float32 numpy evaluation's own error (tests/_shopformer_sweep_cases.py)"""
    from cvsd_amd import shopformer as SF
    cfg, sd, _ = R.fixture_model(fix, name)
    image = SF.parse_image(SF.image_from_state_dict(sd, cfg))
    img64, img32 = R.forward(*image, x) if img64 is None else img64, R.forward(*image, x, dtype=np.float32)
    for key, _ in KEYS:
        r = check_elements(got[key], img64[key], img32[key], key, f"{name} {tag}")
        print(f"{name} {tag}{key}: max |gpu - f64(image)| {r['err_max']:.3e} = {r['ratio_max']:.3f} x numpy fp32's, mean {r['ratio_mean']:.3f} x")


@pytest.mark.parametrize("name", CONFIGS)
def test_outputs_within_the_references_own_fp32_error(fix, models, name):
    model, x = models[name]
    got = model.forward(x)
    # the part of the error that is summation order alone (asserted per element by _every_element) = distance to a float64 evaluation of the SAME fp32
    # weight image (the rest of the distance to the reference is the second rounding of the folded weights)
    from cvsd_amd import shopformer as SF
    cfg, sd, _ = R.fixture_model(fix, name)
    img64 = R.forward(*SF.parse_image(SF.image_from_state_dict(sd, cfg)), x)
    for key, ref in KEYS:
        print(f"{name} {key}: mean |gpu - f64(image)| {np.abs(got[key] - img64[key]).mean():.3e}, "
              f"mean |f64(image) - f64 reference| {np.abs(img64[key] - fix[f'{name}.{ref}_f64']).mean():.3e}")
    _every_element(got, fix, name, x, img64=img64)
    _within(got, fix, name)


@pytest.mark.parametrize("name", CONFIGS)
def test_scores_do_not_depend_on_batch_or_position(fix, models, name):
    model, x = models[name]
    base = model.forward(x)
    assert model.score(x[:0]).shape == (0,)
    for i in (0, 1, 100, 255):
        alone = model.forward(x[i:i + 1])
        for key, _ in KEYS:
            assert np.array_equal(alone[key][0], base[key][i]), (key, i)
    for n in (1, 2, 3, 63, 64, 65, 4097):
        idx = np.arange(n) % len(x)
        got = model.forward(x[idx])
        for key, _ in KEYS:
            assert np.array_equal(got[key], base[key][idx]), (key, n)
    rng = np.random.default_rng(5)
    idx = rng.permutation(4096) % len(x)
    assert np.array_equal(model.score(x[idx]), base["normality_score"][idx])
    assert np.array_equal(model.score(x), base["normality_score"])                 # score-only call: same bits without the optional outputs


def test_launch_count_does_not_depend_on_the_batch(models):
    """the engine's own counter (incremented beside the kernel launch, read through mi355_shopformer_info): an N = 1 call and an
    N = 65,536 call enqueue the same number of kernels, at most 2; so does the device / async entry point"""
    model, x = models["default"]
    assert model.info.group >= 1 and model.info.lds_bytes <= 160 * 1024
    c0 = model.launches
    one = model.score(x[:1])
    c1 = model.launches
    big = model.score(x[np.arange(65536) % len(x)])
    c2 = model.launches
    model.forward(x[:65])
    c3 = model.launches
    print(f"kernel launches: N=1 {c1 - c0}, N=65536 {c2 - c1}, N=65 with tokens and reconstruction {c3 - c2}")
    assert 1 <= c1 - c0 <= 2 and c2 - c1 == c1 - c0 and c3 - c2 == c1 - c0
    assert np.array_equal(big, np.tile(model.score(x), 65536 // len(x))) and one[0] == big[0]
    dev = torch.device("cuda:0")
    xd, sc = torch.from_numpy(x).to(dev), torch.empty(len(x), device=dev)
    c4 = model.launches
    model.score_device_async(xd.data_ptr(), len(x), sc.data_ptr())
    torch.cuda.synchronize()
    assert model.launches - c4 == c1 - c0


def test_device_async_entry_point_equals_the_blocking_one(models):
    model, x = models["default"]
    want = model.forward(x)
    dev = torch.device("cuda:0")
    xd = torch.from_numpy(x).to(dev)
    sc = torch.empty(len(x), device=dev)
    tk = torch.empty((len(x), model.n_tokens, model.d_model), device=dev)
    rc = torch.empty_like(tk)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        model.score_device_async(xd.data_ptr(), len(x), sc.data_ptr(), stream=stream.cuda_stream, tokens_dev=tk.data_ptr(), recon_dev=rc.data_ptr())
    stream.synchronize()
    assert np.array_equal(sc.cpu().numpy(), want["normality_score"])
    assert np.array_equal(tk.cpu().numpy(), want["tokens"]) and np.array_equal(rc.cpu().numpy(), want["reconstructed_tokens"])
    old_c_forms_equal_forward(model, x, want, xd, stream)


def test_video_to_scores_end_to_end(fix, models, v8n_pose):
    """yolov8n-pose synthetic engine -> video_to_poselift (the clip of make_poselift_fixture.py) -> score_poselift == the reference's
    scores for those windows; StreamScorer over the same clip returns the identical floats"""
    import os
    from cvsd_amd import YOLO, StreamScorer, score_poselift, windows_from_poselift
    from cvsd_amd.poselift_bridge import video_to_poselift
    from tools import synth
    pf = np.load(os.path.join(os.path.dirname(__file__), "golden", "poselift_fixture.npz"))
    n_frames, h, w, seed_f, imgsz, batch = (int(v) for v in pf["meta"][:6])
    yolo = YOLO.from_state_dict("yolov8n-pose", v8n_pose[1], device=0)
    data = video_to_poselift(yolo, list(synth.synthetic_clip(n_frames, h, w, seed=seed_f)), conf=float(pf["conf"]), batch=batch, imgsz=imgsz)
    model, _ = models["default"]
    scores, index = score_poselift(model, data)
    assert np.array_equal(scores, model.score(windows_from_poselift(data)[0]))
    _within(model.forward(windows_from_poselift(data)[0]), fix, "default", tag="poselift_")
    _every_element(model.forward(windows_from_poselift(data)[0]), fix, "default", windows_from_poselift(data)[0], tag="poselift_")
    st, live = StreamScorer(model), []
    for f in sorted(data):
        rows = np.asarray([[b[0], b[1], b[0] + b[2], b[1] + b[3], pid] for pid, (b, _) in data[f].items()], np.float32).reshape(-1, 5)
        live += st.update(f, rows, np.asarray([k for _, k in data[f].values()], np.float32).reshape(-1, 17, 3))
    assert sorted(live) == sorted((pid, a, b, float(s)) for (pid, a, b), s in zip(index, scores)) and len(live) > 0
