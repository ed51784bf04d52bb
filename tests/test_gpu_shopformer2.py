"""The shopformer_2 variant on the GPU (two launches: tokenizer, transformer over row groups of 16 windows) against the reference's
outputs stored in tests/golden/shopformer2_fixture*.npz (reads only the repository).  Yardstick of the accuracy test, the one
test_gpu_shopformer.py uses: mean |gpu - float64 reference| <= 1.25 x mean |reference fp32 - float64| + 1e-6."""
import os

import numpy as np
import pytest
import torch

import _shopformer2_numpy as R2
from _shopformer_sweep_cases import check_elements
from _shopformer_c_forms import old_c_forms_equal_forward

pytestmark = pytest.mark.gpu
CONFIGS = ["paper", "default24", "paper_t24"]
KEYS = (("tokens", "tokens"), ("reconstructed_tokens", "recon"), ("normality_score", "score"), ("token_scores", "token_scores"))


@pytest.fixture(scope="module")
def fix():
    return R2.load_fixture()


@pytest.fixture(scope="module")
def models(fix):
    from cvsd_amd import Shopformer
    out = {}
    for name in CONFIGS:
        cfg, sd, x = R2.fixture_model(fix, name)
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
    cfg, sd, _ = R2.fixture_model(fix, name)
    image = SF.parse_image(SF.image_from_state_dict(sd, cfg))
    img64, img32 = R2.forward(*image, x) if img64 is None else img64, R2.forward(*image, x, dtype=np.float32)
    for key, _ in KEYS:
        r = check_elements(got[key], img64[key], img32[key], key, f"{name} {tag}")
        print(f"{name} {tag}{key}: max |gpu - f64(image)| {r['err_max']:.3e} = {r['ratio_max']:.3f} x numpy fp32's, mean {r['ratio_mean']:.3f} x")


@pytest.mark.parametrize("name", CONFIGS)
def test_outputs_within_the_references_own_fp32_error(fix, models, name):
    model, x = models[name]
    assert model.variant == 2 and model.info.variant == 2 and model.n_tokens == 2
    got = model.forward(x)
    # the split against a float64 evaluation of the SAME fp32 weight image (its gpu half is asserted per element by _every_element)
    from cvsd_amd import shopformer as SF
    cfg, sd, _ = R2.fixture_model(fix, name)
    img64 = R2.forward(*SF.parse_image(SF.image_from_state_dict(sd, cfg)), x)
    for key, ref in KEYS:
        print(f"{name} {key}: mean |gpu - f64(image)| {np.abs(got[key] - img64[key]).mean():.3e}, "
              f"mean |f64(image) - f64 reference| {np.abs(img64[key] - fix[f'{name}.{ref}_f64']).mean():.3e}")
    _every_element(got, fix, name, x, img64=img64)
    _within(got, fix, name)


@pytest.mark.parametrize("name", CONFIGS)
def test_scores_do_not_depend_on_batch_or_position(fix, models, name):
    model, x = models[name]
    gt = int(model.info.group_transformer)
    print(f"{name}: tokenizer group {model.info.group}, transformer row group {gt} windows")
    base = model.forward(x)
    assert model.score(x[:0]).shape == (0,) and model.score(x[:0], reduction="none").shape == (0, 2)
    for i in (0, 1, 15, 16, 17, 100, 255):                                   # either side of the transformer's row-group boundary
        alone = model.forward(x[i:i + 1])
        for key, _ in KEYS:
            assert np.array_equal(alone[key][0], base[key][i]), (key, i)
    for n in (1, 2, 3, 15, 16, 17, 4097):
        idx = (np.arange(n) + 5) % len(x)                                        # shifted: windows change their slot in both groups
        got = model.forward(x[idx])
        for key, _ in KEYS:
            assert np.array_equal(got[key], base[key][idx]), (key, n)
    rng = np.random.default_rng(5)
    idx = rng.permutation(4096) % len(x)
    assert np.array_equal(model.score(x[idx]), base["normality_score"][idx])
    assert np.array_equal(model.score(x), base["normality_score"])                 # score-only call: same bits without the optional outputs
    assert np.array_equal(model.score(x, reduction="none"), base["token_scores"])
    assert np.array_equal(model.score(x[idx], reduction="none"), base["token_scores"][idx])


def test_launch_count_does_not_depend_on_the_batch(models):
    model, x = models["default24"]
    assert model.info.group >= 1 and model.info.lds_bytes <= 160 * 1024
    c0 = model.launches
    one = model.score(x[:1])
    c1 = model.launches
    big = model.score(x[np.arange(65536) % len(x)])
    c2 = model.launches
    model.forward(x[:65])
    c3 = model.launches
    print(f"kernel launches: N=1 {c1 - c0}, N=65536 {c2 - c1}, N=65 with every output {c3 - c2}")
    assert 1 <= c1 - c0 <= 2 and c2 - c1 == c1 - c0 and c3 - c2 == c1 - c0
    assert np.array_equal(big, np.tile(model.score(x), 65536 // len(x))) and one[0] == big[0]
    dev = torch.device("cuda:0")
    xd, sc = torch.from_numpy(x).to(dev), torch.empty(len(x), device=dev)
    c4 = model.launches
    model.score_device_async(xd.data_ptr(), len(x), sc.data_ptr())
    torch.cuda.synchronize()
    assert model.launches - c4 == c1 - c0


@pytest.mark.parametrize("name", CONFIGS)
def test_device_async_entry_point_equals_the_blocking_one(models, name):
    model, x = models[name]
    want = model.forward(x)
    dev = torch.device("cuda:0")
    xd = torch.from_numpy(x).to(dev)
    sc = torch.empty(len(x), device=dev)
    ts = torch.empty((len(x), 2), device=dev)
    tk = torch.empty((len(x), model.n_tokens, model.token_dim), device=dev)
    rc = torch.empty_like(tk)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        model.score_device_async(xd.data_ptr(), len(x), sc.data_ptr(), stream=stream.cuda_stream, tokens_dev=tk.data_ptr(),
                                 recon_dev=rc.data_ptr(), token_scores_dev=ts.data_ptr())
    stream.synchronize()
    assert np.array_equal(sc.cpu().numpy(), want["normality_score"]) and np.array_equal(ts.cpu().numpy(), want["token_scores"])
    assert np.array_equal(tk.cpu().numpy(), want["tokens"]) and np.array_equal(rc.cpu().numpy(), want["reconstructed_tokens"])
    sc2 = torch.zeros(len(x), device=dev)
    model.score_device_async(xd.data_ptr(), len(x), sc2.data_ptr())              # scores alone: tokens stay in the handle's scratch
    torch.cuda.synchronize()
    assert np.array_equal(sc2.cpu().numpy(), want["normality_score"])
    old_c_forms_equal_forward(model, x, want, xd, stream)


def test_video_to_scores_end_to_end(fix, models, v8n_pose):
    """yolov8n-pose synthetic engine -> video_to_poselift (the clip of make_poselift_fixture.py) -> score_poselift with the paper
    model == the reference's scores for the stored s2 windows; StreamScorer over the same clip returns the identical floats"""
    from cvsd_amd import YOLO, StreamScorer, score_poselift, windows_from_poselift
    from cvsd_amd.poselift_bridge import video_to_poselift
    from tools import synth
    pf = np.load(os.path.join(os.path.dirname(__file__), "golden", "poselift_fixture.npz"))
    n_frames, h, w, seed_f, imgsz, batch = (int(v) for v in pf["meta"][:6])
    yolo = YOLO.from_state_dict("yolov8n-pose", v8n_pose[1], device=0)
    data = video_to_poselift(yolo, list(synth.synthetic_clip(n_frames, h, w, seed=seed_f)), conf=float(pf["conf"]), batch=batch, imgsz=imgsz)
    model, _ = models["paper"]
    assert model.neck
    scores, index = score_poselift(model, data)
    wins = windows_from_poselift(data, num_keypoints=18, neck=True)[0]
    assert wins.shape == pf["s2_test_xy_x"].shape
    assert np.array_equal(scores, model.score(wins))
    _within(model.forward(wins), fix, "paper", tag="poselift_")
    _every_element(model.forward(wins), fix, "paper", wins, tag="poselift_")
    st, live = StreamScorer(model), []
    for f in sorted(data):
        rows = np.asarray([[b[0], b[1], b[0] + b[2], b[1] + b[3], pid] for pid, (b, _) in data[f].items()], np.float32).reshape(-1, 5)
        live += st.update(f, rows, np.asarray([k for _, k in data[f].values()], np.float32).reshape(-1, 17, 3))
    assert sorted(live) == sorted((pid, a, b, float(s)) for (pid, a, b), s in zip(index, scores)) and len(live) > 0


def test_the_older_variant_has_no_per_token_scores():
    import _shopformer_numpy as R
    from cvsd_amd import Shopformer
    fix1 = R.load_fixture()
    cfg, sd, x = R.fixture_model(fix1, "default")
    model = Shopformer.from_state_dict(sd, cfg, device=0)
    assert model.variant == 1 and model.info.variant == 1 and not model.neck
    with pytest.raises(ValueError, match="shopformer_2"):
        model.score(x[:4], reduction="none")
    assert "token_scores" not in model.forward(x[:4])
