"""The GCAE decoder launch on the GPU against the reference's poses stored in
tests/golden/shopformer_decoder_fixture*.npz (reads only the repository).  Yardstick of the accuracy tests, the one
test_gpu_shopformer.py uses: mean |gpu - float64 reference| <= 1.25 x mean |reference fp32 - float64| + 1e-6."""
import ctypes as C

import numpy as np
import pytest
import torch

import _shopformer_decoder_numpy as RD
from _shopformer_sweep_cases import check_elements

pytestmark = pytest.mark.gpu
CONFIGS = ["default", "kp18_t24", "h32_l4", "paper", "default24"]
POSE_KEYS = ("gcae_reconstructed", "reconstructed_poses", "pose_error")


@pytest.fixture(scope="module")
def fix():
    return RD.load_fixture()


@pytest.fixture(scope="module")
def models():
    """name -> (model with the decoder, config, state dict, the fixture's 64 windows, forward(x, poses=True) of them: computed once)"""
    from cvsd_amd import Shopformer
    out = {}
    for name in CONFIGS:
        cfg, sd, x = RD.fixture_model(name)
        m = Shopformer.from_state_dict(sd, cfg, device=0, decoder=True)
        out[name] = (m, cfg, sd, x, m.forward(x, poses=True))
    return out


@pytest.mark.parametrize("name", CONFIGS)
def test_decoder_within_the_references_own_fp32_error(fix, models, name):
    from cvsd_amd import shopformer as SF
    model, cfg, sd, x, _ = models[name]
    assert model.has_decoder and model.decoder_info.frames == int(fix[f"{name}.frames"])
    got = model.decode(fix[f"{name}.tokens_f32"])
    f64, f32 = fix[f"{name}.poses_f64"], fix[f"{name}.poses_f32"]
    # summation order alone, asserted per element below (distance to a float64 evaluation of the SAME fp32 image on the same fp32 tokens)
    # and what is left of the distance to the reference (the fp32 rounding of the folded weights and of the fp32 tokens)
    image = SF.parse_image(SF.image_from_state_dict(sd, cfg, decoder=True))
    img64 = RD.decode(*image, fix[f"{name}.tokens_f32"])
    e_gpu, e_ref = float(np.abs(got - f64).mean()), float(np.abs(f32 - f64).mean())
    print(f"{name} poses: gpu mean err {e_gpu:.3e}, reference fp32 mean err {e_ref:.3e}, ratio {e_gpu / e_ref:.3f}; "
          f"mean |gpu - f64(image)| {np.abs(got - img64).mean():.3e}, mean |f64(image) - f64 reference| {np.abs(img64 - f64).mean():.3e}")
    assert got.shape == f64.shape and got.dtype == np.float32
    # every element, in units of the float32 numpy evaluation's own error (tests/_shopformer_sweep_cases.py)
    r = check_elements(got, img64, RD.decode(*image, fix[f"{name}.tokens_f32"], dtype=np.float32), "gcae_reconstructed", name)
    print(f"{name} poses: max |gpu - f64(image)| {r['err_max']:.3e} = {r['ratio_max']:.3f} x numpy fp32's, mean {r['ratio_mean']:.3f} x")
    assert e_gpu <= 1.25 * e_ref + 1e-6, (e_gpu, e_ref)


@pytest.mark.parametrize("name", CONFIGS)
def test_forward_with_poses_equals_its_parts_bit_for_bit(models, name):
    from cvsd_amd import Shopformer
    model, cfg, sd, x, full = models[name]
    plain = model.forward(x)
    assert set(full) == set(plain) | set(POSE_KEYS)
    for k in plain:
        assert np.array_equal(full[k], plain[k]), k
    assert np.array_equal(full["gcae_reconstructed"], model.decode(plain["tokens"]))
    assert full["reconstructed_poses"] is full["gcae_reconstructed"] or np.array_equal(full["reconstructed_poses"], full["gcae_reconstructed"])
    assert full["gcae_reconstructed"].shape == x.shape and full["pose_error"].shape == (len(x),) + x.shape[2:]
    lean = model.forward(x, outputs=False, poses=True)                            # without the optional token outputs: the same bits
    assert set(lean) == {"normality_score", *POSE_KEYS} and all(np.array_equal(lean[k], full[k]) for k in lean)
    score_only = Shopformer.from_state_dict(sd, cfg, device=0)                    # the same checkpoint, version-1 / version-2 image
    assert not score_only.has_decoder
    assert np.array_equal(model.score(x), score_only.score(x))


@pytest.mark.parametrize("name", CONFIGS)
def test_pose_error_is_the_squared_distance_to_the_window(fix, models, name):
    model, _, _, x, full = models[name]
    assert np.array_equal(full["pose_error"], RD.pose_error_f32(full["gcae_reconstructed"], x))
    # its overall mean is the reference's stage-1 loss F.mse_loss(reconstruction, windows)
    got = float(full["pose_error"].astype(np.float64).mean())
    m64, m32 = float(fix[f"{name}.mse_f64"]), float(fix[f"{name}.mse_f32"])
    print(f"{name} mse: gpu {got:.9f}, reference f64 {m64:.9f}, |gpu - f64| {abs(got - m64):.3e}, reference |fp32 - f64| {abs(m32 - m64):.3e}")
    assert abs(got - m64) <= 1.25 * abs(m32 - m64) + 1e-6


@pytest.mark.parametrize("name", CONFIGS)
def test_poses_do_not_depend_on_batch_or_position(models, name):
    model, _, _, x, full = models[name]
    g = model.decoder_info.group
    assert 1 <= g <= 16 and model.decoder_info.lds_bytes <= 160 * 1024
    tokens = full["tokens"]
    base = model.decode(tokens)
    assert np.array_equal(base, full["gcae_reconstructed"])
    assert model.decode(tokens[:0]).shape == (0,) + x.shape[1:] and model.forward(x[:0], poses=True)["pose_error"].shape == (0,) + x.shape[2:]
    for i in sorted({0, 1, g - 1, g, g + 1, 2 * g - 1, 2 * g, 63}):              # either side of the row-group boundaries
        assert np.array_equal(model.decode(tokens[i:i + 1])[0], base[i]), i
        alone = model.forward(x[i:i + 1], poses=True)
        assert all(np.array_equal(alone[k][0], full[k][i]) for k in POSE_KEYS), i
    for n in sorted({1, 2, 3, 15, 16, 17, g - 1, g, g + 1, 4097} - {0}):
        idx = (np.arange(n) + 3) % len(x)                                         # shifted: every window at another slot of its group
        assert np.array_equal(model.decode(tokens[idx]), base[idx]), n
        got = model.forward(x[idx], poses=True)
        assert all(np.array_equal(got[k], full[k][idx]) for k in full), n
    idx = np.random.default_rng(5).permutation(len(x))
    assert np.array_equal(model.decode(tokens[idx]), base[idx])
    got = model.forward(x[idx], poses=True)
    assert all(np.array_equal(got[k], full[k][idx]) for k in full)


def test_interpolation_edges_follow_the_clamped_formula(models):
    """first and last output frame of a shopformer_2 config, where a wrong clamp of the source index shows: frame 0 has src < 0
    clamped to 0 (weight 0 on frame 1), the last frame has i1 clamped onto i0"""
    from cvsd_amd import shopformer as SF
    model, cfg, sd, x, full = models["paper"]
    geo, t = SF.parse_image(SF.image_from_state_dict(sd, cfg, decoder=True))
    assert geo["interp"] == 1 and (geo["Tdec"], geo["T"]) == (8, 12)
    i0, i1, w = RD.interp_table(8, 12)
    assert (i0[0], i1[0], float(w[0])) == (0, 1, 0.0) and (i0[-1], i1[-1]) == (7, 7) and 0 < float(w[-1]) < 1
    want = RD.decode(geo, t, full["tokens"])
    got = full["gcae_reconstructed"]
    # the model sums in float64, the kernel in float32: five chained products of K <= 144 terms each, unit roundoff u = 2^-24, on
    # values up to max |want|: K * u * max |want| bounds the float32 chains' distance to the model (a wrong clamp moves a frame by
    # the distance between neighbouring frames, four orders of magnitude more)
    tol = 144 * 2.0 ** -24 * max(1.0, float(np.abs(want).max()))
    for fr in (0, -1):
        err = float(np.abs(got[:, :, fr] - want[:, :, fr]).max())
        print(f"frame {fr}: max |gpu - numpy model| {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol
    # both clamps leave one source frame: output frame 0 is the layers' frame 0, the last output frame the layers' frame 7
    lay = RD.layers(geo, t, full["tokens"])
    assert np.abs(got[:, :, 0] - lay[:, :, 0]).max() <= tol and np.abs(got[:, :, -1] - lay[:, :, 7]).max() <= tol
    assert np.abs(lay[:, :, 0] - lay[:, :, 1]).mean() > 1000 * tol / 144 and np.abs(lay[:, :, 7] - lay[:, :, 6]).mean() > 1000 * tol / 144


@pytest.mark.parametrize("name", ["default", "paper"])
def test_launch_counts(models, name):
    from cvsd_amd import Shopformer
    model, cfg, sd, x, full = models[name]
    score_path = 2 if model.variant == 2 else 1

    def count(f):
        c = model.launches
        f()
        return model.launches - c

    big = x[np.arange(4097) % len(x)]
    assert count(lambda: model.decode(full["tokens"][:1])) == 1 and count(lambda: model.decode(full["tokens"][np.arange(4097) % len(x)])) == 1
    assert count(lambda: model.score(x[:1])) == score_path and count(lambda: model.score(big)) == score_path
    assert count(lambda: model.forward(x[:1])) == score_path
    assert count(lambda: model.forward(x[:1], poses=True)) == score_path + 1
    assert count(lambda: model.forward(big, poses=True)) == score_path + 1
    assert count(lambda: model.forward(x[:1], outputs=False, poses=True)) == score_path + 1


@pytest.mark.parametrize("name", ["default", "paper"])
def test_device_async_forms_equal_the_blocking_ones(models, name):
    from cvsd_amd import _lib
    model, _, _, x, full = models[name]
    dev = torch.device("cuda:0")
    n = len(x)
    xd = torch.from_numpy(x).to(dev)
    sc = torch.empty(n, device=dev)
    pose, err = torch.empty(x.shape, device=dev), torch.empty((n,) + x.shape[2:], device=dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):                                              # without a tokens buffer: the handle's scratch
        model.score_device_async(xd.data_ptr(), n, sc.data_ptr(), stream=stream.cuda_stream, poses_dev=pose.data_ptr(), pose_error_dev=err.data_ptr())
    stream.synchronize()
    assert np.array_equal(sc.cpu().numpy(), full["normality_score"])
    assert np.array_equal(pose.cpu().numpy(), full["gcae_reconstructed"]) and np.array_equal(err.cpu().numpy(), full["pose_error"])
    tk, rc, pose2 = torch.empty(full["tokens"].shape, device=dev), torch.empty(full["tokens"].shape, device=dev), torch.zeros(x.shape, device=dev)
    with torch.cuda.stream(stream):
        model.score_device_async(xd.data_ptr(), n, sc.data_ptr(), stream=stream.cuda_stream, tokens_dev=tk.data_ptr(), recon_dev=rc.data_ptr(),
                                 poses_dev=pose2.data_ptr())
    stream.synchronize()
    assert np.array_equal(tk.cpu().numpy(), full["tokens"]) and np.array_equal(rc.cpu().numpy(), full["reconstructed_tokens"])
    assert np.array_equal(pose2.cpu().numpy(), full["gcae_reconstructed"])
    # the raw C call on device buffers
    pose3 = torch.zeros(x.shape, device=dev)
    with torch.cuda.stream(stream):
        rcode = _lib.lib().mi355_shopformer_decode_device_async(model._h, tk.data_ptr(), n, pose3.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert rcode == 0 and np.array_equal(pose3.cpu().numpy(), full["gcae_reconstructed"])
    pose4 = torch.zeros(x.shape, device=dev)
    model.decode_device_async(rc.data_ptr(), n, pose4.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(pose4.cpu().numpy(), model.decode(full["reconstructed_tokens"]))


@pytest.mark.parametrize("name", ["default", "paper"])
def test_a_model_without_the_decoder_refuses(models, name):
    from cvsd_amd import Shopformer, _lib
    from cvsd_amd.shopformer import ShopformerDecoderInfo, ShopformerOutputs
    _, cfg, sd, x, full = models[name]
    model = Shopformer.from_state_dict(sd, cfg, device=0)
    dev = torch.device("cuda:0")
    xd, sc, pose = torch.from_numpy(x).to(dev), torch.empty(len(x), device=dev), torch.empty(x.shape, device=dev)
    c0 = model.launches
    with pytest.raises(ValueError, match="decoder"):
        model.decode(full["tokens"])
    with pytest.raises(ValueError, match="decoder"):
        model.forward(x, poses=True)
    with pytest.raises(ValueError, match="decoder"):
        model.score_device_async(xd.data_ptr(), len(x), sc.data_ptr(), poses_dev=pose.data_ptr())
    with pytest.raises(ValueError, match="decoder"):
        model.decode_device_async(xd.data_ptr(), len(x), pose.data_ptr())
    # the raw C calls: an error code and the message, no launch
    L = _lib.lib()
    tok = np.ascontiguousarray(full["tokens"])
    out = np.empty(x.shape, np.float32)
    calls = [lambda: L.mi355_shopformer_decode(model._h, tok.ctypes.data, len(x), out.ctypes.data),
             lambda: L.mi355_shopformer_decode_device_async(model._h, xd.data_ptr(), len(x), pose.data_ptr(), None),
             lambda: L.mi355_shopformer_decoder_info(model._h, C.byref(ShopformerDecoderInfo()))]
    o = ShopformerOutputs(C.sizeof(ShopformerOutputs), 0, sc.data_ptr(), None, None, None, pose.data_ptr(), None)
    calls.append(lambda: L.mi355_shopformer_score_ex_device_async(model._h, xd.data_ptr(), len(x), C.byref(o), None))
    score = np.empty(len(x), np.float32)
    oh = ShopformerOutputs(C.sizeof(ShopformerOutputs), 0, score.ctypes.data, None, None, None, out.ctypes.data, None)
    calls.append(lambda: L.mi355_shopformer_score_ex(model._h, x.ctypes.data, len(x), C.byref(oh)))
    for call in calls:
        assert call() == -1                                                       # MI355_EINVAL
        assert "built without the decoder" in L.mi355_last_error().decode()
    torch.cuda.synchronize()
    assert model.launches == c0
    # a caller compiled against the struct before it grew (its size stops after `recon`) gets the earlier behaviour, on either image
    old = ShopformerOutputs(ShopformerOutputs.poses.offset, 0, score.ctypes.data, None, None, None, 0xdead, 0xdead)
    for m in (model, models[name][0]):
        score[:] = -1
        assert L.mi355_shopformer_score_ex(m._h, x.ctypes.data, len(x), C.byref(old)) == 0
        assert np.array_equal(score, full["normality_score"])
