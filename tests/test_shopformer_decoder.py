"""The GCAE decoder without a GPU: the loader (decoder=False images untouched, the version-3 fold / pack / round trip, the factor
rule, refusals in Python and in the C loader) and the folded decoder in float64 numpy against the REFERENCE'S OWN float64 poses
stored in tests/golden/shopformer_decoder_fixture*.npz (tests/golden/make_shopformer_decoder_fixture.py).

Figures measured when the fixture was made, mean |numpy f64 of the fp32 image - reference f64| against the reference's own
mean |fp32 - f64|: default 7.4e-08 / 6.5e-07, kp18_t24 5.1e-08 / 5.0e-07, h32_l4 3.0e-08 / 2.8e-07, paper 1.3e-07 / 3.7e-07,
default24 2.2e-07 / 3.7e-07 (the image's error is the one fp32 rounding of the folded weights and, for the two shopformer_2 configs,
the float32 source index and weight of the interpolation).  The unrounded float64 fold: 1e-15 of full scale without interpolation,
2.8e-07 / 5.1e-07 with it."""
import ctypes as C
import hashlib
import struct

import numpy as np
import pytest

import _shopformer_decoder_numpy as RD
from cvsd_amd import shopformer as SF

CONFIGS = ["default", "kp18_t24", "h32_l4", "paper", "default24"]
# SHA-256 of the version-1 images of the three shopformer/ fixture checkpoints: the values tests/test_shopformer2.py pins
V1_SHA256 = {"default": "31033be276f33a4addfe72e73314eef542a9ad3560ee68fcf3f1e3113e39197b",
             "kp18_t24": "853b47a35bc2f4cdbf6c6d02a35276349f590efc2b0eebdcc517c110a96c343c",
             "h32_l4": "c08d25628f106d06c08755bbfa171da38ebe594dd9e8991813b4e8c6eeb4ddf9"}
# package, T, V, tokens, factors, frames out of the layers, interpolation: the table of the decoder's geometry
TABLE = {"default": (12, 17, 3, [2, 2, 1, 1], 12, 0), "kp18_t24": (24, 18, 3, [2, 2, 2, 1], 24, 0),
         "paper": (12, 18, 2, [2, 2, 1, 1], 8, 1), "default24": (24, 17, 2, [2, 2, 2, 1], 16, 1)}


@pytest.fixture(scope="module")
def fix():
    return RD.load_fixture()


@pytest.fixture(scope="module")
def models():
    return {name: RD.fixture_model(name) for name in CONFIGS}


@pytest.mark.parametrize("name", CONFIGS)
def test_without_decoder_the_image_is_unchanged_byte_for_byte(models, name):
    cfg, sd, _ = models[name]
    score_only = {k: v for k, v in sd.items() if not k.startswith("gcae.decoder.")}
    blob = SF.image_from_state_dict(sd, cfg, decoder=False)
    assert blob == SF.image_from_state_dict(sd, cfg) == SF.image_from_state_dict(score_only, cfg)
    ver = struct.unpack_from("<I", blob, 8)[0]
    assert ver == (2 if SF.is_variant_2(cfg) else 1)
    if name in V1_SHA256:
        assert hashlib.sha256(blob).hexdigest() == V1_SHA256[name]
    # and a version-3 image holds that image's tensors, bit for bit, plus the decoder's
    geo, t = SF.parse_image(blob)
    geo3, t3 = SF.parse_image(SF.image_from_state_dict(sd, cfg, decoder=True))
    assert set(t) < set(t3) and all(k.startswith("dec.") for k in set(t3) - set(t))
    assert all(np.array_equal(t[k], t3[k]) for k in t) and all(geo3[k] == v for k, v in geo.items())


@pytest.mark.parametrize("name", CONFIGS)
def test_version_3_image_round_trips_and_is_the_rounded_float64_fold(models, name):
    cfg, sd, _ = models[name]
    geo, t32 = SF.fold_state_dict(sd, cfg, decoder=True)
    blob = SF.build_image(geo, t32)
    assert struct.unpack_from("<II", blob, 8) == (3, len(SF.CFG_FIELDS_V3))
    geo2, back = SF.parse_image(blob)
    _, t64 = SF.fold_state_dict(sd, cfg, dtype=np.float64, decoder=True)
    assert geo2 == geo and set(back) == set(t32) == set(t64)
    assert SF.build_image(geo2, back) == blob
    for k in t32:
        np.testing.assert_array_equal(back[k].reshape(-1), t32[k].reshape(-1), err_msg=k)
        np.testing.assert_array_equal(t32[k], t64[k].astype(np.float32), err_msg=k)
    V, H, L = geo["V"], geo["H"], geo["L"]
    assert back["dec.ip.w"].shape == (V * H, 1, L * V) and back["dec.l3.w"].shape == (2, 1, H)
    # the BatchNorm statistics of the synthetic decoder are non-trivial: the fold changed the weights
    assert not np.allclose(back["dec.l0.w"][:, 0, :].T, np.asarray(sd["gcae.decoder.layers.0.weight"])[:, :, 0, 0], atol=1e-3)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_factor_table_and_interpolation_flag(fix, models, name):
    cfg, sd, _ = models[name]
    geo, _ = SF.fold_state_dict(sd, cfg, decoder=True)
    T, V, ntok, factors, frames, interp = TABLE[name]
    assert (geo["T"], geo["V"], geo["ntok"]) == (T, V, ntok)
    assert [geo[f"u{i}"] for i in range(4)] == factors == fix[f"{name}.factors"].tolist()
    assert geo["Tdec"] == frames == int(fix[f"{name}.frames"]) and geo["interp"] == interp
    assert SF.decoder_factors(2, T) == factors


def test_missing_or_misshaped_decoder_keys_are_refused_with_the_key_named(models):
    cfg, sd, _ = models["default"]
    with pytest.raises(ValueError, match="gcae.decoder.initial_proj.weight"):
        SF.image_from_state_dict({k: v for k, v in sd.items() if not k.startswith("gcae.decoder.")}, cfg, decoder=True)
    for key in ("gcae.decoder.layers.4.weight", "gcae.decoder.layers.5.running_var", "gcae.decoder.layers.12.bias"):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            SF.image_from_state_dict({k: v for k, v in sd.items() if k != key}, cfg, decoder=True)
    bad = dict(sd)
    bad["gcae.decoder.layers.8.weight"] = np.zeros((64, 64, 2, 1), np.float32)          # a transposed convolution where the config has a 1x1
    with pytest.raises(ValueError, match=r"gcae\.decoder\.layers\.8\.weight"):
        SF.image_from_state_dict(bad, cfg, decoder=True)
    cfg2, sd2, _ = models["paper"]
    bad = dict(sd2)
    bad["gcae.decoder.initial_proj.bias"] = np.zeros(17 * 64, np.float32)
    with pytest.raises(ValueError, match=r"gcae\.decoder\.initial_proj\.bias"):
        SF.image_from_state_dict(bad, cfg2, decoder=True)


def _create(blob):
    from cvsd_amd import _lib
    h = C.c_void_p()
    rc = _lib.lib().mi355_shopformer_create(blob, len(blob), 0, C.byref(h))
    msg = _lib.lib().mi355_last_error().decode(errors="replace")
    if h.value:
        _lib.lib().mi355_shopformer_destroy(h)
    return rc, msg


@pytest.mark.parametrize("name", ["default", "paper"])
def test_c_loader_refuses_bad_version_3_images_before_the_device(models, name):
    cfg, sd, _ = models[name]
    geo, t32 = SF.fold_state_dict(sd, cfg, decoder=True)
    for over, named in (({"u3": 2}, "decoder upsample factor"), ({"u0": 3}, "decoder upsample factor"), ({"Tdec": geo["Tdec"] + 1}, "decoder frame count"),
                        ({"interp": 1 - geo["interp"]}, "decoder interpolation flag"), ({"variant": 3}, "variant")):
        g = dict(geo)
        g.update(over)
        rc, msg = _create(SF.build_image(g, t32))
        assert rc == -3 and named in msg, (over, rc, msg)                        # MI355_EFORMAT, not a HIP error
    for gone in ("dec.ip.w", "dec.l2.b", "dec.l3.w"):
        rc, msg = _create(SF.build_image(geo, {k: v for k, v in t32.items() if k != gone}))
        assert rc == -3 and gone in msg, (gone, rc, msg)
    wrong = dict(t32)
    wrong["dec.l1.w"] = t32["dec.l1.w"][:, :1]                                   # one parity where the factor says two
    rc, msg = _create(SF.build_image(geo, wrong))
    assert rc == -3 and "dec.l1.w" in msg, (rc, msg)


@pytest.mark.parametrize("name", CONFIGS)
def test_folded_decoder_in_float64_meets_the_yardstick_against_the_reference(fix, models, name):
    cfg, sd, _ = models[name]
    geo, t32 = SF.parse_image(SF.image_from_state_dict(sd, cfg, decoder=True))
    got = RD.decode(geo, t32, fix[f"{name}.tokens_f64"])
    f64, f32 = fix[f"{name}.poses_f64"], fix[f"{name}.poses_f32"]
    e_np, e_ref = float(np.abs(got - f64).mean()), float(np.abs(f32 - f64).mean())
    print(f"{name}: mean |numpy f64(image) - f64| {e_np:.3e}, reference fp32 mean err {e_ref:.3e}, ratio {e_np / e_ref:.3f}")
    assert got.shape == f64.shape == (64, 2, geo["T"], geo["V"])
    assert e_np <= 1.25 * e_ref + 1e-6, (e_np, e_ref)
    # the unrounded float64 fold reproduces the reference to float64 noise where no interpolation follows; with it, to the float32
    # rounding of the source index and weight that the formula fixes
    _, t64 = SF.fold_state_dict(sd, cfg, dtype=np.float64, decoder=True)
    err = np.abs(RD.decode(geo, t64, fix[f"{name}.tokens_f64"]) - f64).max() / np.abs(f64).max()
    print(f"{name}: float64 fold, max error {err:.2e} of full scale")
    assert err <= (1e-6 if geo["interp"] else 1e-12), err
