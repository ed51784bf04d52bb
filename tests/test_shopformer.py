"""Shopformer score path without a GPU: the loader (fold, pack, image), the windowing, and the folded network against the
REFERENCE'S OWN float64 outputs stored in tests/golden/shopformer_fixture*.npz (tests/golden/make_shopformer_fixture.py).

Figures measured when the fixture was made (max error / full scale of the tensor, worst of the three configs):
  float64 fold through pack / unpack, evaluated in float64 ....... tokens 1e-15, reconstruction 3e-15, score 2e-15  (bound 1e-10 -> 1e-12)
  the float32 weight image itself, evaluated in float64 .......... 7.4e-08 / 4.3e-08 / 5.3e-08: rounding the folded weights to fp32
  once (6e-8 relative each) is in it, so it cannot meet a 1e-10 bound; it is instead required to BE the rounding of the float64 fold,
  bit for bit, which ties the kernel's image to the 1e-12 proof."""
import os

import numpy as np
import pytest
import torch

import _shopformer_numpy as R
from _poselift_windows import unflatten
from cvsd_amd import shopformer as SF

CONFIGS = ["default", "kp18_t24", "h32_l4"]
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def fix():
    return R.load_fixture()


@pytest.mark.parametrize("name", CONFIGS)
def test_image_round_trips_and_is_the_rounded_float64_fold(fix, name):
    cfg, sd, _ = R.fixture_model(fix, name)
    geo, t32 = SF.fold_state_dict(sd, cfg)
    geo2, back = SF.parse_image(SF.build_image(geo, t32))
    _, t64 = SF.fold_state_dict(sd, cfg, dtype=np.float64)
    assert geo2 == geo and set(back) == set(t32) == set(t64)
    assert geo["ntok"] == 3 and [geo[f"s{i}"] for i in range(4)] == ([2, 2, 1, 1] if geo["T"] == 12 else [2, 2, 2, 1])
    for k in t32:
        np.testing.assert_array_equal(back[k].reshape(-1), t32[k].reshape(-1), err_msg=k)
        np.testing.assert_array_equal(t32[k], t64[k].astype(np.float32), err_msg=k)
    w = np.arange(40 * 9 * 24, dtype=np.float32).reshape(40, 9, 24)
    np.testing.assert_array_equal(SF.unpack_mfma(SF.pack_mfma(w), 40, 9, 24), w)


@pytest.mark.parametrize("field,value", [("num_keypoints", 25), ("seq_len", 16), ("hidden_channels", 48), ("latent_channels", 6),
                                          ("transformer_heads", 3), ("transformer_layers", 5), ("num_tokens", 3)])
def test_unsupported_config_is_refused_with_the_field_named(field, value):
    with pytest.raises(ValueError, match=field):
        SF.resolve_config({field: value})


def test_heads_must_divide_the_token_width():
    with pytest.raises(ValueError, match="transformer_heads"):
        SF.resolve_config({"latent_channels": 4, "num_keypoints": 17, "transformer_heads": 8})
    assert SF.resolve_config({"latent_channels": 4, "transformer_heads": 4})["transformer_heads"] == 4


def test_without_a_gpu_construction_raises(fix):
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from cvsd_amd import Shopformer
    from cvsd_amd._lib import Mi355Error
    cfg, sd, _ = R.fixture_model(fix, "default")
    with pytest.raises((Mi355Error, ValueError)):
        Shopformer.from_state_dict(sd, cfg)


@pytest.mark.parametrize("name", CONFIGS)
def test_folded_network_in_float64_equals_the_reference_in_float64(fix, name):
    cfg, sd, x = R.fixture_model(fix, name)
    geo, t64 = SF.fold_state_dict(sd, cfg, dtype=np.float64)
    # through the kernel's layout: pack to MFMA fragment order and back (float64 keeps the fold unrounded)
    t64 = {k: (SF.unpack_mfma(_pack64(v), *v.shape) if SF._is_matrix(k) else v) for k, v in t64.items()}
    out = R.forward(geo, t64, x)
    _, t32 = SF.parse_image(SF.image_from_state_dict(sd, cfg))
    out32 = R.forward(geo, t32, x)
    for key, ref in (("tokens", "tokens"), ("reconstructed_tokens", "recon"), ("normality_score", "score")):
        want = fix[f"{name}.{ref}_f64"]
        err = np.abs(out[key] - want).max() / np.abs(want).max()
        err32 = np.abs(out32[key] - want).max() / np.abs(want).max()
        print(f"{name} {key}: float64 fold {err:.2e} of full scale; fp32 image {err32:.2e}")
        assert out[key].shape == want.shape
        assert err <= 1e-12, (key, err)          # the issue's 1e-10, tightened to what held (figures in the module docstring)
        # rounding each folded weight to fp32 once (2^-24 = 6e-8 relative): measured 1.4e-8 .. 7.4e-8 of full scale over the 9 cells; one
        # mis-folded channel of 64 moves a tensor by 1e-3 or more, so 2e-7 (3 roundings' worth) separates the two by four orders
        assert err32 <= 2e-7, (key, err32)


def _pack64(w):
    """pack_mfma's permutation applied to float64 (the product packs float32)"""
    co, taps, ci = w.shape
    nct, cib = (co + 15) // 16, (ci + 15) // 16
    pad = np.zeros((nct * 16, taps, cib * 16), np.float64)
    pad[:co, :, :ci] = w
    idx = SF.unpack_mfma(np.arange(nct * taps * cib * 256), nct * 16, taps, cib * 16)      # logical -> flat position
    flat = np.zeros(nct * taps * cib * 256, np.float64)
    flat[idx.reshape(-1)] = pad.reshape(-1)
    return flat


@pytest.mark.parametrize("split", ["train", "test"])
def test_windows_from_poselift_equal_the_reference_loader(split):
    pf = np.load(os.path.join(GOLD, "poselift_fixture.npz"))
    data = unflatten(pf["frame_keys"], pf["row_frame"], pf["row_pid"], pf["row_bbox"], pf["row_kpts"])
    x, index = SF.windows_from_poselift(data, seq_len=int(pf["meta"][6]), stride=int(pf["meta"][7]))
    np.testing.assert_array_equal(x, pf[f"{split}_xy_x"])                    # same float32 bits, same order
    assert len(index) == len(x) > 0 and all(b - a >= 11 for _, a, b in index)


class _StubModel:
    seq_len, num_keypoints = 12, 17

    def score(self, w):
        return np.asarray(w, np.float64).reshape(len(w), -1).sum(1).astype(np.float32)


def test_stream_scorer_cuts_the_same_windows_as_the_offline_path():
    pf = np.load(os.path.join(GOLD, "poselift_fixture.npz"))
    data = unflatten(pf["frame_keys"], pf["row_frame"], pf["row_pid"], pf["row_bbox"], pf["row_kpts"])
    model = _StubModel()
    scores, index = SF.score_poselift(model, data)
    offline = sorted((pid, a, b, float(s)) for (pid, a, b), s in zip(index, scores))
    st, live = SF.StreamScorer(model), []
    for f in sorted(data):
        rows = np.asarray([[b[0], b[1], b[0] + b[2], b[1] + b[3], pid] for pid, (b, _) in data[f].items()], np.float32).reshape(-1, 5)
        live += st.update(f, rows, np.asarray([k for _, k in data[f].values()], np.float32).reshape(-1, 17, 3))
    assert sorted(live) == offline and len(live) > 0


def test_gap_rule_and_nan_poses():
    k = np.ones((17, 3), np.float32)
    k[:, 0] = np.arange(17)
    data = {f: {1: [np.zeros(4, np.float32), k * (1 + 0.01 * f)]} for f in list(range(12)) + [30] + list(range(31, 42))}
    x, index = SF.windows_from_poselift(data)
    assert [i[1:] for i in index] == [(0, 11), (30, 41)]                     # the window that straddles the 18-frame gap is dropped
    data[5][1][1] = np.full((17, 3), np.nan, np.float32)
    assert (0, 11) not in [i[1:] for i in SF.windows_from_poselift(data)[1]]
    assert np.abs(x).max() <= 1.0


def test_flat_keypoint_rows_are_read_like_the_loader_reads_them():
    k = np.ones((17, 3), np.float32)
    k[:, 0] = np.arange(17)
    nested = {f: {1: [np.zeros(4, np.float32), k * (1 + 0.01 * f)]} for f in range(12)}
    flat = {f: {1: [np.zeros(4, np.float32), (k * (1 + 0.01 * f)).reshape(-1)]} for f in range(12)}
    np.testing.assert_array_equal(SF.windows_from_poselift(flat)[0], SF.windows_from_poselift(nested)[0])


def test_stream_scorer_gives_back_the_poses_of_ended_tracks_and_keeps_the_cut_positions():
    k = np.ones((17, 3), np.float32)
    k[:, 0] = np.arange(17)
    frames = list(range(14)) + list(range(40, 60))                            # one id, a 26-frame hole
    data = {f: {7: [np.zeros(4, np.float32), k * (1 + 0.01 * f)]} for f in frames}
    model = _StubModel()
    scores, index = SF.score_poselift(model, data)
    st, live = SF.StreamScorer(model), []
    for f in frames:
        live += st.update(f, np.asarray([[0, 0, 1, 1, 7]], np.float32), np.asarray([data[f][7][1]]))
        if f == 40:
            assert len(st._ring[7]) == 1                                       # the 12 poses from before the hole are gone
    assert sorted(live) == sorted((pid, a, b, float(s)) for (pid, a, b), s in zip(index, scores)) and len(live) >= 2
    st.update(200, np.zeros((0, 5), np.float32), np.zeros((0, 17, 3), np.float32))
    assert not st._ring
