"""The shopformer_2 variant without a GPU: the restated stride rule, the refusals, the fold and the version-2 image against the
REFERENCE'S OWN float64 outputs (tests/golden/shopformer2_fixture*.npz, made by tests/golden/make_shopformer2_fixture.py), the neck
joint of the windows, the unchanged version-1 image, and the C loader's refusals of bad version-2 images.

Figures measured when the fixture was made (max error / full scale, worst of the three configs): float64 fold evaluated in float64
1.7e-15 (bound 1e-12, the one test_shopformer.py uses); the float32 image evaluated in float64 8.7e-08 (bound 2e-7, likewise)."""
import copy
import ctypes as C
import hashlib
import os
import struct

import numpy as np
import pytest
import torch

import _shopformer2_numpy as R2
import _shopformer_numpy as R
from _poselift_windows import unflatten
from cvsd_amd import shopformer as SF
from tools import synth_shopformer2 as S2

CONFIGS = ["paper", "default24", "paper_t24"]
GOLD = os.path.join(os.path.dirname(__file__), "golden")
KEYS = (("tokens", "tokens"), ("reconstructed_tokens", "recon"), ("normality_score", "score"), ("token_scores", "token_scores"))
# SHA-256 of the version-1 weight image of the three shopformer/ fixture checkpoints, computed on the parent commit
V1_SHA256 = {"default": "31033be276f33a4addfe72e73314eef542a9ad3560ee68fcf3f1e3113e39197b",
             "kp18_t24": "853b47a35bc2f4cdbf6c6d02a35276349f590efc2b0eebdcc517c110a96c343c",
             "h32_l4": "c08d25628f106d06c08755bbfa171da38ebe594dd9e8991813b4e8c6eeb4ddf9"}
# SHA-256 of windows_from_poselift(poselift fixture, num_keypoints=18) (zero-padded joint 17), computed on the parent commit
KP18_NO_NECK_SHA256 = "ae6407889b3469bfe7bd49febbaa352f202ba8762b6b4cdd78354125f890f7aa"


@pytest.fixture(scope="module")
def fix():
    return R2.load_fixture()


def _poselift():
    pf = np.load(os.path.join(GOLD, "poselift_fixture.npz"))
    return pf, unflatten(pf["frame_keys"], pf["row_frame"], pf["row_pid"], pf["row_bbox"], pf["row_kpts"])


def test_restated_stride_rule_equals_the_recorded_table(fix):
    assert len(fix["strides_table"]) == 12
    for T, nt, s0, s1, s2, s3, final, pool in fix["strides_table"]:
        assert SF.compute_strides_2(int(T), int(nt)) == ([s0, s1, s2, s3], final, bool(pool)), (T, nt)
    assert SF.compute_strides_2(12, 2)[0] == [3, 2, 1, 1] and SF.compute_strides_2(24, 2)[0] == [3, 2, 2, 1]
    assert SF.compute_strides_2(12, 5) == ([2, 1, 1, 1], 6, True)               # 12 // 5 = 2: ends at 6 frames, the pool would make 5


def _with(path, value):
    cfg = copy.deepcopy(S2.CONFIGS["paper"])
    d = cfg["model"]
    *head, last = path.split(".")
    for k in head:
        d = d[k]
    d[last] = value
    return cfg


@pytest.mark.parametrize("path,value,named", [
    ("num_tokens", 5, "num_tokens"),                       # strides [2, 1, 1, 1] end at 6 frames: needs the adaptive pool
    ("num_tokens", 3, "num_tokens"),
    ("seq_len", 36, "seq_len"),
    ("in_channels", 3, "in_channels"),
    ("gcae.num_layers", 3, "gcae.num_layers"),
    ("transformer.input_dim", 136, "transformer.input_dim"),
    ("transformer.num_heads", 5, "transformer.num_heads"),
    ("transformer.num_layers", 5, "transformer.num_layers"),
    ("transformer.dim_feedforward", 66, "transformer.dim_feedforward"),
    ("transformer.dim_feedforward", 1024, "transformer.dim_feedforward"),
    ("transformer.d_model", 150, "transformer.d_model"),
    ("num_keypoints", 25, "num_keypoints"),
    ("gcae.hidden_channels", 48, "gcae.hidden_channels"),
])
def test_unsupported_config_is_refused_with_the_field_named(path, value, named):
    with pytest.raises(ValueError, match=named.replace(".", r"\.")):
        SF.resolve_config_2(_with(path, value))


def test_pool_configs_are_refused_by_the_stride_check_itself(monkeypatch):
    monkeypatch.setitem(SF.SUPPORTED_2, "num_tokens", (2, 5))
    with pytest.raises(ValueError, match="adaptive average pool"):
        SF.resolve_config_2(_with("num_tokens", 5))


def test_variant_is_detected_from_the_config_or_given(fix):
    cfg, sd, _ = R2.fixture_model(fix, "paper")
    assert SF.is_variant_2(cfg) and not SF.is_variant_2({"seq_len": 12}) and not SF.is_variant_2(None)
    geo, _ = SF.fold_state_dict(sd, cfg)
    assert geo["variant"] == 2 and geo["ntok"] == 2 and [geo[f"s{i}"] for i in range(4)] == [3, 2, 1, 1]
    assert SF.fold_state_dict(sd, cfg, variant=2)[0] == geo
    with pytest.raises(ValueError, match="has no tensor"):
        SF.fold_state_dict(sd, {"num_keypoints": 18}, variant=1)                # a shopformer_2 state dict is not a shopformer/ one
    with pytest.raises(ValueError, match="variant"):
        SF.fold_state_dict(sd, cfg, variant=3)


@pytest.mark.parametrize("name", CONFIGS)
def test_folded_network_in_float64_equals_the_reference_in_float64(fix, name):
    cfg, sd, x = R2.fixture_model(fix, name)
    geo, t64 = SF.fold_state_dict(sd, cfg, dtype=np.float64)
    from test_shopformer import _pack64
    t64 = {k: (SF.unpack_mfma(_pack64(v), *v.shape) if SF._is_matrix(k) else v) for k, v in t64.items()}
    out = R2.forward(geo, t64, x)
    geo32, t32 = SF.parse_image(SF.image_from_state_dict(sd, cfg))
    out32 = R2.forward(geo32, t32, x)
    for key, ref in KEYS:
        want = fix[f"{name}.{ref}_f64"]
        err = np.abs(out[key] - want).max() / np.abs(want).max()
        err32 = np.abs(out32[key] - want).max() / np.abs(want).max()
        print(f"{name} {key}: float64 fold {err:.2e} of full scale; fp32 image {err32:.2e}")
        assert out[key].shape == want.shape
        assert err <= 1e-12, (key, err)
        assert err32 <= 2e-7, (key, err32)


@pytest.mark.parametrize("name", CONFIGS)
def test_version_2_image_round_trips_and_is_the_rounded_float64_fold(fix, name):
    cfg, sd, _ = R2.fixture_model(fix, name)
    geo, t32 = SF.fold_state_dict(sd, cfg)
    blob = SF.build_image(geo, t32)
    assert struct.unpack_from("<II", blob, 8) == (2, len(SF.CFG_FIELDS_V2))
    geo2, back = SF.parse_image(blob)
    _, t64 = SF.fold_state_dict(sd, cfg, dtype=np.float64)
    assert geo2 == geo and set(back) == set(t32) == set(t64)
    assert geo["in_proj"] == geo["out_proj"] == int(name == "default24") and ("inp.w" in t32) == (name == "default24")
    for k in t32:
        np.testing.assert_array_equal(back[k].reshape(-1), t32[k].reshape(-1), err_msg=k)
        np.testing.assert_array_equal(t32[k], t64[k].astype(np.float32), err_msg=k)


def test_checkpoint_forms_yaml_config_and_split_state_dicts(fix, tmp_path):
    cfg, sd, _ = R2.fixture_model(fix, "paper")
    want = SF.image_from_state_dict(sd, cfg)
    tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    p1 = str(tmp_path / "best.pt")
    torch.save({"model_state_dict": tsd, "config": cfg, "epoch": 3}, p1)
    assert SF.image_from_checkpoint(p1) == want                                   # the config stored in the checkpoint
    p2 = str(tmp_path / "split.pt")
    torch.save({"gcae_state_dict": {k[5:]: v for k, v in tsd.items() if k.startswith("gcae.")},
                "transformer_state_dict": {k[12:]: v for k, v in tsd.items() if k.startswith("transformer.")}}, p2)
    import yaml
    y = str(tmp_path / "paper.yaml")
    with open(y, "w") as f:
        yaml.safe_dump(cfg, f)
    assert SF.image_from_checkpoint(p2, y) == want and SF.image_from_checkpoint(p2, cfg) == want


@pytest.mark.parametrize("name", sorted(V1_SHA256))
def test_version_1_image_is_unchanged_byte_for_byte(name):
    fix1 = R.load_fixture()
    cfg, sd, _ = R.fixture_model(fix1, name)
    blob = SF.image_from_state_dict(sd, cfg)
    assert struct.unpack_from("<II", blob, 8) == (1, len(SF.CFG_FIELDS))
    assert hashlib.sha256(blob).hexdigest() == V1_SHA256[name]


@pytest.mark.parametrize("split", ["train", "test"])
def test_neck_windows_equal_the_shopformer_2_loader(split):
    pf, data = _poselift()
    x, index = SF.windows_from_poselift(data, seq_len=int(pf["meta"][6]), stride=int(pf["meta"][7]), num_keypoints=18, neck=True)
    np.testing.assert_array_equal(x, pf[f"s2_{split}_xy_x"])                 # same float32 bits, same order
    assert x.dtype == np.float32 and len(index) == len(x) > 0


def test_without_neck_the_windows_are_unchanged():
    pf, data = _poselift()
    x, _ = SF.windows_from_poselift(data, num_keypoints=18)
    assert hashlib.sha256(x.tobytes()).hexdigest() == KP18_NO_NECK_SHA256
    np.testing.assert_array_equal(SF.windows_from_poselift(data)[0], pf["train_xy_x"])
    with pytest.raises(ValueError, match="neck"):
        SF.windows_from_poselift(data, num_keypoints=17, neck=True)


def test_neck_rule_for_missing_shoulders_equals_the_recorded_outputs(fix):
    for j, (pose, want) in enumerate(zip(fix["neck_in"], fix["neck_out"])):
        got = SF._with_neck(pose if j != 4 else pose[:15])
        np.testing.assert_array_equal(got, want)
    assert np.array_equal(fix["neck_out"][1][17], fix["neck_in"][1][6]) and not fix["neck_out"][3][17, :2].any()


class _StubModel2:
    seq_len, num_keypoints, neck = 12, 18, True

    def score(self, w):
        assert np.asarray(w).shape[1:] == (2, 12, 18)
        return np.asarray(w, np.float64).reshape(len(w), -1).sum(1).astype(np.float32)


def test_stream_scorer_cuts_the_same_neck_windows_as_the_offline_path():
    pf, data = _poselift()
    model = _StubModel2()
    scores, index = SF.score_poselift(model, data)
    np.testing.assert_array_equal(scores, model.score(pf["s2_train_xy_x"]))      # score_poselift took `neck` from the model
    offline = sorted((pid, a, b, float(s)) for (pid, a, b), s in zip(index, scores))
    st, live = SF.StreamScorer(model), []
    for f in sorted(data):
        rows = np.asarray([[b[0], b[1], b[0] + b[2], b[1] + b[3], pid] for pid, (b, _) in data[f].items()], np.float32).reshape(-1, 5)
        live += st.update(f, rows, np.asarray([k for _, k in data[f].values()], np.float32).reshape(-1, 17, 3))
    assert sorted(live) == offline and len(live) > 0


# ---------------------------------------------------------------------------------------------- the C loader, no GPU needed
def _create(blob):
    from cvsd_amd import _lib
    h = C.c_void_p()
    rc = _lib.lib().mi355_shopformer_create(blob, len(blob), 0, C.byref(h))
    msg = _lib.lib().mi355_last_error().decode(errors="replace")
    if h.value:
        _lib.lib().mi355_shopformer_destroy(h)
    return rc, msg


def _patched(geo, t32, **over):
    g = dict(geo)
    g.update(over)
    return SF.build_image(g, t32)


@pytest.mark.parametrize("over,named", [
    ({"ff": 516}, "transformer.dim_feedforward"), ({"ff": 66}, "transformer.dim_feedforward"), ({"heads": 5}, "transformer.num_heads"),
    ({"layers": 5}, "transformer.num_layers"), ({"Din": 136}, "transformer.input_dim"), ({"s0": 4}, "block stride"),
    ({"in_proj": 1}, "input projection"), ({"norm_kind": 0}, "norm kind"), ({"act_kind": 0}, "activation kind"), ({"ntok": 3}, "token count"),
    ({"D": 148}, "transformer.d_model"),
])
def test_c_loader_refuses_bad_version_2_fields_before_the_device(fix, over, named):
    cfg, sd, _ = R2.fixture_model(fix, "paper")
    geo, t32 = SF.fold_state_dict(sd, cfg)
    rc, msg = _create(_patched(geo, t32, **over))
    assert rc == -3 and named in msg, (rc, msg)                                  # MI355_EFORMAT, not a HIP error


def test_c_loader_refuses_truncated_and_incomplete_version_2_images(fix):
    cfg, sd, _ = R2.fixture_model(fix, "default24")
    geo, t32 = SF.fold_state_dict(sd, cfg)
    blob = SF.build_image(geo, t32)
    table_end = 16 + 4 * len(SF.CFG_FIELDS_V2) + 4 + 64 * len(t32)
    for cut in (40, 16 + 4 * len(SF.CFG_FIELDS_V2), table_end - 10):
        rc, msg = _create(blob[:cut])
        assert rc == -3 and "truncated" in msg, (cut, rc, msg)
    rc, msg = _create(blob[:table_end + 4096])                                   # table whole, data cut
    assert rc == -3 and "outside the file" in msg, (rc, msg)
    for gone in ("en.g", "outp.w", "d3.n3.b"):
        rc, msg = _create(SF.build_image(geo, {k: v for k, v in t32.items() if k != gone}))
        assert rc == -3 and gone in msg, (gone, rc, msg)
    head = bytearray(blob)
    struct.pack_into("<I", head, 8, 3)
    rc, msg = _create(bytes(head))
    assert rc == -3 and "version" in msg


def test_without_a_gpu_construction_raises(fix):
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from cvsd_amd import Shopformer
    from cvsd_amd._lib import Mi355Error
    cfg, sd, _ = R2.fixture_model(fix, "paper")
    with pytest.raises(Mi355Error, match="no HIP device"):
        Shopformer.from_state_dict(sd, cfg)
