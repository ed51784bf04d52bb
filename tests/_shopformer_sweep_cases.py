"""TEST INFRASTRUCTURE: the geometry sweep of the three Shopformer launches and the per-element
comparison every Shopformer GPU test uses.

Case tables.  A case is a plain dict; ``build(case)`` turns it into (config, seeded state dict) with the generators of
tools/synth_shopformer*.py, ``references(case, config, sd, x)`` evaluates the folded weight image in numpy, once in float64 and once
in float32 (tests/_shopformer*_numpy.py with ``dtype=``).
  V1_CASES   the 16 (V, T, H, L) geometries x heads (1, 2, 4) x layers (1, 4): 96 models of the ``shopformer/`` variant
  V2_CASES   (a) ``spread``: one (d_model, heads) pair per geometry, dim_feedforward cycling (4, 36, 64, 260, 512), layers 1..4; d_model
             equal to, above and below input_dim (without and with the two projections);
             (b) ``ladder``: every d_model 4, 8, ..., 144 on one 12-frame and one 24-frame geometry, the head count walking through the
             divisors of d_model, one layer
  DEC_CASES  the 16 geometries x both variants, with the GCAE decoder
Every case has its own weight seed and window seed.  The adjacency of a 17- and an 18-joint skeleton is data of the committed fixtures
(``default.adj`` / ``kp18_t24.adj`` for variant 1, ``default24.adj`` / ``paper.adj`` for variant 2).  The positional-encoding table is a
checkpoint buffer the kernels only read: a width some fixture stores uses that fixture's table, any other width uses the seeded table
``default_rng(seed).uniform(-1, 1, (1, 8, D))``.

``check_elements(got, f64, f32, name)`` is the comparison: per output array, ``max |got - f64| <= RATIO_MAX[name] * max |f32 - f64|``
and ``mean |got - f64| <= RATIO_MEAN[name] * mean |f32 - f64|``, where f64 / f32 are the numpy evaluations of the same image on the
same windows.  Numpy cannot restate the order of the kernel's MFMA chains, so nothing here is bit for bit: the float32 numpy
evaluation is the yardstick, and the constants say how many yardsticks the kernel may be away.

The constants are the worst ratio measured on an MI355X over every case of the three tables and the fixture configs (256 windows
each, plus the PoseLift windows), times 1.5 for the windows and seeds not drawn, rounded up to one decimal:

  output                 worst max ratio, case                                    worst mean ratio, case                               RATIO_MAX  RATIO_MEAN
  tokens                 3.371  v1-v18_t24_h32_l4-hd1-ly1                         2.272  v1-v18_t24_h64_l8-hd2-ly1                          5.1        3.5
  reconstructed_tokens   6.216  spread-v18_t12_h32_l8-d144-hd12-ff512-ly2         5.361  fixture default24 (shopformer_2), 256 windows      9.4        8.1
  normality_score        3.683  v1-v18_t12_h64_l4-hd4-ly1                         3.017  v1-v18_t12_h64_l4-hd4-ly1                          5.6        4.6
  token_scores           3.366  spread-v17_t12_h32_l8-d4-hd1-ff36-ly2             2.967  spread-v18_t24_h64_l4-d36-hd12-ff512-ly3           5.1        4.5
  gcae_reconstructed     2.840  dec2-v17_t24_h64_l8-d136-hd4-ff36-ly1             1.982  dec1-v17_t24_h32_l4                                4.3        3.0
  pose_error             2.526  dec2-v18_t24_h32_l8-d144-hd4-ff36-ly1             2.004  dec1-v17_t24_h32_l4                                3.8        3.1

(ratio = |gpu - f64| / |numpy fp32 - f64|, max over max and mean over mean, per array.)  The medians over all arrays are 1.4 to 2.1: the
kernel's k-ordered fma chains sit about two numpy-fp32 errors from float64, the deepest shopformer_2 stacks five to six.  Two conditions
hold beside the measurement: with these constants the absolute bound RATIO_MAX * max |f32 - f64| stays below 1e-4 of the array's
largest |f64| on every array of every case (``check_elements`` asserts it; the largest seen is 2.7e-5, reconstructed_tokens of
spread-v17_t12_h32_l8-d4-hd1-ff36-ly2), and tests/test_shopformer_sweep_cases.py shows that the bound rejects a swapped joint, a dropped
edge tap, a row taken from its neighbour, a zeroed group of four features and a window given its neighbour's result.
"""
import numpy as np

from cvsd_amd import shopformer as SF
from tools import synth_shopformer as S1
from tools import synth_shopformer2 as S2
from tools import synth_shopformer_decoder as SDEC

# ------------------------------------------------------------------------------------------------------ the comparison
RATIO_MAX = {"tokens": 5.1, "reconstructed_tokens": 9.4, "normality_score": 5.6, "token_scores": 5.1, "gcae_reconstructed": 4.3,
             "pose_error": 3.8}
RATIO_MEAN = {"tokens": 3.5, "reconstructed_tokens": 8.1, "normality_score": 4.6, "token_scores": 4.5, "gcae_reconstructed": 3.0,
              "pose_error": 3.1}
SHARP = 1e-4            # RATIO_MAX * max |f32 - f64| must stay below SHARP * max |f64|: the bound is far inside the array's range
AXES = {1: ("window",), 2: ("window", "token"), 3: ("window", "token", "feature"), 4: ("window", "channel", "frame", "joint")}


def element_ratios(got, f64, f32) -> dict:
    """the figures ``check_elements`` asserts on, without asserting: the errors of ``got`` and of the float32 yardstick against
    ``f64`` (max and mean), their ratios, the index of the worst element and the largest |f64|"""
    got, f64, f32 = np.asarray(got), np.asarray(f64, np.float64), np.asarray(f32)
    err, yard = np.abs(got.astype(np.float64) - f64), np.abs(f32.astype(np.float64) - f64)
    out = {"err_max": float(err.max()), "err_mean": float(err.mean()), "yard_max": float(yard.max()), "yard_mean": float(yard.mean()),
           "worst": tuple(int(i) for i in np.unravel_index(int(err.argmax()), err.shape)), "range": float(np.abs(f64).max())}
    out["ratio_max"] = out["err_max"] / out["yard_max"] if out["yard_max"] > 0 else (0.0 if out["err_max"] == 0 else float("inf"))
    out["ratio_mean"] = out["err_mean"] / out["yard_mean"] if out["yard_mean"] > 0 else (0.0 if out["err_mean"] == 0 else float("inf"))
    return out


def check_elements(got, f64, f32, name, tag="") -> dict:
    """one output array against the float64 evaluation, element by element, in units of the float32 evaluation's own error"""
    got, f64, f32 = np.asarray(got), np.asarray(f64), np.asarray(f32)
    assert got.shape == f64.shape == f32.shape, (tag, name, got.shape, f64.shape, f32.shape)
    assert np.isfinite(got).all(), f"{tag} {name}: {int((~np.isfinite(got)).sum())} elements are not finite"
    r = element_ratios(got, f64, f32)
    where = ", ".join(f"{a} {i}" for a, i in zip(AXES.get(got.ndim, ()), r["worst"])) or str(r["worst"])
    flat = int(np.ravel_multi_index(r["worst"], got.shape))
    bound = RATIO_MAX[name] * r["yard_max"]
    assert bound < SHARP * r["range"], (f"{tag} {name}: the bound {RATIO_MAX[name]} x max |f32 - f64| = {bound:.3e} is not below {SHARP} of the "
                                        f"array's range {r['range']:.3e}")
    assert r["err_max"] <= bound, (f"{tag} {name}: max |got - f64| = {r['err_max']:.3e} at element {flat} ({where}): got {got[r['worst']]!r}, float64 "
                                   f"{f64[r['worst']]!r}; allowed {RATIO_MAX[name]} x max |f32 - f64| = {bound:.3e} (ratio {r['ratio_max']:.2f})")
    assert r["err_mean"] <= RATIO_MEAN[name] * r["yard_mean"], (
        f"{tag} {name}: mean |got - f64| = {r['err_mean']:.3e}; allowed {RATIO_MEAN[name]} x mean |f32 - f64| = "
        f"{RATIO_MEAN[name] * r['yard_mean']:.3e} (ratio {r['ratio_mean']:.2f}); worst element {flat} ({where})")
    return r


# ------------------------------------------------------------------------------------------------------ the case tables
GEOMETRIES = [(V, T, H, L) for V in (17, 18) for T in (12, 24) for H in (32, 64) for L in (4, 8)]
FF_CYCLE = (4, 36, 64, 260, 512)
# spread (a): geometry index -> (d_model, heads); input_dim = L * V is 68, 136, 72 or 144, so rows 0, 3, 9, 10 and 15 have no projection,
# rows 2, 5, 6 and 12 project upwards and the rest downwards
SPREAD = [(68, 17), (4, 1), (144, 144), (136, 8), (8, 2), (140, 7), (100, 4), (4, 4),
          (16, 16), (144, 12), (72, 24), (64, 1), (132, 3), (20, 5), (36, 12), (144, 1)]
LADDER_GEOMETRIES = [(18, 12, 64, 8), (17, 24, 32, 4)]


def gname(g) -> str:
    return "v{}_t{}_h{}_l{}".format(*g)


def _v1_cases():
    out = []
    for gi, g in enumerate(GEOMETRIES):
        for heads in (1, 2, 4):
            for layers in (1, 4):
                i = len(out)
                out.append({"id": f"v1-{gname(g)}-hd{heads}-ly{layers}", "variant": 1, "geometry": g, "heads": heads, "layers": layers,
                            "decoder": False, "seed_w": 1000 + i, "seed_x": 5000 + i})
    return out


def _v2_case(tag, i, g, d, heads, ff, layers, decoder=False, seed=2000):
    return {"id": f"{tag}-{gname(g)}-d{d}-hd{heads}-ff{ff}-ly{layers}", "variant": 2, "geometry": g, "d_model": d, "heads": heads, "ff": ff,
            "layers": layers, "decoder": decoder, "group": tag, "seed_w": seed + i, "seed_x": seed + 4000 + i}


def _v2_cases():
    out = [_v2_case("spread", i, g, d, h, FF_CYCLE[i % 5], i % 4 + 1) for i, (g, (d, h)) in enumerate(zip(GEOMETRIES, SPREAD))]
    for g in LADDER_GEOMETRIES:
        for j, d in enumerate(range(4, 145, 4)):
            div = [h for h in range(1, d + 1) if d % h == 0]
            out.append(_v2_case("ladder", len(out), g, d, div[j % len(div)], FF_CYCLE[j % 5], 1))
    return out


def _dec_cases():
    out = []
    for gi, g in enumerate(GEOMETRIES):
        out.append({"id": f"dec1-{gname(g)}", "variant": 1, "geometry": g, "heads": (1, 2, 4)[gi % 3], "layers": 1, "decoder": True,
                    "seed_w": 3000 + 2 * gi, "seed_x": 7000 + 2 * gi, "seed_dec": 9000 + 2 * gi})
        c = _v2_case("dec2", 2 * gi + 1, g, (96, g[0] * g[3])[gi % 2], 4, 36, 1, decoder=True, seed=3000)
        c["seed_dec"] = 9001 + 2 * gi
        out.append(c)
    return out


V1_CASES = _v1_cases()
V2_CASES = _v2_cases()
DEC_CASES = _dec_cases()
ALL_CASES = V1_CASES + V2_CASES + DEC_CASES
OUTPUTS_1 = ("tokens", "reconstructed_tokens", "normality_score")
OUTPUTS_2 = OUTPUTS_1 + ("token_scores",)
POSE_OUTPUTS = ("gcae_reconstructed", "pose_error")


def outputs_of(case):
    return (OUTPUTS_2 if case["variant"] == 2 else OUTPUTS_1) + (POSE_OUTPUTS if case["decoder"] else ())


# ------------------------------------------------------------------------------------------------------ case -> checkpoint
_FIX = {}


def _fixture(variant):
    if variant not in _FIX:
        _FIX[variant] = (S1 if variant == 1 else S2).load_fixture()
    return _FIX[variant]


def adjacency(variant, V):
    name = {(1, 17): "default", (1, 18): "kp18_t24", (2, 17): "default24", (2, 18): "paper"}[(variant, V)]
    return _fixture(variant)[name + ".adj"]


def pe_table(variant, D, seed):
    """the fixture's table when one of that width is stored, else the seeded one of the module docstring"""
    stored = {1: {136: "default", 144: "kp18_t24", 68: "h32_l4"}, 2: {144: "paper"}}[variant].get(D)
    if stored:
        return _fixture(variant)[stored + ".pe"]
    return np.random.default_rng(seed).uniform(-1, 1, (1, 8, D)).astype(np.float32)


def config_of(case):
    V, T, H, L = case["geometry"]
    if case["variant"] == 1:
        return {"seq_len": T, "num_keypoints": V, "num_tokens": 2, "hidden_channels": H, "latent_channels": L,
                "transformer_heads": case["heads"], "transformer_layers": case["layers"]}
    return {"model": {"in_channels": 2, "num_keypoints": V, "seq_len": T, "num_tokens": 2,
                      "gcae": {"hidden_channels": H, "latent_channels": L, "num_layers": 4},
                      "transformer": {"input_dim": L * V, "d_model": case["d_model"], "num_heads": case["heads"], "num_layers": case["layers"],
                                      "dim_feedforward": case["ff"]}}}


def build(case):
    """-> (config, state dict) of one case"""
    V, T, H, L = case["geometry"]
    cfg = config_of(case)
    if case["variant"] == 1:
        sd = S1.synthetic_state_dict(cfg, adjacency(1, V), pe_table(1, L * V, case["seed_w"]), seed=case["seed_w"])
    else:
        sd = S2.synthetic_state_dict(cfg, adjacency(2, V), pe_table(2, case["d_model"], case["seed_w"]), seed=case["seed_w"])
    if case["decoder"]:
        sd = dict(sd)
        sd.update(SDEC.synthetic_decoder_state_dict(cfg, seed=case["seed_dec"]))
    return cfg, sd


def windows(case, n):
    V, T, _, _ = case["geometry"]
    return S1.synthetic_windows(n, {"seq_len": T, "num_keypoints": V}, seed=case["seed_x"])


def references(case, cfg, sd, x):
    """-> (float64 outputs, float32 outputs) of the numpy evaluations of the case's weight image on windows ``x``; with the decoder,
    ``gcae_reconstructed`` is the decoder on that evaluation's own tokens and ``pose_error`` half the squared distance to the window"""
    import _shopformer2_numpy as R2
    import _shopformer_decoder_numpy as RD
    import _shopformer_numpy as R1
    geo, t = SF.parse_image(SF.image_from_state_dict(sd, cfg, decoder=case["decoder"]))
    R = R1 if case["variant"] == 1 else R2
    out = []
    for dtype in (np.float64, np.float32):
        o = dict(R.forward(geo, t, x, dtype=dtype))
        if case["decoder"]:
            o["gcae_reconstructed"] = RD.decode(geo, t, o["tokens"], dtype=dtype)
            if dtype is np.float64:
                d = o["gcae_reconstructed"] - np.asarray(x, np.float64)
                o["pose_error"] = 0.5 * (d[:, 0] ** 2 + d[:, 1] ** 2)
            else:
                o["pose_error"] = RD.pose_error_f32(o["gcae_reconstructed"], x)
        assert all(v.dtype == dtype for v in o.values()), {k: v.dtype for k, v in o.items()}
        out.append(o)
    return out[0], out[1]


# ------------------------------------------------------------------------------------------------------ the planner, restated
LDS_BYTES = 160 * 1024


def _pad_stride(k):
    c = (k + 3) // 4 * 4
    return c + 4 if (c // 4) % 2 == 0 else c


def _up4(n):
    return (n + 3) // 4 * 4


def lds_tokenizer(geo, G):
    """bytes of LDS of the first launch for G windows per workgroup (shopformer_host.hip's formula)"""
    V, T, H, D, ntok = geo["V"], geo["T"], geo["H"], geo["D"], geo["ntok"]
    v2 = geo.get("variant", 1) == 2
    csH, csD, csQ, csF = _pad_stride(H), _pad_stride(max(D, geo.get("Din", D))), _pad_stride(3 * D), _pad_stride(geo["ff"])
    inp = _up4(G * T * V * 2)
    tf = 0 if v2 else G * ntok * (5 * csD + csQ + csF) + _up4(G * geo["heads"] * ntok * ntok)
    return (2 * inp + max(G * geo["T1"] * V * csH, tf) + G * max(geo["T2"], geo["T4"]) * V * csH) * 4


def lds_transformer(geo, GT):
    """bytes of LDS of variant 2's transformer launch for a row group of GT windows"""
    D, ntok = geo["D"], geo["ntok"]
    csD, csQ, csF = _pad_stride(max(D, geo["Din"])), _pad_stride(3 * D), _pad_stride(geo["ff"])
    rows = GT * ntok
    return (3 * rows * csD + rows * max(csQ + csD, csF) + _up4(GT * geo["heads"] * ntok * ntok)) * 4


def lds_decoder(geo, G):
    V, H, ntok = geo["V"], geo["H"], geo["ntok"]
    return (G * ntok * _pad_stride(geo["L"] * V) + G * ntok * V * _pad_stride(H) + _up4(G * 2 * geo["Tdec"] * V)) * 4


def plan(geo) -> dict:
    """-> {'G': tokenizer windows per workgroup, 'GT': transformer row group (0 for variant 1), 'GD': decoder row group (0 without
    one)}; 0 for G or GT where not even one window fits"""
    G = next((g for g in range(8, 0, -1) if lds_tokenizer(geo, g) <= LDS_BYTES), 0)
    GT = next((g for g in (16, 8, 4, 2, 1) if lds_transformer(geo, g) <= LDS_BYTES), 0) if geo.get("variant", 1) == 2 else 0
    GD = 0
    if "Tdec" in geo:
        GD = 4
        while GD > 1 and lds_decoder(geo, GD) > LDS_BYTES:
            GD -= 1
    return {"G": G, "GT": GT, "GD": GD}


def geometry_of(variant, V, T, H, L, heads, layers=1, d_model=None, ff=SF.FF_DIM) -> dict:
    """the planner's inputs for any config of the accepted envelope, without building a checkpoint"""
    if variant == 1:
        strides, D = SF.block_strides(T, 2), L * V
    else:
        strides, D = SF.compute_strides_2(T, 2, SF.N_BLOCKS)[0], d_model
    tn = [T]
    for s in strides:
        tn.append((tn[-1] - 1) // s + 1)
    return {"V": V, "T": T, "H": H, "L": L, "heads": heads, "layers": layers, "ff": ff, "D": D, "Din": L * V, "ntok": tn[4], "variant": variant,
            "T1": tn[1], "T2": tn[2], "T3": tn[3], "T4": tn[4]}
