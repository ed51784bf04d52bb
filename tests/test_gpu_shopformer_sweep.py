"""The three Shopformer launches on the GPU over the geometries the loaders accept (tests/_shopformer_sweep_cases.py): every output of
every case, element by element, against the float64 numpy evaluation of the same weight image, in units of the float32 numpy
evaluation's own error (``check_elements``).  Each model runs n = 3 * group - 1 windows (at least 19), so that a full group of the
workgroup's windows, a second full group and a short last group are all there; calls on the first 1 .. group - 1 windows return the
bits of the big call's first rows."""
import numpy as np
import pytest

import _shopformer_sweep_cases as C

pytestmark = pytest.mark.gpu


def evaluate(case):
    """-> (model, windows, forward of them with every output the case has, the groups the engine planned).  A model the Python loader
    accepts must load: a refusal by mi355_shopformer_create raises here and fails the test."""
    from cvsd_amd import Shopformer
    cfg, sd = C.build(case)
    model = Shopformer.from_state_dict(sd, cfg, device=0, decoder=case["decoder"])
    groups = {"G": int(model.info.group), "GT": int(model.info.group_transformer) if case["variant"] == 2 else 0,
              "GD": int(model.decoder_info.group) if case["decoder"] else 0}
    x = C.windows(case, max(19, 3 * max(max(groups.values()), 1) - 1))
    return model, cfg, sd, x, model.forward(x, poses=case["decoder"]), groups


def check_case(case):
    model, cfg, sd, x, got, groups = evaluate(case)
    assert groups == C.plan(model.geometry), (case["id"], groups)                # the planner as tests/_shopformer_sweep_cases.py restates it
    assert model.info.lds_bytes <= C.LDS_BYTES and model.variant == case["variant"]
    f64, f32 = C.references(case, cfg, sd, x)
    assert set(C.outputs_of(case)) <= set(got)
    for name in C.outputs_of(case):
        r = C.element_ratios(got[name], f64[name], f32[name])
        print(f"{case['id']} {groups} n={len(x)} {name}: max |gpu - f64| {r['err_max']:.3e} = {r['ratio_max']:.3f} x numpy fp32's, "
              f"mean {r['err_mean']:.3e} = {r['ratio_mean']:.3f} x; bound / range {C.RATIO_MAX[name] * r['yard_max'] / r['range']:.2e}")
    for name in C.outputs_of(case):
        C.check_elements(got[name], f64[name], f32[name], name, case["id"])
    for r in range(1, max(groups.values())):                                      # a short only group: the big call's first rows, bit for bit
        part = model.forward(x[:r], poses=case["decoder"])
        for name in C.outputs_of(case):
            assert np.array_equal(part[name], got[name][:r]), (case["id"], name, r)


def _chunks(cases, k=6):
    return [cases[i:i + k] for i in range(0, len(cases), k)]


@pytest.mark.parametrize("geometry", C.GEOMETRIES, ids=C.gname)
def test_variant_1_every_element(geometry):
    cases = [c for c in C.V1_CASES if c["geometry"] == geometry]
    assert len(cases) == 6
    for case in cases:
        check_case(case)


SPREAD = _chunks([c for c in C.V2_CASES if c["group"] == "spread"])
LADDER = _chunks([c for c in C.V2_CASES if c["group"] == "ladder"])


@pytest.mark.parametrize("cases", SPREAD, ids=[f"geometries_{6 * i}_to_{6 * i + len(g) - 1}" for i, g in enumerate(SPREAD)])
def test_variant_2_spread_every_element(cases):
    for case in cases:
        check_case(case)


@pytest.mark.parametrize("cases", LADDER, ids=[f"{C.gname(g[0]['geometry'])}_d{g[0]['d_model']}_to_d{g[-1]['d_model']}" for g in LADDER])
def test_variant_2_width_ladder_every_element(cases):
    assert len({c["geometry"] for c in cases}) == 1
    for case in cases:
        check_case(case)


@pytest.mark.parametrize("geometry", C.GEOMETRIES, ids=C.gname)
def test_decoder_every_element(geometry):
    cases = [c for c in C.DEC_CASES if c["geometry"] == geometry]
    assert [c["variant"] for c in cases] == [1, 2]
    for case in cases:
        check_case(case)


# ------------------------------------------------------------------------------------------------------ row-group overrides
def _same_bits(case, monkeypatch, env, values, field, expect):
    from cvsd_amd import Shopformer
    model, cfg, sd, x, base, groups = evaluate(case)
    tried = []
    for v in values:
        want = expect(v, groups, model.geometry)
        if want is None:
            continue
        monkeypatch.setenv(env, str(v))
        other = Shopformer.from_state_dict(sd, cfg, device=0, decoder=case["decoder"])
        monkeypatch.delenv(env)
        got_group = int(other.info.group_transformer) if field == "GT" else int(other.decoder_info.group)
        assert got_group == want, (case["id"], env, v, got_group)
        got = other.forward(x, poses=case["decoder"])
        for name in C.outputs_of(case):
            assert np.array_equal(got[name], base[name]), (case["id"], env, v, name)
        tried.append(v)
    return groups, tried


SF2_OVERRIDE = [next(c for c in C.V2_CASES if c["group"] == "spread" and (c["d_model"], c["heads"]) == dh) for dh in ((144, 144), (20, 5))]
SFD_OVERRIDE = [c for c in C.DEC_CASES if c["geometry"] in ((17, 12, 32, 4), (18, 24, 64, 8))]


@pytest.mark.parametrize("case", SF2_OVERRIDE, ids=[c["id"] for c in SF2_OVERRIDE])
def test_transformer_row_group_does_not_change_a_bit(case, monkeypatch):
    """MI355_SF2_ROW_GROUP = 1, 2, 4, 8, 16 up to the planned row group (8 for the first case, 16 for the second): every output of
    the n windows equals the default model's bit for bit"""
    groups, tried = _same_bits(case, monkeypatch, "MI355_SF2_ROW_GROUP", (1, 2, 4, 8, 16), "GT", lambda v, g, geo: v if v <= g["GT"] else None)
    assert tried == [v for v in (1, 2, 4, 8, 16) if v <= groups["GT"]] and len(tried) >= 4


@pytest.mark.parametrize("case", SFD_OVERRIDE, ids=[c["id"] for c in SFD_OVERRIDE])
def test_decoder_row_group_does_not_change_a_bit(case, monkeypatch):
    """MI355_SFD_ROW_GROUP = 1, 2, 3, 5, 8 (the engine shrinks a group that does not fit the LDS): the same bits as the default 4"""
    def fitting(v, g, geo):
        while v > 1 and C.lds_decoder(geo, v) > C.LDS_BYTES:
            v -= 1
        return v
    groups, tried = _same_bits(case, monkeypatch, "MI355_SFD_ROW_GROUP", (1, 2, 3, 5, 8), "GD", fitting)
    assert groups["GD"] == 4 and tried == [1, 2, 3, 5, 8]
