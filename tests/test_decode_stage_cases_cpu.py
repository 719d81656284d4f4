"""The case list of test_decode_stages_gpu.py, judged on the CPU: (1) the launches zg_debug_gemv_plan plans for it reach every
model-tier route and every kernel instantiation tests/golden/gemv_plan.json records, or the test names what it cannot reach and
why; (2) the bound the GPU test applies, 3 x Y with Y the float32 numpy evaluation's own error (stage_ref), has teeth: three
emulated defects fed through stage_ref exceed it by 1.5 x at every width, weight type and batch of the list; (3) the score
regimes (score_regimes.py): every regime case meets its regime's conditions in a float64 forward of its own model, the regimes
reach every attention path and cache format the list has, and four emulated attention defects that pass at the old cases' scale
exceed the regime cases' bounds by half."""
import dataclasses
import functools
import json

import numpy as np
import pytest

import score_regimes as rg
import stage_ref as sr
import test_gemv_plan_cpu as gp
from decode_stage_cases import CASES, MODEL_ROUTES, REGIME_CASES, ROUTES, VOCAB, attention_how, attention_operands, instantiation, plan_case

TWO_BITS = "needs two bits of ZGPT2_DECODE_PATHS_OFF at once ({}); the list sets one bit per handle"
NO_WORKSPACE = ("K = 3072 in one slice: a launch without the split-K workspace; the model tier gives every launch its workspace (base_gemv), so "
                "K >= 2048 runs in four slices there — op-tier shapes of the fixture only")
# Instantiations the fixture records that no case of the list reaches, by name, each with its reason.  The test fails when one of
# these IS reached (the entry is stale) as well as when anything else is missed.
UNREACHED = {
    ("mfma16", "GR_MFMA16", 4, 6, 0, 0, 0): TWO_BITS.format("16 line-shaped loads off and 32 wave-per-tile lm_head off: K / 32 = 12 or 24 is the wave-per-tile kernel's otherwise"),
    ("mfma16", "GR_MFMA16", 16, 2, 0, 0, 0): TWO_BITS.format("1 planes off and 16 line-shaped loads off, K <= 1024"),
    ("mfma16", "GR_MFMA16", 16, 2, 0, 1, 0): TWO_BITS.format("2 four-wave Linear off and 16 line-shaped loads off, K <= 1024"),
    ("mfma16", "GR_MFMA16_KS", 16, 2, 0, 0, 0): TWO_BITS.format("1 planes off and 16 line-shaped loads off, K = 3072 / 4096 in four slices"),
    ("mfma16", "GR_MFMA16_KS", 16, 2, 0, 1, 0): TWO_BITS.format("2 four-wave Linear off and 16 line-shaped loads off, K = 3072 / 4096 in four slices"),
    ("mfma16", "GR_MFMA16", 16, 6, 0, 0, 1): NO_WORKSPACE,
    ("mfma16", "GR_MFMA16", 16, 6, 0, 1, 0): NO_WORKSPACE,
    ("mfma16", "GR_MFMA16", 16, 6, 1, 1, 0): NO_WORKSPACE,
}


def test_the_case_list_is_a_few_dozen_distinct_cases():
    assert 24 <= len(CASES) <= 64
    assert len({c.id for c in CASES}) == len(CASES)
    assert {c.E for c in CASES} == {128, 384, 768, 1024, 1280, 1600, 2048}
    assert {c.batch for c in CASES} >= {1, 2, 3, 5, 8}
    assert {c.wt for c in CASES} == {"bf16", "f32", "b24"} and {c.kv for c in CASES} == {"f32", "f16", "b24"}
    assert {c.off for c in CASES} == {0, 1, 2, 4, 8, 16, 32, 64}
    assert {c.seq_len for c in CASES if c.ctx == 320} == {1, 256, 257, 320}
    assert VOCAB % 16 != 0
    for c in CASES:  # wide models: one layer, one short context
        assert c.E <= 384 or (c.layers == 1 and c.ctx == 64), c.id


def test_the_list_reaches_every_model_route_and_every_recorded_instantiation():
    gold = json.load(open(gp.GOLDEN))
    recorded = set()
    for p in gold["plans"]:
        p = dict(zip(gp.FIELDS, p))
        if p["supported"] and ROUTES[p["route"]] in MODEL_ROUTES:
            recorded.update(instantiation(p))
    routes, reached, modes_seen = set(), {}, set()
    for c in CASES:
        modes, plans = plan_case(c)
        modes_seen.add(tuple(sorted(modes.items())))
        for cls, p in plans.items():
            assert p["supported"], (c.id, cls)
            routes.add(ROUTES[p["route"]])
            for k in instantiation(p):
                reached.setdefault(k, (c.id, cls))
    assert routes >= set(MODEL_ROUTES), set(MODEL_ROUTES) - routes
    missed = recorded - set(reached)
    assert missed == set(UNREACHED), {"missed and not named": missed - set(UNREACHED), "named but reached": {k: reached[k] for k in set(UNREACHED) & set(reached)}}
    # what the issue of this test lists by name
    assert {k[1] for k in reached if k[0] == "mt"} == {1, 2, 4, 8}
    assert {k[1] for k in reached if k[0] == "steps"} == {12, 24, 32}
    assert {k[2] for k in reached if k[:2] == ("pairs", "GR_PL4")} == {1, 2, 3, 4, 5}
    # every combination of the decode modes a handle can be in
    want_modes = {(0, 0, 0, 0), (0, 0, 0, 1), (1, 0, 0, 0), (1, 0, 1, 0), (1, 1, 0, 0), (1, 1, 1, 0)}  # (planes, stats, tags, fused)
    got_modes = {(m["planes"], m["stats"], m["tags"], m["fused"]) for m in map(dict, modes_seen)}
    assert got_modes >= want_modes, want_modes - got_modes


def defect_figures(E, wt, M, seed):
    """For the Linears of a Block of width E (N x K: 3E x E behind a LayerNorm, E x E, E x 4E) with weights stored as wt and M
    input rows: the yardstick Y and what the three emulated defects measure, all in stage_ref's metric."""
    rng = np.random.default_rng(seed)
    out = []
    for N, K, ln in ((3 * E, E, True), (E, E, False), (E, 4 * E, False)):
        w = (rng.standard_normal((N, K), dtype=np.float32) * np.float32(0.02)).astype(np.float32)
        if wt == "bf16":
            w = sr.round_bf16(w)
        W = sr.stored_matrix(w, wt)
        bias = rng.standard_normal(N, dtype=np.float32) * np.float32(0.02)
        x = rng.standard_normal((M, K), dtype=np.float32)
        lnp = (np.float32(1) + rng.standard_normal(K, dtype=np.float32) * np.float32(0.02), rng.standard_normal(K, dtype=np.float32) * np.float32(0.02)) if ln else None
        ref, s, y32 = sr.linear_stage(x, W, bias, ln=lnp)
        fig = {"N": N, "K": K, "Y": sr.metric(y32, ref, s)}
        # (a) the activations the Linear multiplies, cut to two of their three bf16 planes
        a = (sr.layernorm(x, lnp[0], lnp[1]) if ln else x).astype(np.float32)
        two = sr.split3(a)[:2].astype(np.float64).sum(axis=0)
        fig["two planes"] = sr.metric(sr.linear(two, W, bias), sr.linear(a, W, bias), sr.linear_scale(a, W, bias))
        # (b) fp32 / B24 weights cut to bf16
        if wt != "bf16":
            fig["bf16 weights"] = sr.metric(sr.linear_stage(x, sr.round_bf16(W), bias, ln=lnp)[0], ref, s)
        # (c) an fp32 K / V row (an output of ln_1 + c_attn) rounded to fp16
        if ln:
            fig["fp16 row"] = sr.metric(sr.store_kv(ref[:, E:].astype(np.float32), "f16"), ref[:, E:].astype(np.float32).astype(np.float64), s[:, E:])
        out.append(fig)
    # lm_head as the model has it: wte both embeds the token and scores it, so a sequence's own logit is a sum of like-signed
    # products.  Both sides of the GPU test's lm_head check are measured with four ulp of the logit granted (stage_ref.LOGIT_ULPS): so is this.
    wte = sr.stored_matrix(sr.round_bf16(rng.standard_normal((VOCAB, E), dtype=np.float32) * np.float32(0.02)) if wt == "bf16" else
                           rng.standard_normal((VOCAB, E), dtype=np.float32) * np.float32(0.02), wt)
    x = wte[:M] + sr.round_bf16(rng.standard_normal((M, E), dtype=np.float32) * np.float32(0.02))
    lnp = (np.float32(1) + rng.standard_normal(E, dtype=np.float32) * np.float32(0.02), rng.standard_normal(E, dtype=np.float32) * np.float32(0.02))
    ref, s, y32 = sr.linear_stage(x, wte, None, ln=lnp)
    granted = lambda got: sr.metric_granted(got, ref, s, sr.LOGIT_ULPS)
    fig = {"N": VOCAB, "K": E, "Y": granted(y32), "Y, plain metric": sr.metric(y32, ref, s), "largest |logit| / s": float(np.max(np.abs(ref) / s))}
    a = sr.layernorm(x, lnp[0], lnp[1]).astype(np.float32)
    two = sr.split3(a)[:2].astype(np.float64).sum(axis=0)
    fig["two planes"] = granted(sr.linear(two, wte) + (ref - sr.linear(a, wte)))
    if wt != "bf16":
        fig["bf16 weights"] = granted(sr.linear_stage(x, sr.round_bf16(wte), None, ln=lnp)[0])
    out.append(fig)
    return out


@pytest.mark.parametrize("E,wt", sorted({(c.E, c.wt) for c in CASES}))
def test_three_defects_exceed_the_bound_by_half(E, wt):
    """BOUND_Y x Y (3, or what stage_ref.BOUND_Y names for a route) is the GPU test's bound.  Every defect must measure at least
    1.5 x that, on every Linear shape of the width, at the smallest and the largest batch of the list at this width and weight
    type, under the widest bound any case of that width, type and batch is given for the launch."""
    mine = [c for c in CASES if (c.E, c.wt) == (E, wt)]
    for M in sorted({min(c.batch for c in mine), max(c.batch for c in mine)}):
        plans = [plan_case(c)[1] for c in mine if c.batch == M]
        factor = {cls: max(sr.bound_y(ROUTES[p[cls]["route"]]) for p in plans) for cls in (1, 3, 5, 6)}
        for cls, fig in zip((1, 3, 5, 6), defect_figures(E, wt, M, seed=E + M)):
            for name in ("two planes", "bf16 weights", "fp16 row"):
                if name in fig:
                    bound = factor[cls] * fig["Y"]
                    print(f"E {E} {wt} M {M} {fig['N']}x{fig['K']}: Y {fig['Y']:.2e}  {name} {fig[name]:.2e}  ({fig[name] / bound:.1f} x the bound of {factor[cls]:.0f} Y)")
                    assert fig[name] >= 1.5 * bound, (E, wt, M, fig)


# ---------------------------------------------------------------------------------------------- the score regimes (score_regimes.py)
# What the cases above cannot see, printed by the teeth test below at each regime case's shape with N(0, 0.02) weights (score spread
# 0.1 .. 0.4, E 768: 1.5): the query cut to two planes measures 0.08 .. 0.90 x the 3 Y bound, a maximum started at 0 and a merge
# relative to the first split 0.05 .. 0.39 x, the unbroken emulation's own figure — all pass; scores rounded to 16 mantissa bits
# 0.05 .. 0.6 x at E 128 and 1.5 / 4.2 x at E 768, the one defect of the four that the widest of those cases could see.
@functools.lru_cache(maxsize=None)
def regime_teeth(case):
    q, K, V, past = attention_operands(case)
    return rg.teeth(case.id, case.regime, q, K, V, past, 256)


def test_the_regime_cases_are_new_cases_beside_an_unchanged_list():
    assert all(c.regime == "" for c in CASES) and all(rg.parse(c.regime)[0] for c in REGIME_CASES)
    ids = [c.id for c in CASES + REGIME_CASES]
    assert len(set(ids)) == len(ids) and len(REGIME_CASES) <= 48
    assert all(c.layers == 1 and c.wt == "bf16" and c.id.endswith("-" + c.regime) for c in REGIME_CASES)
    for c in REGIME_CASES:  # one-key: the hot position is a cached one or the row the step appends
        hot = rg.parse(c.regime)[1]
        assert hot is None or 0 <= hot < c.seq_len, c.id


@pytest.mark.parametrize("case", REGIME_CASES, ids=lambda c: c.id)
def test_a_regime_case_meets_its_regimes_conditions_in_float64(case):
    q, K, V, past = attention_operands(case)
    sc = rg.scores(q, K, past)
    print(f"REGIME {case.id}: {rg.describe(sc)}")
    assert rg.conditions(case.regime, sc, past) == []
    if case.regime == "trained":
        q, K, V = (t.astype(np.float32) for t in (q, K, V))
        ref, s = sr.causal_attention(q, K, V, past)
        Y = sr.metric(sr.causal_attention(q, K, V, past, np.float32)[0], ref, s)
        assert Y >= rg.Y_FLOOR, (case.id, Y)


def test_the_regimes_reach_every_attention_path():
    seen = {}
    for c in REGIME_CASES:
        modes, _ = plan_case(c)
        seen.setdefault(rg.parse(c.regime)[0], set()).add((attention_how(c, modes), c.kv, c.batch == 1))
    hows = {attention_how(c) for c in CASES}
    assert len(hows) == 5 and {h for h in hows if "two-pass" in h} and {h for h in hows if "fused" in h}, hows
    for name in ("trained", "one-key"):
        assert {h for h, _, _ in seen[name]} == hows, (name, hows - {h for h, _, _ in seen[name]})
        assert {(kv, one) for _, kv, one in seen[name]} >= {(kv, one) for kv in ("f16", "b24") for one in (True, False)}, name
    far = {h for h, _, _ in seen["far-below"]}
    assert any("fused" in h for h in far) and any("merged by its last split" in h for h in far) and any(h.endswith("merged in float64") for h in far), far
    # one-key: every hot position the fused launch has at each T, and the first and the last of six splits under both two-pass cases
    hot = lambda pick: {(c.seq_len, rg.parse(c.regime)[1]) for c in REGIME_CASES if rg.parse(c.regime)[0] == "one-key" and pick(c)}
    assert hot(lambda c: plan_case(c)[0]["fused"]) == {(6, 0), (6, 5), (257, 0), (257, 255), (257, 256), (320, 0), (320, 255), (320, 256), (320, 319)}
    for batch in (1, 2):
        assert hot(lambda c: c.seq_len == 1300 and c.batch == batch) == {(1300, 3), (1300, 1290)}


@pytest.mark.parametrize("case", REGIME_CASES, ids=lambda c: c.id)
def test_the_regime_bounds_have_teeth(case):
    """Under `trained` the query cut to two planes and scores of 16 mantissa bits exceed 3 Y by half at every width and T of the
    list; under far-below a maximum started at 0 does (it returns 0 / 0).  The same defects at the case's shape with today's
    N(0, 0.02) weights are printed beside them."""
    bites = regime_teeth(case)
    name = rg.parse(case.regime)[0]
    if name == "trained":
        regime_teeth(dataclasses.replace(case, regime=""))
        assert bites["two planes"] and bites["scores b24"], (case.id, bites)
    elif name == "far-below":
        assert bites["max from 0"], (case.id, bites)


def test_every_emulated_defect_exceeds_its_bound_in_some_regime():
    by_regime = {}
    for c in REGIME_CASES:
        for d, hit in regime_teeth(c).items():
            if hit:
                by_regime.setdefault(d, set()).add(rg.parse(c.regime)[0])
    assert set(by_regime) == set(rg.DEFECTS), by_regime
    assert "one-key" in by_regime["merge from first"]  # exp(m_s - m_first) overflows where the hot key sits in a later split
