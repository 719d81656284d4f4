"""The case list of test_pass_stages_gpu.py, judged on the CPU: (1) the launches zg_debug_prefill_plan plans for it reach both GEMM
families and the fp32-weight three-pass kernel for every Linear role, the K slices, tails, plane counts, the stream-K hand-over,
the row counts around the tiles and every attention path the issue of this test lists — or the test names what a model-level
pass cannot reach within these sizes and why; (2) no case exceeds the row budget that keeps its float64 references to a few
seconds; (3) the bound the GPU test applies, 3 x Y with Y the float32 numpy evaluation's own error (stage_ref), has teeth: five
emulated defects measured in the same metric exceed it by 1.5 x at the list's widths, weight types and smallest and largest M;
(4) the score regimes (score_regimes.py): every regime case meets its regime's conditions in a float64 forward of its own model,
the regimes reach every attention kernel, range count and cache format, and emulated attention defects that pass at the old
cases' scale exceed the regime cases' bounds by half."""
import dataclasses
import functools
import time

import numpy as np
import pytest

import score_regimes as rg
import stage_ref as sr
from pass_stage_cases import (CASES, REGIME_CASES, VOCAB, attention_how, attention_operands, attention_plan, first_range_last_key, outcome, pass_route,
                              plan_case)

ROLES = ("c_attn", "attn c_proj", "c_fc", "mlp c_proj")
# What test_prefill_plan_cpu.py's table holds that a model-level pass cannot reach within the row budget, each with its reason.
# The test fails when one of these IS reached (the entry is stale).
UNREACHED = {
    "ns = 2": "the 128 x 256 tiles need at least 256 of them: M >= 4096 at N = 12 x 256 columns and beyond; test_prefill_linear_gpu.py runs one",
    "REDUCE_LN_SPLIT": "the reduce kernel followed by a separate LayerNorm needs N = n_embed > 2048",
    "T128 whole mlp c_proj": "K = 4 n_embed >= 512 is sliced unless the grid has 129 tiles or more: M > 8192 at n_embed = 128",
}


def planned():
    out = []
    for c in CASES:
        plans, att = plan_case(c)
        for cls, l, role, p in plans:
            assert p["status"] == 0, (c.id, role, p)
            out.append((c, role, p, outcome(role, p)))
    return out


def test_the_case_list_is_a_few_dozen_distinct_cases_within_the_row_budget():
    assert 24 <= len(CASES) <= 48
    assert len({c.id for c in CASES}) == len(CASES)
    assert VOCAB // 64 * 64 == 320 and VOCAB % 64 == 13
    for c in CASES:
        assert c.M <= 1024 and c.past + c.n <= c.context, c.id
        assert c.layers == 1 or c.M * c.E <= 400_000, c.id
        assert c.E <= 384 or c.M <= 136, c.id  # wide models: few rows (their yardstick runs row by row over all of them)
        assert not (c.score and not c.logits), c.id


def test_the_list_reaches_what_the_issue_lists():
    rows = planned()
    seen = {(role, o) for _, role, _, o in rows}
    fam = lambda role, name: {o for r, o in seen if r == role and o[0] == name}
    # both GEMM families and the three-pass kernel for every Linear role, at E 128 / 384 / 768 under pins 1 and 2
    for role in ROLES:
        for name in ("S4", "T128", "T128_WP"):
            assert fam(role, name), (role, name)
        for E in (128, 384, 768):
            for pin, name in ((1, "S4"), (2, "T128")):
                assert any(c.E == E and c.pin[0] == pin and r == role and o[0] == name for c, r, _, o in rows if c.wt == "bf16"), (role, E, pin)
    assert any(c.E == 1600 and o[0] == "S4" and r == "c_attn" and p["grid_x"] == 25 for c, r, p, o in rows)  # 1 x 25 tiles of 192 columns: 4800 = 24.x
    assert {c.E for c in CASES} == {128, 384, 768, 1600}
    # fp32 / B24 weights on the persistent kernel too
    assert {c.wt for c, r, _, o in rows if o[0] == "S4" and c.wt != "bf16"} == {"f32", "b24"}
    # both 128-row kernels (whole and through the workspace) with 2 and 3 planes
    assert {(o[1], o[3]) for r, o in seen if o[0] == "T128"} == {("whole", 2), ("whole", 3), ("partial", 2), ("partial", 3)}
    # the persistent kernel's K slices, and two planes on it
    assert {o[3] for r, o in seen if o[0] == "S4" and o[1] == 1} == {1, 2, 3, 4}
    assert any(c.planes == 2 and o[0] == "S4" for c, _, _, o in rows)
    # every tail a model can reach
    assert {o[4] for _, o in seen} == {"NO_TAIL", "LN_SPLIT", "REDUCE", "REDUCE_RESID_LN"}
    for name in ("S4", "T128", "T128_WP"):
        assert {o[4] for r, o in seen if o[0] == name and r == "mlp c_proj"} >= {"REDUCE", "REDUCE_RESID_LN"}, name
    # the stream-K hand-over of c_attn: 24 tiles on 16 workgroups, twice on one handle
    sk = [(c, p) for c, r, p, o in rows if r == "c_attn" and o[0] == "S4" and o[2] == 1]
    assert [(c.E, c.M, c.wgs, c.twice, p["grid_x"]) for c, p in sk] == [(384, 1024, 16, True, 16)]
    # what cannot be reached stays unreached
    assert not any(o[0] != "S4" and o[2] == 2 for _, o in seen), UNREACHED["ns = 2"]
    assert "REDUCE_LN_SPLIT" not in {o[4] for _, o in seen}, UNREACHED["REDUCE_LN_SPLIT"]
    assert not any(r == "mlp c_proj" and o[:2] == ("T128", "whole") for r, o in seen), UNREACHED["T128 whole mlp c_proj"]
    # rows around the tiles, a sequence boundary inside a tile wherever M has a divisor
    assert {c.M for c in CASES} >= {1, 127, 128, 129, 255, 256, 257}
    assert all(any(c.M == M and c.batch > 1 for c in CASES) for M in (128, 129, 255, 256))
    # attention: one range, split ranges + merge, continuations on each format (n = 1 and the end of the context among them),
    # whole prompts on the 16- and 24-bit caches (the qkv columns are read)
    att = [(c, plan_case(c)[1]) for c in CASES]
    assert any(a[0] == 0 and a[2] == 1 and c.n <= 128 for c, a in att)
    assert any(a[0] == 0 and a[2] > 1 and 129 <= c.n <= 320 and c.heads <= 2 and a[1] == 4 for c, a in att)
    assert {a[0] for c, a in att if c.past > 0} == {1, 2, 3}
    assert {c.kv for c, a in att if c.past > 0 and a[2] > 1} >= {"f32", "f16"}
    assert any(c.past > 0 and c.n == 1 and c.past + 1 == c.context for c in CASES)
    assert {c.kv for c in CASES if c.past > 0 and c.past + c.n == c.context} >= {"f16", "b24"}
    assert {c.kv for c in CASES if c.past == 0 and c.kv != "f32"} == {"f16", "b24"}
    # score: below a block and crossing one (2 x 130 rows), on each weight type; one pass that stops behind its last append
    assert any(c.score and c.M < 256 for c in CASES) and any(c.score and c.batch == 2 and c.n == 130 for c in CASES)
    assert {c.wt for c in CASES if c.score} == {"bf16", "f32", "b24"}
    assert any(not c.logits for c in CASES) and sum(c.planes == 2 for c in CASES) >= 1


def defect_figures(E, wt, M, n_seq, seed, lm_head):
    """For the Linears of a Block of width E with weights stored as wt and M input rows, and for the attention of n_seq new
    positions: the yardstick Y and what the emulated defects measure, all in stage_ref's metric."""
    rng = np.random.default_rng(seed)
    out = []
    for role, N, K, resid, act in (("c_attn", 3 * E, E, False, None), ("attn c_proj", E, E, True, None), ("c_fc", 4 * E, E, False, "gelu"),
                                   ("mlp c_proj", E, 4 * E, True, None)):
        w = rng.standard_normal((N, K), dtype=np.float32) * np.float32(0.02)
        W = sr.stored_matrix(sr.round_bf16(w) if wt == "bf16" else w, wt)
        bias = rng.standard_normal(N, dtype=np.float32) * np.float32(0.02)
        a = rng.standard_normal((M, K), dtype=np.float32)
        a = sr.gelu(a, np.float32) if role == "mlp c_proj" else a
        r = rng.standard_normal((M, N), dtype=np.float32) if resid else None
        ref, s, Y = sr.pass_linear_stage(a, W, bias, resid=r, act=act, n_seq=n_seq)
        fig = {"role": role, "N": N, "K": K, "Y": Y}
        two = sr.split3(a)[:2].astype(np.float64).sum(axis=0)
        fig["two planes"] = sr.metric(sr.pass_linear_stage(two, W, bias, resid=r, act=act, yardstick=False)[0], ref, s)
        if wt != "bf16":
            fig["bf16 weights"] = sr.metric(sr.pass_linear_stage(a, sr.round_bf16(W), bias, resid=r, act=act, yardstick=False)[0], ref, s)
        if role == "c_attn":
            kv = ref[:, E:].astype(np.float32)
            fig["fp16 row"] = sr.metric(sr.store_kv(kv, "f16"), kv.astype(np.float64), s[:, E:])
        if resid:  # the last of four K slabs of the sliced sum left out
            cut = K - K // 4
            fig["a K slab left out"] = sr.metric(sr.pass_linear_stage(a[:, :cut], W[:, :cut], bias, resid=r, yardstick=False)[0], ref, s)
        out.append(fig)
    if lm_head:  # wte both embeds and scores: both sides with four ulp of the logit granted, as the GPU test measures it
        wte = rng.standard_normal((VOCAB, E), dtype=np.float32) * np.float32(0.02)
        wte = sr.stored_matrix(sr.round_bf16(wte) if wt == "bf16" else wte, wt)
        Mh = min(M, 64)
        x = wte[np.arange(Mh) % VOCAB] + sr.round_bf16(rng.standard_normal((Mh, E), dtype=np.float32) * np.float32(0.02))
        g, b = np.float32(1) + rng.standard_normal(E, dtype=np.float32) * np.float32(0.02), rng.standard_normal(E, dtype=np.float32) * np.float32(0.02)
        a = sr.layernorm(x, g, b).astype(np.float32)
        ref, s, y32 = sr.linear_stage(a, wte, None)
        granted = lambda got: sr.metric_granted(got, ref, s, sr.LOGIT_ULPS)
        fig = {"role": "lm_head", "N": VOCAB, "K": E, "Y": granted(y32)}
        fig["two planes"] = granted(sr.linear(sr.split3(a)[:2].astype(np.float64).sum(axis=0), wte))
        if wt != "bf16":
            fig["bf16 weights"] = granted(sr.linear(a, sr.round_bf16(wte)))
        out.append(fig)
    # attention: n_seq (8 at the least, 96 at the most) new positions behind 40 cached ones, two heads; the mask off by one key in either direction
    n = min(max(n_seq, 8), 96)
    q, K_, V_ = (rng.standard_normal((1, 2, t, 64), dtype=np.float32) for t in (n, 40 + n, 40 + n))
    ref, s = sr.causal_attention(q, K_, V_, 40)
    fig = {"role": "attention", "N": n, "K": 40 + n, "Y": sr.metric(sr.causal_attention(q, K_, V_, 40, np.float32)[0], ref, s)}
    fig["mask one key short"] = sr.metric(sr.causal_attention(q, K_, V_, 40, shift=-1)[0], ref, s)
    fig["mask one key long"] = sr.metric(sr.causal_attention(q, K_, V_, 40, shift=1)[0][:, :, :-1], ref[:, :, :-1], s[:, :, :-1])
    out.append(fig)
    return out


DEFECTS = ("two planes", "bf16 weights", "fp16 row", "a K slab left out", "mask one key short", "mask one key long")


@pytest.mark.parametrize("E,wt", sorted({(c.E, c.wt) for c in CASES}))
def test_the_defects_exceed_the_bound_by_half(E, wt):
    """BOUND_Y x Y (3 unless stage_ref.BOUND_Y names a route) is the GPU test's bound.  Every defect must measure at least 1.5 x
    that on every Linear role of the width, at the smallest and the largest M of the list at this width and weight type."""
    mine = [c for c in CASES if (c.E, c.wt) == (E, wt)]
    t0 = time.perf_counter()
    for c in sorted({min(mine, key=lambda c: c.M), max(mine, key=lambda c: c.M)}, key=lambda c: c.M):
        factor = {}
        for cls, l, role, p in plan_case(c)[0]:
            role = role.split(" strip")[0]
            factor[role] = max(factor.get(role, 3.0), sr.bound_y(pass_route(p)))
        for fig in defect_figures(E, wt, c.M, c.n, seed=E + c.M, lm_head=any(m.score for m in mine)):
            f = factor.get(fig["role"], 3.0)
            for name in DEFECTS:
                if name in fig:
                    bound = f * fig["Y"]
                    print(f"E {E} {wt} M {c.M} {fig['role']} {fig['N']}x{fig['K']}: Y {fig['Y']:.2e}  {name} {fig[name]:.2e}  ({fig[name] / bound:.1f} x the bound of {f:.0f} Y)")
                    assert fig[name] >= 1.5 * bound, (E, wt, c.M, fig)
    assert time.perf_counter() - t0 < 60, "the references of one width must stay quick"


# ---------------------------------------------------------------------------------------------- the score regimes (score_regimes.py)
# What the cases above cannot see, printed by the teeth test below at each regime case's shape with N(0, 0.02) weights: the query
# cut to two planes — the product the six plane products exist for — measures 0.12 .. 0.49 x the 3 Y bound, scores rounded to 16
# mantissa bits 0.14 .. 0.5 x at E 128 and 1.2 x at E 384, a maximum started at 0 and a merge relative to the first range
# 0.13 .. 0.38 x, the unbroken emulation's own figure: all of them pass, or fall short of the margin of a half.
@functools.lru_cache(maxsize=None)
def regime_teeth(case):
    q, K, V, past = attention_operands(case)
    return rg.teeth(case.id, case.regime, q, K, V, past, 32 * attention_plan(case)[1], wide=sr.bound_y("PF_ATTN_WIDE"))


def test_the_regime_cases_are_new_cases_beside_an_unchanged_list():
    assert all(c.regime == "" for c in CASES) and all(rg.parse(c.regime)[0] for c in REGIME_CASES)
    ids = [c.id for c in CASES + REGIME_CASES]
    assert len(set(ids)) == len(ids) and len(REGIME_CASES) <= 32
    for c in REGIME_CASES:
        assert c.layers == 1 and c.wt == "bf16" and c.planes == 3 and c.id.endswith("-" + c.regime) and c.M <= 512, c.id
        hot = rg.parse(c.regime)[1]
        assert hot is None or 0 <= hot < c.past + c.n - 1, c.id  # one-key: a position some query of the pass looks back at


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
        seen.setdefault(rg.parse(c.regime)[0], set()).add((attention_how(c).split(",")[0] + (", merged" if attention_plan(c)[2] > 1 else ", one range"), c.kv))
    # the whole-prompt kernel with one range and with ranges merged; the continuation kernel per cache format, one range and merged
    want = {("whole-prompt kernel, one range", "f32"), ("whole-prompt kernel, merged", "f32"), ("continuation kernel, merged", "f32"),
            ("continuation kernel, one range", "f16"), ("continuation kernel, merged", "f16"), ("continuation kernel, one range", "b24")}
    for name in ("trained", "one-key"):
        assert seen[name] >= want, (name, want - seen[name])
    assert seen["far-below"]
    # one-key: the sink every row looks at, the last key of the first key range (whole prompt and continuation), a key among the cached ones
    hot = [(c, rg.parse(c.regime)[1]) for c in REGIME_CASES if rg.parse(c.regime)[0] == "one-key"]
    assert any(h == 0 and c.past == 0 for c, h in hot) and any(0 < h < c.past for c, h in hot)
    assert {c.past > 0 for c, h in hot if h == first_range_last_key(c) and attention_plan(c)[2] > 1} == {False, True}
    # six heads under each route pin
    assert {c.pin[0] for c in REGIME_CASES if c.E == 384 and c.regime == "trained"} == {1, 2}


@pytest.mark.parametrize("case", REGIME_CASES, ids=lambda c: c.id)
def test_the_regime_bounds_have_teeth(case):
    """Under `trained` the query cut to two planes and scores of 16 mantissa bits exceed the bound — 6 Y, stage_ref.BOUND_Y's
    PF_ATTN_WIDE — by half at every width and shape of the list; under far-below a maximum started at 0 does.  The same defects at the case's shape with today's N(0, 0.02) weights
    are printed beside them."""
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
    assert "one-key" in by_regime["merge from first"]  # exp(m_s - m_first) overflows where the hot key sits in a later key range
