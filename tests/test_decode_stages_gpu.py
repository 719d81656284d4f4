"""Every kernel hand-over of one decode step against float64, stage by stage.

A tapped step (zg_debug_gpt_step_taps) returns what each launch class wrote.  Each stage's float64 reference (stage_ref) is
computed from the input the DEVICE gave that stage, so nothing compounds over layers and a failure names its launch.  Metric of
a Linear: per output |got - ref64| / s, s = sqrt(sum_k (a_k w_nk)^2) + |bias_n| + |resid_n|; of the attention: s = the l2 norm of
the weighted V terms.  Bound: 3 x Y, Y = the same metric for a float32 numpy evaluation (float32 LayerNorm, blocked float32 `@`)
of the same stage from the same tapped input — computed here, from the reference side alone.  K / V rows appended to a 16- or
24-bit cache get half an ulp of that format on top (stage_ref.HALF_ULP); every other cache position must keep the prefill's
bits.  Planes are held to the exactness they claim (a valid three-term split; 1 ulp of fp32 against gain * x), the tile
statistics to the worst-case rounding of a 16-term fp32 sum (stage_ref.STATS_BOUND), the token to the lowest index of the
maximum of the tapped logits (include/zgpt2.h: "lowest index wins ties"), and the tapped logits to bit-equality with
zg_gpt_forward on a twin handle.  The cases and what the library plans for them: decode_stage_cases.py; that the list reaches
every route, and that 3 x Y has teeth against three emulated defects: test_decode_stage_cases_cpu.py.

Measured on one MI355X (59 cases, every case under 0.8 s; lm_head rows with four ulp of the logit granted, see below):

| route / check | checks | Y min .. max | kernel worst | worst / Y |
|---|---|---|---|---|
| GR_VALU | 82 | 6.0e-08 .. 8.7e-07 | 9.6e-07 | 1.56 |
| GR_VALU_GROUPS (mlp c_proj, fp32 weights, E 1600 x 5 rows) | 1 | 6.7e-07 | 6.9e-07 | 1.03 |
| GR_KSPLIT | 30 | 5.3e-08 .. 5.8e-07 | 3.9e-07 | 1.60 |
| GR_LNK | 34 | 2.2e-07 .. 6.8e-07 | 9.0e-07 | 1.72 |
| GR_LNK in the fused batch-1 launch | 18 | 2.3e-07 .. 7.2e-07 | 8.4e-07 | 1.60 |
| GR_MFMA16 | 66 | 1.1e-07 .. 8.9e-07 | 9.8e-07 | 2.30 |
| GR_MFMA16_KS | 10 | 4.3e-07 .. 7.7e-07 | 5.9e-07 | 0.84 |
| GR_PL4 | 98 | 9.4e-08 .. 8.2e-07 | 1.1e-06 | 1.71 |
| GR_PL4_KS | 13 | 4.1e-07 .. 6.8e-07 | 5.9e-07 | 0.99 |
| GR_LM_WPT (bound 6 Y) | 11 | 2.7e-07 .. 3.6e-07 | 1.1e-06 | 3.69 |
| attention, partials merged in float64 (also the fused launch) | 40 | 2.3e-07 .. 8.1e-06 | 2.2e-06 | 1.15 |
| attention, merged by its last split, tagged | 33 | 2.9e-07 .. 1.1e-05 | 2.5e-06 | 1.35 |
| attention, merged by its last split, tickets | 3 | 4.0e-07 .. 3.4e-06 | 1.0e-06 | 0.95 |
| planes against float32(gain * x), in ulp (bound 1) | 72 | | 0.50 | |
| tile statistics (bound 3.8e-06) | 46 | | 4.2e-07 | |

The attention again under the score regimes of score_regimes.py (41 one-layer cases beside those above, 3.2 s together; the
cases above have scores +-0.05 .. 0.3 wide, exp(s - m) = 1 to within a third): `trained` — q and k rows times a power of two,
every head's float64 score spread in [8, 60] — under the rule above; one-key@P — position P holds 1 - 2^-24 of head 0's mass or
more — and far-below — every score of head 0 under -104 — with 8 ulp of the output granted on both sides for head 0
(stage_ref.ATTN_ULPS: Y is 0 where one key has all the mass) and the rule above for the other heads.  Every case re-asserts its
regime from the tapped q and cache and prints spread and largest probability.  Measured on the same MI355X:

| how | regime | checks | Y min .. max | kernel worst | worst / Y |
|---|---|---|---|---|---|
| partials merged in float64, fused launch | trained | 4 | 3.3e-07 .. 2.7e-06 | 2.3e-06 | 1.54 |
| partials merged in float64, fused launch | one-key, head 0 (hot 0, 5, 255, 256, 319 = the appended row) | 9 | 0 | 0 beyond the grant | |
| partials merged in float64, fused launch | far-below, head 0 | 3 | 3.6e-06 .. 1.5e-05 | 1.3e-05 | 1.22 |
| partials merged in float64 (off 64; fp16 / B24 cache) | trained | 3 | 1.2e-06 .. 1.7e-06 | 1.2e-06 | 0.91 |
| partials merged in float64 (off 64; fp16 / B24 cache) | one-key, head 0 | 3 | 0 | 0 beyond the grant | |
| partials merged in float64 (off 64) | far-below, head 0 | 1 | 1.1e-06 | 0 beyond the grant | 0.00 |
| partials, six splits, attn c_proj's two-pass merge behind | trained | 2 | 2.4e-06 .. 3.7e-06 | 2.1e-06 | 0.62 |
| partials, six splits, attn c_proj's two-pass merge behind | one-key, head 0 (hot 3 and 1290) | 4 | 0 | 0 beyond the grant | |
| merged by its last split, tagged (fp32, fp16, B24 cache) | trained | 5 | 1.2e-06 .. 2.8e-06 | 2.8e-06 | 1.60 |
| merged by its last split, tagged | one-key, head 0 | 4 | 0 | 0 beyond the grant | |
| merged by its last split, tagged | far-below, head 0 | 1 | 3.4e-06 | 4.3e-06 | 1.27 |
| merged by its last split, tickets | trained | 1 | 2.3e-06 | 1.4e-06 | 0.60 |
| merged by its last split, tickets | one-key, head 0 | 1 | 0 | 0 beyond the grant | |
| the heads a one-key / far-below case leaves alone, all of the above | | 26 | 1.8e-07 .. 1.6e-05 | 2.8e-06 | 1.03 |

attn c_proj behind them (the consumer-side merges, GR_VALU / GR_KSPLIT / GR_PL4 rows above) stayed within its 3 Y in all 41.
On the CPU (test_decode_stage_cases_cpu.py) a float32 emulation of a split kernel passes these bounds, and broken in four ways
it does not: the query cut to two planes 1.9 .. 8.6 x and scores of 16 mantissa bits 7 .. 47 x the 3 Y bound under `trained` at
every width and T (at the scale of the cases above 0.08 .. 0.9 x: passes, and 0.05 .. 0.6 x, E 768 1.5 / 4.2 x), a running maximum started at 0
returns 0 / 0 under far-below, a merge weighted by exp(m_s - m of the first split) overflows under one-key with the hot key in
a later split.

Emulated defects in the same metric (CPU, every width, weight type, smallest and largest batch; Y there 2.0e-07 .. 1.2e-06):
activations cut to two planes 6.2e-06 .. 1.0e-05 (least 2.8 x its bound), an fp32 K / V row rounded to fp16 7.8e-04 .. 1.5e-03
(least 315 x), fp32 / B24 weights cut to bf16 4.5e-03 .. 6.7e-03 (least 2670 x).

Findings, none of them a wrong result:
- lm_head: wte both embeds and scores, so a sequence's own logit is a sum of like-signed products, |logit| up to 18.5 s, and
  is off by ulps of the logit (kernels up to 2.8, the yardstick 1.2), which the metric's l2 norm does not cover and which
  inflated Y until a lost plane passed.  Both sides grant four ulp of the logit (stage_ref.LOGIT_ULPS).
- GR_LM_WPT: one of 11 launches at 3.69 Y on an ordinary logit: two sequential chains of 48 matrix-core accumulations at
  K = 1024.  Bound 6 Y for that route (stage_ref.BOUND_Y); the defects still clear it by 1.5 x (asserted on the CPU).
- embed: its planes split the EXACT product gain * x (the compiler fuses the multiply into the remainder's subtraction), so in
  all 29 plane cases some sums carry more than 24 bits; they are within half an ulp of float32(gain * x), and a valid split.
- mlp c_proj with fp32 weights at E = 1600 x 5 rows runs as GR_VALU_GROUPS: that route is not op-tier only.
- The score regimes: no decode attention path is off by more than 1.6 Y with scores tens of units wide, and with one key
  holding all the mass every path returns V's row to within the grant — the fused launch's wave for row T - 1, the merges by
  tag, by ticket and in attn c_proj (two-pass above four splits), the fp16 and B24 caches.  The E 768 `trained` cases use 48 keys,
  not 6: over 96 heads the range of six scores varies by more than the factor 60 / 8 the regime allows, whatever the gain."""
import numpy as np
import pytest

import score_regimes as rg
import stage_ref as sr
from decode_stage_cases import CASES, CLASS_NAMES, REGIME_CASES, ROUTES, TOK_LO, VOCAB, attention_how, make_tokens, make_weights, plan_case, t_hi_of
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd.synth import GPTConfig

pytestmark = pytest.mark.gpu

MATRICES = ("wte", "wpe", "c_attn_w", "c_proj_w", "c_fc_w", "mlp_proj_w")


def stored(case, w, name):
    return sr.stored_matrix(w[name], case.wt) if name.split(".")[-1] in MATRICES else w[name]


class Report:
    """Figures of one case: every check prints its line before anything is asserted; the failures are raised together."""

    def __init__(self, case):
        self.case, self.failed = case, []

    def check(self, stage, route, worst, bound, Y=None):
        y = "" if Y is None else f" Y {Y:.3e}"
        print(f"STAGE {self.case.id} | {stage} | {route} |{y} worst {worst:.3e} bound {bound:.3e}")
        if not worst <= bound:
            self.failed.append(f"{stage} [{route}]: {worst:.3e} > {bound:.3e}")

    def require(self, ok, what):
        if not ok:
            print(f"STAGE {self.case.id} | {what} | FAILED")
            self.failed.append(what)


def check_planes(rep, stage, raw, K, B, want_f32=None):
    """The rows < B of a plane buffer: a valid exact split, and (where the planes restate a tapped fp32 row) within 1 ulp of it."""
    planes = sr.decode_planes(raw, K)
    rep.require(bool(sr.planes_are_a_valid_split(planes)[:B].all()), f"{stage}: each of hi / mid / lo is the bf16 rounding of the remainder, nothing left over")
    if sr.planes_beyond_fp32(planes[:, :B]):
        print(f"STAGE {rep.case.id} | {stage}: {sr.planes_beyond_fp32(planes[:, :B])} of {B * K} plane sums carry more than fp32's 24 bits")
    v = sr.planes_value(planes)[:B]
    if want_f32 is not None:
        ulps = np.abs(v - want_f32.astype(np.float64)) / np.spacing(np.maximum(np.abs(want_f32), np.float32(1e-30))).astype(np.float64)
        rep.check(f"{stage}: planes against float32(gain * x), in ulp", "planes", float(ulps.max()), 1.0)
    return v


def check_stats(rep, stage, raw, x, B, E):
    st = sr.decode_stats(raw, E)
    ref, s = sr.tile_stats(x)
    rep.check(f"{stage}: tile statistics", "stats", sr.metric(st[:B], ref, np.maximum(s, 1e-300)), sr.STATS_BOUND)
    rep.require(not st[B:].any(), f"{stage}: statistics rows {B}..7 untouched")


def run_case(case, monkeypatch):
    cfg = GPTConfig(VOCAB, case.ctx, case.layers, case.heads, case.E)
    B, E, H, L, T, P = case.batch, case.E, case.heads, case.layers, case.seq_len, case.seq_len - 1
    w = make_weights(case, cfg)
    prompt, toks = make_tokens(case)
    monkeypatch.setenv("ZGPT2_DECODE_PATHS_OFF", str(case.off))
    kw = dict(batch=B, weights_f32=case.wt == "f32", weights_b24=case.wt == "b24", kv_f16=case.kv == "f16", kv_b24=case.kv == "b24")
    m = zgpt.GPT(cfg, **kw)
    twin = zgpt.GPT(cfg, share_weights_with=m, **kw)
    try:
        m.load_weights(w)
        for g in (m, twin):
            if P:
                g.prefill(prompt[:, :P], compute_logits=False)
        taps, info = m.step_taps(T, toks)
        token = m.argmax()
        lg_twin = twin.forward(T, toks)
        rep = Report(case)
        check_step(rep, case, cfg, w, toks, taps, info, token, lg_twin)
        if case.ties:
            check_ties(rep, case, m, w, toks, taps)
    except _lib.ZgError as e:
        if e.code == -3:  # ZG_ERR_HIP: a fault or a timed-out hand-over — nothing more is started on this GPU by this session
            pytest.exit(f"{case.id}: {e}", returncode=3)
        raise
    finally:
        twin.close()
        m.close()
    assert not rep.failed, "\n".join([case.id] + rep.failed)


def by_class(taps):
    d = {}
    for t in taps:
        d.setdefault((t["cls"], t["layer"]), {})[t["name"]] = t
    return d


def check_step(rep, case, cfg, w, toks, taps, info, token, lg_twin):
    B, E, H, L, T, P, V = case.batch, case.E, case.heads, case.layers, case.seq_len, case.seq_len - 1, VOCAB
    modes, plans = plan_case(case)
    rep.require({k: info[k] for k in modes} == modes, f"decode modes {({k: info[k] for k in modes})} as planned on the CPU {modes}")
    rep.require(info["t_hi"] == t_hi_of(case) and info["lm_grid"] == plans[6]["grid"], "t_hi and the lm_head grid as planned")
    pl, st = bool(info["planes"]), bool(info["stats"])
    route = {k: ROUTES[p["route"]] for k, p in plans.items()}
    if info["fused"]:
        route[1] += " in the fused launch"
    tap = by_class(taps)
    data = lambda cls, l, name: tap[(cls, l)][name]["data"]
    W = lambda name: stored(case, w, name)
    n_splits = (info["t_hi"] + 255) // 256

    # ---- class 0, embed: x = wte[token] + wpe[position], one fp32 add of the stored values
    x = data(0, 0, "x").reshape(B, E)
    rep.require(np.array_equal(x, W("wte")[toks.astype(np.int64)] + W("wpe")[P]), "embed: x is wte[token] + wpe[position] to the bit")
    if pl:
        check_planes(rep, "embed", data(0, 0, "xp"), E, B, w["h0.ln_1_g"] * x)
    if st:
        check_stats(rep, "embed", data(0, 0, "xst"), x, B, E)

    for l in range(L):
        p = f"h{l}."
        # ---- class 1, ln_1 + c_attn: q, and the K / V rows appended at position P
        ref, s, y32 = sr.linear_stage(x, W(p + "c_attn_w"), w[p + "c_attn_b"], ln=(w[p + "ln_1_g"], w[p + "ln_1_b"]))
        Y = sr.metric(y32, ref, s)
        t1 = {k: v["data"] for k, v in tap[(1, l)].items()}
        rep.require(bool(tap[(1, l)]["q"]["flags"] & _lib.TAP_FUSED) == bool(info["fused"]), f"L{l} class 1: the table says whether the launch was the fused one")
        q = t1["q"].reshape(B, E)
        Kc, Vc = (sr.decode_cache(t1, n, case.kv, B, H, T) for n in ("k", "v"))
        new = np.concatenate([q, Kc[:, :, P].reshape(B, E), Vc[:, :, P].reshape(B, E)], axis=1).astype(np.float64)
        hu = sr.HALF_ULP[case.kv]
        store = hu * (np.abs(ref) + 3 * Y * s) + (2.0 ** -25 if case.kv == "f16" else 0.0)  # (fp16 subnormals: half their spacing)
        store[:, :E] = 0.0
        rep.check(f"L{l} class 1 {CLASS_NAMES[1]}: q and the new K / V rows (cache {case.kv})", route[1],
                  float(np.max(np.maximum(np.abs(new - ref) - store, 0.0) / s)), sr.bound_y(route[1]) * Y, Y)
        before = {k: v["data"] for k, v in tap[(-1, l)].items()}
        same = all(np.array_equal(before[n].reshape(B, H, T, -1)[:, :, :P], t1[n].reshape(B, H, T, -1)[:, :, :P]) for n in before)
        rep.require(same, f"L{l} class 1: cache positions < {P} keep the bits the prefill left")

        # ---- class 2, attention over the device's own cache and q
        qh = q.reshape(B, H, 64)
        aref, asc = sr.attention(qh, Kc, Vc)
        a32, _ = sr.attention(qh, Kc, Vc, np.float32)
        Y = sr.metric(a32, aref, asc)
        how = attention_how(case, info)
        if pl:
            heads = check_planes(rep, f"L{l} class 2 merged heads", data(2, l, "ap"), E, B)
            heads32 = heads
        else:
            part = data(2, l, "part").reshape(B, H, info["max_splits"], 66)
            heads = sr.merge_partials(part, n_splits).reshape(B, E)
            heads32 = sr.merge_partials(part, n_splits, np.float32).reshape(B, E)
        if not case.regime:
            rep.check(f"L{l} class 2 attention over {T} keys, {n_splits} split(s)", how, sr.metric(heads.reshape(B, H, 64), aref, asc), 3 * Y, Y)
        else:  # the regime's conditions again, on the q and the cache the device holds; its outputs under the regime's rule
            sc = rg.scores(qh[:, :, None], Kc, P)
            print(f"STAGE {case.id} | L{l} class 2 regime | {how} | {rg.describe(sc)}")
            for what in rg.conditions(case.regime, sc, P):
                rep.require(False, f"L{l} class 2: the tapped q and cache are not in the regime: {what}")
            for what, worst, bound, Yr in rg.attention_checks(case.regime, heads.reshape(B, H, 1, 64), aref[:, :, None], asc[:, :, None], a32[:, :, None], P):
                rep.check(f"L{l} class 2 attention over {T} keys, {n_splits} split(s)" + (f": {what}" if what else ""), f"{how}, {rg.parse(case.regime)[0]}", worst, bound, Yr)

        # ---- class 3, (merge +) attn c_proj + residual
        ref, s, y32 = sr.linear_stage(heads, W(p + "c_proj_w"), w[p + "c_proj_b"], resid=x, x32=heads32)
        Y = sr.metric(y32, ref, s)
        x3 = data(3, l, "x").reshape(B, E)
        rep.check(f"L{l} class 3 {CLASS_NAMES[3]}", route[3], sr.metric(x3, ref, s), sr.bound_y(route[3]) * Y, Y)
        if pl:
            check_planes(rep, f"L{l} class 3", data(3, l, "xp"), E, B, w[p + "ln_2_g"] * x3)
        if st:
            check_stats(rep, f"L{l} class 3", data(3, l, "xst"), x3, B, E)

        # ---- class 4, ln_2 + c_fc + gelu
        ref, s, y32 = sr.linear_stage(x3, W(p + "c_fc_w"), w[p + "c_fc_b"], ln=(w[p + "ln_2_g"], w[p + "ln_2_b"]), act="gelu")
        Y = sr.metric(y32, ref, s)
        h4 = check_planes(rep, f"L{l} class 4 gelu output", data(4, l, "hp"), 4 * E, B) if pl else data(4, l, "h4").reshape(B, 4 * E)
        rep.check(f"L{l} class 4 {CLASS_NAMES[4]}", route[4], sr.metric(h4, ref, s), sr.bound_y(route[4]) * Y, Y)

        # ---- class 5, mlp c_proj + residual
        ref, s, y32 = sr.linear_stage(h4, W(p + "mlp_proj_w"), w[p + "mlp_proj_b"], resid=x3)
        Y = sr.metric(y32, ref, s)
        x = data(5, l, "x").reshape(B, E)
        rep.check(f"L{l} class 5 {CLASS_NAMES[5]}", route[5], sr.metric(x, ref, s), sr.bound_y(route[5]) * Y, Y)
        for name, on in (("xp", pl), ("xst", st)):
            if not on:
                continue
            written = not tap[(5, l)][name]["flags"] & _lib.TAP_NOT_WRITTEN
            rep.require(written == (l + 1 < L), f"L{l} class 5: the table marks {name} as written for a next layer only")
            if not written:
                rep.require(np.array_equal(data(5, l, name), data(3, l, name)), f"L{l} class 5 (last layer): {name} unchanged")
            elif name == "xp":
                check_planes(rep, f"L{l} class 5", data(5, l, "xp"), E, B, w[f"h{l + 1}.ln_1_g"] * x)
            else:
                check_stats(rep, f"L{l} class 5", data(5, l, "xst"), x, B, E)

    # ---- class 6, ln_f + lm_head, the token, and the anchor
    ref, s, y32 = sr.linear_stage(x, W("wte"), None, ln=(w["ln_f_g"], w["ln_f_b"]))
    Y = sr.metric_granted(y32, ref, s, sr.LOGIT_ULPS)
    lg = data(6, 0, "logits").reshape(B, V)
    print(f"STAGE {case.id} | class 6: largest |logit| {float(np.max(np.abs(ref) / s)):.1f} s; plain metric: Y {sr.metric(y32, ref, s):.3e} kernel {sr.metric(lg, ref, s):.3e}")
    rep.check(f"class 6 {CLASS_NAMES[6]} (four ulp of the logit granted on both sides: stage_ref.LOGIT_ULPS)", route[6],
              sr.metric_granted(lg, ref, s, sr.LOGIT_ULPS), sr.bound_y(route[6]) * Y, Y)
    rep.require(np.array_equal(token.astype(np.int64), lg.argmax(axis=1)), f"argmax {token} is the lowest index of the maximum of the tapped logits {lg.argmax(axis=1)}")
    rep.require(lg.tobytes() == lg_twin.tobytes(), "anchor: tapped logits bit-equal to zg_gpt_forward on a twin handle")


def check_ties(rep, case, m, w, toks, taps):
    """lm_head again with wte rows duplicated so that sequence 0's maximum is tied between two indices: in different 16-row tiles
    of one workgroup (where a workgroup holds more than one), in different workgroups, and in rows 0 and V - 1.  The rows are
    twice the winning row (a positive logit doubled is the new maximum) and belong to tokens no sequence was fed, so the step up
    to lm_head is unchanged."""
    _, plans = plan_case(case)
    p6 = plans[6]
    R = p6["rows_per_wg"] or p6["rows_per_wave"] * p6["waves_per_wg"]  # rows of wte per workgroup
    lg = by_class(taps)[(6, 0)]["logits"]["data"].reshape(case.batch, VOCAB)
    t = int(lg[0].argmax())
    rep.require(lg[0, t] > 0, "ties: the winning logit of sequence 0 is positive")
    pairs = {"different workgroups": (3, 3 + R), "rows 0 and V - 1": (0, VOCAB - 1)}
    if R >= 32:
        pairs["different 16-row tiles of one workgroup"] = (3, 19)
    else:
        print(f"STAGE {case.id} | ties: a workgroup of {ROUTES[p6['route']]} holds {R} rows here, one tile: no tie inside a workgroup to make")
    for what, (a, b) in pairs.items():
        assert b < TOK_LO or b == VOCAB - 1, (what, a, b, R)
        wte = w["wte"].copy()
        wte[a] = wte[b] = np.float32(2.0) * w["wte"][t]
        _lib.check(m._L.zg_gpt_load_tensor(m.h, 0, _lib.ptr(wte), wte.size))
        t2, _ = m.step_taps(case.seq_len, toks)
        token = m.argmax()
        lg2 = by_class(t2)[(6, 0)]["logits"]["data"].reshape(case.batch, VOCAB)
        rep.require(lg2[0, a] == lg2[0, b] == lg2[0].max(), f"ties, {what}: rows {a} and {b} hold the same logit and it is the maximum")
        rep.require(int(token[0]) == a, f"ties, {what} ({ROUTES[p6['route']]}, {R} rows per workgroup): token {int(token[0])}, lowest tied index {a}")
        rep.require(np.array_equal(token.astype(np.int64), lg2.argmax(axis=1)), f"ties, {what}: every sequence's token is the lowest index of its maximum")


@pytest.mark.parametrize("case", CASES + REGIME_CASES, ids=lambda c: c.id)
def test_every_stage_of_a_decode_step_against_float64(zg, monkeypatch, case):
    run_case(case, monkeypatch)
