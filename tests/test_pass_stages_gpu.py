"""Every kernel hand-over of the whole-prompt pass against float64, stage by stage.

A tapped pass (zg_debug_gpt_pass_taps) returns what each launch of zg_gpt_prefill / zg_gpt_extend / zg_gpt_score wrote.  Each
stage's float64 reference (stage_ref) is computed from the input the DEVICE gave that stage, so nothing compounds over layers and
a failure names its launch.  Metric of a Linear: per output |got - ref64| / s, s = sqrt(sum_k (a_k w_nk)^2) + |bias_n| + |resid_n|;
of the attention: s = the l2 norm of the weighted V terms; of a LayerNorm: s = |g| (|x| + |mean|) / sigma + |b|.  Bound: 3 x Y,
Y = the same metric for a float32 numpy evaluation of the same stage from the same tapped input (Linears: the blocked float32
sum row by row, over all rows up to 256 and a fixed sample beyond: stage_ref.yardstick_rows) — computed here, from the reference
side alone; the float64 reference and the kernel's error always cover every row.  K / V rows appended to a 16- or 24-bit cache
are bitwise the format's rounding of the qkv columns where the launch stored those, and get half an ulp of the format
elsewhere; every cache position in front of the pass and the rows behind its end must keep their bits.  Planes are held to being
a valid three-term split.  The plan ints of every GEMM launch and the attention's kernel and geometry must be what
pass_stage_cases.plan_case predicted on the CPU, and the logits bit-equal to the plain call on a twin handle, with one decode
step on top.  The cases: pass_stage_cases.py; that the list reaches every route a model can, and that 3 x Y has teeth against
five emulated defects: test_pass_stage_cases_cpu.py.

Measured on one MI355X (34 cases, every case under 0.7 s with its references; lm_head rows with four ulp of the logit granted):

| route / check | checks | Y min .. max | kernel worst | worst / Y |
|---|---|---|---|---|
| LayerNorm + split, ln_split_kernel (first ln_1, ln_f) | 6 | 2.3e-07 .. 7.6e-07 | 1.8e-06 | 2.40 |
| LayerNorm + split, ln_split_kernel behind a GEMM (tail LN_SPLIT) | 16 | 9.1e-08 .. 2.1e-06 | 1.8e-06 | 1.00 |
| LayerNorm + split in the reduce + residual tail (REDUCE_RESID_LN) | 37 | 1.6e-07 .. 4.0e-06 | 3.4e-06 | 2.28 |
| PF_T128 whole, 3 planes (bound 6 Y) | 47 | 6.1e-08 .. 7.6e-07 | 1.6e-06 | 4.25 |
| PF_T128 whole, 2 planes | 4 | 2.1e-07 .. 4.0e-07 | 6.9e-07 | 1.73 |
| PF_T128 through the workspace, 3 planes | 26 | 8.5e-08 .. 8.4e-07 | 1.5e-06 | 2.96 |
| PF_T128 through the workspace, 2 planes | 5 | 4.0e-07 .. 6.6e-07 | 1.4e-06 | 2.12 |
| PF_T128_WP (fp32 / B24 weights, three passes) | 27 | 2.2e-07 .. 8.8e-07 | 1.5e-06 | 2.57 |
| PF_S4, 3 plane pairs, 1 K slice (bound 6 Y) | 33 | 2.1e-07 .. 7.8e-07 | 2.9e-06 | 3.97 |
| PF_S4, 3 plane pairs, 1 K slice, stream-K hand-over (both runs) | 2 | 6.4e-07 | 1.8e-06 | 2.81 |
| PF_S4, 3 plane pairs, 2 / 3 / 4 K slices | 2 / 3 / 12 | 3.4e-07 .. 9.3e-07 | 1.5e-06 | 1.77 / 1.71 / 1.81 |
| PF_S4, 2 plane pairs, 1 / 3 / 4 K slices | 2 / 1 / 1 | 4.1e-07 .. 7.2e-07 | 1.3e-06 | 2.43 / 0.81 / 1.01 |
| PF_S4, 6 plane pairs (fp32 / B24 weights), 1 / 3 / 4 K slices | 9 / 2 / 5 | 2.6e-07 .. 8.4e-07 | 2.0e-06 | 2.77 / 0.97 / 1.42 |
| attention, whole-prompt kernel, one range | 26 | 0 .. 5.1e-06 | 4.3e-06 | 1.19 |
| attention, whole-prompt kernel, ranges merged | 9 | 2.4e-06 .. 1.3e-05 | 5.5e-06 | 0.97 |
| attention, continuation kernel, fp32 cache, ranges merged | 1 | 1.8e-06 | 1.5e-06 | 0.83 |
| attention, continuation kernel, fp16 cache, one range / merged | 2 / 2 | 1.4e-06 .. 1.3e-05 | 4.9e-06 | 0.64 / 0.39 |
| attention, continuation kernel, B24 cache, one range | 3 | 2.4e-07 .. 1.4e-06 | 1.2e-06 | 1.39 |
| two-plane control: c_attn's q against the three-plane reference (must be above 3 Y) | 3 | 4.1e-07 .. 6.3e-07 | 1.1e-05 | 17.6 .. 23.5 |

The lm_head rows of the score stage are among PF_T128 whole (bf16 weights: 320 rows of wte and the strip of 13) and PF_T128_WP.
Every bitwise check held in all 34 cases: the embed, the appended cache rows against the format's rounding of the stored k / v
columns, the cache in front of and behind the appended range, pf_a behind the last Block, the copied score logits, the plan ints
and attention geometry against the CPU prediction, and the anchor (tapped call, plain call on the twin, one forward step on top).
tests/test_prefill_linear_gpu.py holds the same metric beside its own assertions (22 launches, worst 3.24 Y on PF_T128 whole,
the 128 x 256 tiles 2.0 Y); tests/test_attn_prefill_gpu.py likewise (14 cases up to 1023 rows, worst 1.19 Y).

The attention again under the score regimes of score_regimes.py (20 one-layer cases beside the 34 above, 3.4 s together; as
test_decode_stages_gpu.py: `trained` under 6 Y — stage_ref.BOUND_Y's PF_ATTN_WIDE, see the findings —, one-key@P and far-below with
8 ulp of the output granted on both sides for the outputs of head 0 that see P, stage_ref.ATTN_ULPS; hot keys: position 0 for
every row, the last key of the first key range, a key of the second range, a key among the cached ones).  Measured on the same MI355X:

| how | regime | checks | Y min .. max | kernel worst | worst / Y |
|---|---|---|---|---|---|
| whole-prompt kernel, one range (E 128, E 384 under both pins) | trained | 3 | 2.2e-06 .. 3.3e-06 | 7.0e-06 | 3.02 |
| whole-prompt kernel, one range | one-key, head 0 | 1 | 0 | 0 beyond the grant | |
| whole-prompt kernel, one range | far-below, head 0 | 1 | 2.8e-05 | 7.4e-05 | 2.63 |
| whole-prompt kernel, 3 ranges merged | trained | 2 | 3.9e-06 .. 4.0e-06 | 7.7e-06 | 1.90 |
| whole-prompt kernel, 3 ranges merged | one-key, head 0 (hot 0, 127, 200) | 4 | 0 | 0 beyond the grant | |
| continuation kernel, fp32 cache, 2 ranges merged | trained / one-key, head 0 | 1 / 1 | 3.5e-06 / 0 | 7.1e-06 / 0 beyond the grant | 2.00 |
| continuation kernel, fp16 cache, one range | trained / one-key, head 0 | 1 / 1 | 1.2e-06 / 0 | 3.2e-06 / 0 beyond the grant | 2.70 |
| continuation kernel, fp16 cache, 3 ranges merged | trained / one-key, head 0 | 1 / 2 | 4.5e-06 / 0 | 7.2e-06 / 0 beyond the grant | 1.59 |
| continuation kernel, B24 cache, one range | trained / one-key, head 0 | 1 / 1 | 2.8e-06 / 0 | 3.4e-06 / 0 beyond the grant | 1.22 |
| the outputs a one-key / far-below case leaves alone, all of the above | | 11 | 1.1e-06 .. 6.4e-06 | 8.3e-06 | 1.37 |

Emulated defects in the same metric (CPU, every width and weight type of the list, smallest and largest M; Y there 2.9e-07 ..
1.4e-06): activations cut to two planes, an appended fp32 K / V row rounded to fp16, fp32 / B24 weights cut to bf16, one K slab of
a sliced residual add left out, the causal mask off by one key — the least any of them measures is 4.0 x its bound (two planes,
c_fc at E 384 and attn c_proj at E 768).

Findings, none of them a wrong result:
- PF_T128 and PF_S4 with bf16 weights: seven of 176 launches lie above 3 Y (4.25, 3.23, 3.07 Y on the 128-row kernel at K = 128;
  3.07 Y at K = 768 and 3.67 / 3.74 / 3.97 Y at K = 1600 on the persistent kernel).  Both carry one fp32 accumulator per output
  through the whole K loop, the lo, mid and hi plane of each 16-column step one behind the other: 3 K / 16 sequential matrix-core
  accumulations, where the yardstick is a blocked sum.  The kernels' worst value is 1.0e-6 .. 2.9e-6 whatever the shape, about
  2e-7 x sqrt(chain length), as GR_MFMA16 measures in the decode step (9.8e-7); the 4.25 Y is at M = 1, where Y is one row's
  2.5e-7.  Correct by reading; bound 6 Y for the two routes (stage_ref.BOUND_Y), and every emulated defect still clears that by
  2.0 x at the least (asserted on the CPU).
- An output whose metric scale s is exactly 0 exists (the first query of a sequence sees one key, and the seeded V row holds an
  exact zero): stage_ref.metric holds such an output to being exact instead of dividing 0 by 0.
- The score regimes: with scores tens of units wide the prompt attention's error is 3.2e-6 .. 7.7e-6 whatever the shape, 1.2 .. 2.7 Y
  and 3.02 Y in one launch of nine (E 384, 3 x 43 rows; 2.63 Y far below 0), where the decode kernels stay within 1.6 Y: a score
  is one accumulator through 24 sequential matrix-core accumulations of a query scaled by log2(e) / 8 and rounded before its
  split, and exp turns the score's absolute error into a relative error of p, which at +-0.05 never showed.  Correct by reading;
  bound 6 Y for the regime cases (stage_ref.BOUND_Y, PF_ATTN_WIDE), which the query cut to two planes exceeds by 1.98 x at the
  least and scores of 16 mantissa bits by 11 x (asserted on the CPU); the cases above keep 3 Y.  With one key holding all the
  mass both kernels and the range merge return V's row to within the 8 ulp granted, on every cache format.
- The persistent kernel does not store the k / v columns of pf_qkv when the cache is fp32 (the attention reads the cache): the
  tapped table marks them not-written, and the appended rows are then held to the Linear's bound directly."""
import time

import numpy as np
import pytest

import score_regimes as rg
import stage_ref as sr
from pass_stage_cases import (CASES, CLASS_NAMES, FIELDS, REGIME_CASES, TOK_LO, V64, VOCAB, attention_how, make_tokens, make_weights, pass_route, pf_ws_floats,
                              plan_case)
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd.synth import GPTConfig

pytestmark = pytest.mark.gpu

MATRICES = ("wte", "wpe", "c_attn_w", "c_proj_w", "c_fc_w", "mlp_proj_w")
KV_MODE, WEIGHT_TYPE = {"f32": 0, "f16": 1, "b24": 2}, {"bf16": 0, "f32": 1, "b24": 2}


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


def by_class(taps):
    d = {}
    for t in taps:
        d.setdefault((t["cls"], t["layer"]), {}).setdefault(t["name"], []).append(t)
    return d


def rows_of(cache, past, n):
    """[B][H][T][64] -> the rows of positions past .. past + n - 1 as [B n][H 64], row b n + t."""
    B, H = cache.shape[:2]
    return cache[:, :, past:past + n].transpose(0, 2, 1, 3).reshape(B * n, H * 64)


def run_case(case, zg, monkeypatch):
    cfg = GPTConfig(VOCAB, case.context, case.layers, case.heads, case.E)
    B, n, past = case.batch, case.n, case.past
    w = make_weights(case, cfg)
    toks, rng = make_tokens(case)
    if case.wgs:
        monkeypatch.setenv("ZGPT2_GEMM_WGS", str(case.wgs))
    else:
        monkeypatch.delenv("ZGPT2_GEMM_WGS", raising=False)
    kw = dict(batch=B, weights_f32=case.wt == "f32", weights_b24=case.wt == "b24", kv_f16=case.kv == "f16", kv_b24=case.kv == "b24",
              prefill_planes=case.planes, score=case.score)
    _lib.check(zg.zg_debug_prefill_route(*case.pin))
    m = zgpt.GPT(cfg, **kw)
    twin = zgpt.GPT(cfg, share_weights_with=m, **kw)
    rep = Report(case)
    t0 = time.perf_counter()
    try:
        m.load_weights(w)
        for g in (m, twin):
            if past:
                g.extend(0, toks[:, :past], compute_logits=False)
        new = toks[:, past:]
        taps, info, lg = m.pass_taps(new, past_len=past, compute_logits=case.logits, score=case.score)
        lg_twin = twin.score(new, past_len=past, want_logits=True)[-1] if case.score else twin.extend(past, new, compute_logits=case.logits)
        gpu_s = time.perf_counter() - t0
        check_pass(rep, case, w, toks, taps, info, lg)
        rep.require(case.logits == (lg is not None) and (lg is None or lg.tobytes() == lg_twin.tobytes()),
                    "anchor: the tapped call's logits bit-equal to the plain call on a twin handle")
        if case.twice:  # the same pass again on the same handle: c_attn's hand-over flags carry the epoch of the launch
            taps2, _, lg2 = m.pass_taps(new, past_len=past, compute_logits=case.logits, score=case.score)
            check_pass(rep, case, w, toks, taps2, info, lg2, only_c_attn=True)
            rep.require(lg2.tobytes() == lg_twin.tobytes(), "anchor: the second tapped call's logits bit-equal to the first plain call's")
        if past + n < case.context:
            nxt = rng.integers(TOK_LO, VOCAB - 1, size=B).astype(np.uint64)
            rep.require(m.forward(past + n + 1, nxt).tobytes() == twin.forward(past + n + 1, nxt).tobytes(),
                        "anchor: one forward step on top bit-equal to the twin's")
        else:
            print(f"STAGE {case.id} | the pass ends at the end of the context: no forward step on top")
    except _lib.ZgError as e:
        if e.code == -3:  # ZG_ERR_HIP: a fault or a timed-out hand-over — nothing more is started on this GPU by this session
            pytest.exit(f"{case.id}: {e}", returncode=3)
        raise
    finally:
        twin.close()
        m.close()
        zg.zg_debug_prefill_route(0, 0)
    print(f"STAGE {case.id} | time | device calls {gpu_s:.2f} s, with the references {time.perf_counter() - t0:.2f} s")
    assert not rep.failed, "\n".join([case.id] + rep.failed)


def check_planes(rep, stage, raw, M, K):
    planes = sr.decode_row_planes(raw, M, K)
    rep.require(bool(sr.planes_are_a_valid_split(planes).all()), f"{stage}: each of hi / mid / lo is the bf16 rounding of the remainder, nothing left over")
    return planes


def check_ln(rep, stage, route, raw, x, g, b):
    """A LayerNorm + split launch (or tail): valid planes whose value is within 3 Y of float64.  Returns the planes."""
    planes = check_planes(rep, stage, raw, *x.shape)
    ref, s, y32 = sr.layernorm_stage(x, g, b)
    Y = sr.metric(y32, ref, s)
    rep.check(stage, route, sr.metric(sr.planes_value(planes), ref, s), 3 * Y, Y)
    return planes


def fed(case, planes):
    """What a Linear multiplies of its input planes: all three, or hi + mid on a two-plane handle with bf16 weights."""
    return sr.planes_value(planes if case.planes == 3 or case.wt != "bf16" else planes[:2])


def check_pass(rep, case, w, toks, taps, info, lg, only_c_attn=False):
    B, E, H, L, n, past, V = case.batch, case.E, case.heads, case.layers, case.n, case.past, VOCAB
    M, end, T = B * n, past + n, min(case.context, past + n + _lib.PASS_TAP_ROWS_BEHIND)
    plans, att = plan_case(case)
    want_info = {"planes": 3 if case.wt != "bf16" else case.planes, "kv_mode": KV_MODE[case.kv], "weight_type": WEIGHT_TYPE[case.wt],
                 "pf_ws_floats": pf_ws_floats(case), "stream_k_operands": int(case.wt == "bf16"), "v64": V64, "score_rows": 256}
    rep.require(info == want_info, f"info {info} as planned {want_info}")
    tap = by_class(taps)
    one = lambda cls, l, name: tap[(cls, l)][name][0]
    data = lambda cls, l, name: one(cls, l, name)["data"]
    W = lambda name: sr.stored_matrix(w[name], case.wt) if name.split(".")[-1] in MATRICES else w[name]
    planned = {}
    for cls, l, role, p in plans:
        planned.setdefault((cls, l), []).append(p)
    got_plans = {k: [dict(zip(FIELDS, (int(v) for v in t["data"]))) for t in d.get("plan", [])] for k, d in tap.items()}
    rep.require({k: v for k, v in got_plans.items() if v} == planned, "the plan ints of every GEMM launch are what plan_case predicted on the CPU")
    route = lambda cls, l, i=0: pass_route(planned[(cls, l)][i])
    cache = lambda cls, l, which: sr.decode_cache({k: v[0]["data"] for k, v in tap[(cls, l)].items()}, which, case.kv, B, H, T)

    # ---- class 0, embed: x = wte[token] + wpe[position], one fp32 add of the stored values
    x = data(0, 0, "x").reshape(M, E)
    pos = np.tile(np.arange(past, end), B)
    rep.require(np.array_equal(x, W("wte")[toks[:, past:].reshape(-1).astype(np.int64)] + W("wpe")[pos]), "embed: x is wte[token] + wpe[pos0 + t] to the bit")
    # ---- class 1, the first LayerNorm + split
    a = check_ln(rep, "class 1 ln_1 + split", "ln_split", data(1, 0, "a"), x, w["h0.ln_1_g"], w["h0.ln_1_b"])

    for l in range(L):
        p = f"h{l}."
        # ---- class 2, c_attn: q, the k / v columns, the appended cache rows and everything around them
        ref, s, Y = sr.pass_linear_stage(fed(case, a), W(p + "c_attn_w"), w[p + "c_attn_b"], n_seq=n)
        q = data(2, l, "q").reshape(M, E)
        Kc, Vc = cache(2, l, "k"), cache(2, l, "v")
        new_kv = np.concatenate([rows_of(Kc, past, n), rows_of(Vc, past, n)], axis=1)
        kv_cols = one(2, l, "qkv_kv")
        cols_written = not kv_cols["flags"] & _lib.TAP_NOT_WRITTEN
        rep.require(cols_written == (not (planned[(2, l)][0]["family"] == 1 and case.kv == "f32")),
                    f"L{l} class 2: the table marks the k / v columns of pf_qkv as written unless the persistent kernel appends to an fp32 cache")
        bound = sr.bound_y(route(2, l)) * Y
        if cols_written:
            cols = kv_cols["data"].reshape(M, 2 * E)
            rep.check(f"L{l} class 2 {CLASS_NAMES[2]}: q and the k / v columns", route(2, l), sr.metric(np.concatenate([q, cols], axis=1), ref, s), bound, Y)
            rep.require(np.array_equal(sr.store_kv(cols, case.kv).view(np.uint32), new_kv.view(np.uint32)),
                        f"L{l} class 2: the appended cache rows are bitwise the {case.kv} rounding of the k / v columns, at [b][h][pos0 + t]")
        else:
            hu = sr.HALF_ULP[case.kv]
            grant = hu * (np.abs(ref) + 3 * Y * s) + (2.0 ** -25 if case.kv == "f16" else 0.0)
            grant[:, :E] = 0.0
            got = np.concatenate([q, new_kv], axis=1).astype(np.float64)
            rep.check(f"L{l} class 2 {CLASS_NAMES[2]}: q and the new K / V rows at [b][h][pos0 + t] (cache {case.kv})", route(2, l),
                      float(np.max(np.maximum(np.abs(got - ref) - grant, 0.0) / s)), bound, Y)
        if case.planes == 2 and case.wt == "bf16" and l == 0:  # the control: against all three planes the lost plane shows
            ref3, s3, Y3 = sr.pass_linear_stage(sr.planes_value(a), W(p + "c_attn_w"), w[p + "c_attn_b"], n_seq=n)
            lost = sr.metric(q, ref3[:, :E], s3[:, :E])
            print(f"STAGE {case.id} | L0 class 2 two-plane control | {route(2, l)} | Y {Y3:.3e} q against the three-plane reference {lost:.3e} = {lost / Y3:.1f} Y")
            rep.require(lost > 3 * Y3, "two-plane control: c_attn's q is ABOVE the three-plane bound against the full reference (the metric sees a lost plane)")
        before, after = tap[(-1, l)], tap[(2, l)]
        for name in before:
            b4, af = (d[name][0]["data"].reshape(B, H, T, -1) for d in (before, after))
            rep.require(np.array_equal(b4[:, :, :past], af[:, :, :past]), f"L{l} class 2: {name} of positions < {past} keeps its bits")
            rep.require(np.array_equal(b4[:, :, end:], af[:, :, end:]), f"L{l} class 2: {name} rows behind the pass's end ({end} .. {T - 1}) are not written")
        if only_c_attn:
            return
        if l + 1 == L and not (case.logits or case.score):
            rep.require(not any((cls, l) in tap for cls in (3, 4, 5, 6)), "the last Block of a pass without logits stops behind its cache append")
            return

        # ---- class 3, attention over the values the device read
        geo = [int(v) for v in data(3, l, "geo")]
        got_att = (geo[1], geo[0] & 0xFF, (geo[0] >> 8) & 0xFF, geo[0] >> 16)
        rep.require(got_att == att and geo[2] == int(att[2] > 1), f"L{l} class 3: kernel and geometry {got_att}, merge {geo[2]}; planned {att}")
        if att[0] == 0 and case.kv != "f32":  # a whole prompt on a 16- / 24-bit cache reads the unrounded qkv columns
            rep.require(cols_written, f"L{l} class 3: the k / v columns the attention reads were stored")
            Kr, Vr = (cols[:, i * E:(i + 1) * E].reshape(B, n, H, 64).transpose(0, 2, 1, 3) for i in (0, 1))
        else:
            Kr, Vr = Kc[:, :, :end], Vc[:, :, :end]
        qh = q.reshape(B, n, H, 64).transpose(0, 2, 1, 3)
        aref, asc = sr.causal_attention(qh, Kr, Vr, past)
        a32 = sr.causal_attention(qh, Kr, Vr, past, np.float32)[0]
        Ya = sr.metric(a32, aref, asc)
        a = check_planes(rep, f"L{l} class 3 heads", data(3, l, "a"), M, E)
        heads = sr.planes_value(a).reshape(B, n, H, 64).transpose(0, 2, 1, 3)
        how = attention_how(case, att)
        if not case.regime:
            rep.check(f"L{l} class 3 attention of {n} positions behind {past}", "attention: " + how, sr.metric(heads, aref, asc), 3 * Ya, Ya)
        else:  # the regime's conditions again, on the q and the keys the device read; its outputs under the regime's rule
            sc = rg.scores(qh, Kr, past)
            print(f"STAGE {case.id} | L{l} class 3 regime | attention: {how} | {rg.describe(sc)}")
            for what in rg.conditions(case.regime, sc, past):
                rep.require(False, f"L{l} class 3: the tapped q and keys are not in the regime: {what}")
            for what, worst, bound, Yr in rg.attention_checks(case.regime, heads, aref, asc, a32, past, wide=sr.bound_y("PF_ATTN_WIDE")):
                rep.check(f"L{l} class 3 attention of {n} positions behind {past}" + (f": {what}" if what else ""), f"attention: {how}, {rg.parse(case.regime)[0]}", worst, bound, Yr)

        # ---- class 4, attn c_proj + residual, and ln_2 + split in its tail
        ref, s, Y = sr.pass_linear_stage(fed(case, a), W(p + "c_proj_w"), w[p + "c_proj_b"], resid=x, n_seq=n)
        x4 = data(4, l, "x").reshape(M, E)
        rep.check(f"L{l} class 4 {CLASS_NAMES[4]}", route(4, l), sr.metric(x4, ref, s), sr.bound_y(route(4, l)) * Y, Y)
        a4 = check_ln(rep, f"L{l} class 4 ln_2 + split", "tail " + str(planned[(4, l)][0]["tail"]), data(4, l, "a"), x4, w[p + "ln_2_g"], w[p + "ln_2_b"])

        # ---- class 5, c_fc + GELU + split
        ref, s, Y = sr.pass_linear_stage(fed(case, a4), W(p + "c_fc_w"), w[p + "c_fc_b"], act="gelu", n_seq=n)
        hp = check_planes(rep, f"L{l} class 5 gelu output", data(5, l, "hp"), M, 4 * E)
        rep.check(f"L{l} class 5 {CLASS_NAMES[5]}", route(5, l), sr.metric(sr.planes_value(hp), ref, s), sr.bound_y(route(5, l)) * Y, Y)

        # ---- class 6, mlp c_proj + residual, and the next ln_1 + split in its tail
        ref, s, Y = sr.pass_linear_stage(fed(case, hp), W(p + "mlp_proj_w"), w[p + "mlp_proj_b"], resid=x4, n_seq=n)
        x = data(6, l, "x").reshape(M, E)
        rep.check(f"L{l} class 6 {CLASS_NAMES[6]}", route(6, l), sr.metric(x, ref, s), sr.bound_y(route(6, l)) * Y, Y)
        written = not one(6, l, "a")["flags"] & _lib.TAP_NOT_WRITTEN
        rep.require(written == (l + 1 < L), f"L{l} class 6: the table marks pf_a as written for a next layer only")
        if written:
            a = check_ln(rep, f"L{l} class 6 next ln_1 + split", "tail " + str(planned[(6, l)][0]["tail"]), data(6, l, "a"), x, w[f"h{l + 1}.ln_1_g"], w[f"h{l + 1}.ln_1_b"])
        else:
            rep.require(np.array_equal(data(6, l, "a"), data(4, l, "a")), f"L{l} class 6 (last layer): pf_a unchanged")

    if not case.score:
        return
    # ---- class 7, score: ln_f of every row, then block by block the lm_head on the matrix cores
    af = check_ln(rep, "class 7 ln_f + split", "ln_split", data(7, 0, "a"), x, w["ln_f_g"], w["ln_f_b"])
    act = fed(case, af).astype(np.float32)  # (exact: hi + mid + lo, or hi + mid, is an fp32 number)
    for blk, r0 in enumerate(range(0, M, 256)):
        rows = min(256, M - r0)
        ref, s, y32 = sr.linear_stage(act[r0:r0 + rows], W("wte"), None)
        Y = sr.metric_granted(y32, ref, s, sr.LOGIT_ULPS)
        got = data(7, blk, "logits").reshape(rows, V64)
        r = route(7, blk)
        rep.check(f"class 7 block {blk} ({rows} rows) {CLASS_NAMES[7]} (four ulp of the logit granted on both sides)", r,
                  sr.metric_granted(got[:, :V], ref, s, sr.LOGIT_ULPS), sr.bound_y(r) * Y, Y)
        out = lg.reshape(M, V)[r0:r0 + rows]
        rep.require(out.tobytes() == np.ascontiguousarray(got[:, :V]).tobytes(), f"class 7 block {blk}: the copied logits are columns < {V} of the block, nothing of {V} .. {V64 - 1}")


@pytest.mark.parametrize("case", CASES + REGIME_CASES, ids=lambda c: c.id)
def test_every_stage_of_a_whole_prompt_pass_against_float64(zg, monkeypatch, case):
    run_case(case, zg, monkeypatch)
