"""The cases of the decode-stage tests and what the library plans for them, without a GPU.

A case is one small model, one batch, one storage choice, one ZGPT2_DECODE_PATHS_OFF value and one position.  plan_case() mirrors
zg_gpt_create's mode decisions (activation planes, tile statistics, tagged hand-overs, the fused batch-1 launch) from the plans
zg_debug_gemv_plan returns for the arguments the *_args builders of api_gpt_step.hip lay out, and then plans the five Linear launches
of a step; test_decode_stages_gpu.py holds the handle's own report (zg_debug_gpt_step_taps info) to these predictions, so the
coverage test_decode_stage_cases_cpu.py asserts on the CPU is the coverage the GPU test runs."""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from test_gemv_plan_cpu import (B24, BF16, EPI_ARGMAX, EPI_GELU, EPI_QKV, EPI_RESID, F32, FIELDS, LN_FOLDED, PLANES_IN, PRO_LN, PRO_MERGE, PRO_NONE,
                                SPLIT_K, STATS_IN)

import score_regimes
from zig_gpt2_amd import _lib, synth

ROUTES = ["GR_VALU", "GR_VALU_GROUPS", "GR_GENERIC", "GR_KSPLIT", "GR_LNK", "GR_MFMA16", "GR_MFMA16_KS", "GR_PL4", "GR_PL4_KS", "GR_LM_WPT"]
MODEL_ROUTES = [r for r in ROUTES if r not in ("GR_VALU_GROUPS", "GR_GENERIC")]  # those two: plain op-tier Linears only
WT = {"bf16": BF16, "f32": F32, "b24": B24}
CLASS_NAMES = {1: "ln_1 + c_attn", 3: "attn c_proj", 4: "ln_2 + c_fc", 5: "mlp c_proj", 6: "lm_head"}
VOCAB = 333  # a few hundred, 20 tiles of 16 and 13 rows over
TOK_MEAN, TOK_OUT = VOCAB - 3, VOCAB - 4  # wte rows with mean 0.3 / std 2, and with a few 30 x outlier channels
TOK_LO = VOCAB // 2                        # input tokens come from [TOK_LO, VOCAB - 2]: the rows below and row V - 1 are free for the ties


@dataclass(frozen=True)
class Case:
    E: int
    batch: int
    wt: str = "bf16"   # weights: bf16, f32, b24
    kv: str = "f32"    # cache: f32, f16, b24
    off: int = 0       # ZGPT2_DECODE_PATHS_OFF while the handle is created and runs
    seq_len: int = 6   # the tapped step's position + 1; seq_len - 1 tokens are prefilled
    ctx: int = 64
    layers: int = 1
    ties: bool = False  # also the argmax ties (lm_head again with duplicated wte rows)
    regime: str = ""    # the attention scores' regime (score_regimes): "" = N(0, 0.02) weights, "trained", "one-key@P", "far-below"

    @property
    def id(self):
        return f"E{self.E}-b{self.batch}-{self.wt}-kv{self.kv}-off{self.off}-t{self.seq_len}-L{self.layers}" + (f"-{self.regime}" if self.regime else "")

    @property
    def heads(self):
        return self.E // 64


def _cases():
    c = []
    # every width at one sequence (VALU, K split, folded LayerNorm, the fused launch) and in lock step (matrix cores, planes)
    for E in (128, 384, 768, 1024, 1280, 1600, 2048):
        c.append(Case(E, 1, layers=2 if E <= 384 else 1, ties=E == 128))
        c.append(Case(E, 8 if E != 384 else 5, layers=2 if E <= 384 else 1, ties=E in (384, 1024, 1600)))
    # the other batch sizes (rows held: 2, 4, 8) and storage types; fp32 / B24 weights stay on the vector ALUs at any batch
    c += [Case(128, 2), Case(768, 3, kv="f16"), Case(1280, 2, kv="b24"), Case(384, 1, kv="f16", layers=2), Case(768, 1, kv="b24"),
          Case(128, 3, wt="f32", layers=2, ties=True), Case(768, 2, wt="f32"), Case(1024, 2, wt="f32", kv="f16"), Case(1600, 5, wt="f32"),
          Case(384, 8, wt="b24", kv="b24", layers=2), Case(1280, 1, wt="b24"), Case(2048, 2, wt="b24"), Case(768, 4, wt="b24", kv="f16", ties=True)]
    # each newer path switched off: 1 planes, 2 the four-wave Linear, 4 tagged hand-overs, 8 tile statistics, 16 line-shaped
    # loads, 32 the wave-per-tile lm_head, 64 the fused batch-1 launch
    c += [Case(768, 8, off=1), Case(1024, 3, off=1), Case(1600, 2, off=1), Case(2048, 8, off=1), Case(384, 2, off=2, layers=2), Case(1024, 8, off=2),
          Case(1024, 5, off=4), Case(1600, 3, off=4), Case(768, 2, off=8), Case(1280, 8, off=8), Case(768, 8, off=16), Case(2048, 3, off=16), Case(128, 2, off=16), Case(1600, 5, off=16),
          Case(384, 8, off=32, ties=True), Case(768, 5, off=32), Case(1024, 2, off=32), Case(128, 1, off=64, layers=2), Case(1024, 1, off=64)]
    # positions: the first, exactly one attention chunk of 256, one key in the second split, the last of the context
    for t in (1, 256, 257, 320):
        c.append(Case(128, 1, seq_len=t, ctx=320, layers=2))
        c.append(Case(128, 3, seq_len=t, ctx=320, layers=2))
    c += [Case(128, 1, kv="f16", seq_len=257, ctx=320), Case(128, 2, kv="b24", seq_len=257, ctx=320), Case(128, 2, off=4, seq_len=320, ctx=320),
          Case(128, 1, off=64, seq_len=257, ctx=320), Case(128, 4, off=1, seq_len=257, ctx=320)]
    # six attention splits: more than the four slots of the consumer-side head merge, so attn c_proj runs merge_attn4's two-pass
    # loop (one sequence without the fused launch; a lock-step batch without planes)
    c += [Case(128, 1, off=64, seq_len=1300, ctx=1536), Case(128, 2, off=1, seq_len=1300, ctx=1536)]
    return c


CASES = _cases()


def _regime_cases():
    """The attention paths again where exp(s - m) is not 1 (score_regimes): one layer, E = 128 unless the route needs more."""
    c = []
    one = lambda *hot: [f"one-key@{p}" for p in hot]
    # one sequence, the fused launch: every regime, every hot position there is at that T (0, the ends of the first chunk of 256,
    # the row this step appends)
    for t, hot in ((6, (0, 5)), (257, (0, 255, 256)), (320, (0, 255, 256, 319))):
        c += [Case(128, 1, seq_len=t, ctx=320, regime=r) for r in ["trained", "far-below"] + one(*hot)]
    # one sequence without the fused launch: partials, merged by attn c_proj (two-pass above four splits: hot in the last and in the first)
    c += [Case(128, 1, off=64, seq_len=257, ctx=320, regime=r) for r in ["trained", "far-below"] + one(256)]
    c += [Case(128, 1, off=64, seq_len=1300, ctx=1536, regime=r) for r in ["trained"] + one(1290, 3)]
    # lock step: merged by the last split, by tag and by ticket; without planes (partials, the two-pass merge)
    c += [Case(128, 3, seq_len=257, ctx=320, regime=r) for r in ["trained"] + one(255)]
    c += [Case(128, 3, seq_len=320, ctx=320, regime=r) for r in ["trained", "far-below"] + one(319)]
    c += [Case(128, 2, off=4, seq_len=320, ctx=320, regime=r) for r in ["trained"] + one(256)]
    c += [Case(128, 2, off=1, seq_len=1300, ctx=1536, regime=r) for r in ["trained"] + one(1290, 3)]
    # the 16- and 24-bit caches, one sequence and two
    for kv, hot in (("f16", (0, 256)), ("b24", (255, 256))):
        for batch, p in zip((1, 2), hot):
            c += [Case(128, batch, kv=kv, seq_len=257, ctx=320, regime=r) for r in ["trained"] + one(p)]
    # twelve heads (48 keys: the range of six scores varies by more than the factor 60 / 8 over 96 heads, whatever the gain)
    c += [Case(768, 1, seq_len=48, regime="trained"), Case(768, 8, seq_len=48, regime="trained")]
    return c


REGIME_CASES = _regime_cases()


def make_weights(case, cfg):
    """Tensor set, shapes and init scale of synth.make_weights from numpy's generator (as fast_weights of test_full_configs_gpu);
    bf16-representable for bf16 handles, full fp32 otherwise (so that B24 and fp32 storage hold more than bf16 could); an outlier
    row and a mean-shifted row of wte; then what the case's score regime changes (score_regimes.apply)."""
    rng = np.random.default_rng(1000 + case.E + 7 * case.batch + 31 * case.off)
    w = {}
    for name, shape, mean, _ in synth.tensor_specs(cfg):
        v = rng.standard_normal(int(np.prod(shape)), dtype=np.float32) * np.float32(0.02) + np.float32(mean)
        w[name] = (synth.round_bf16(v) if case.wt == "bf16" else v).reshape(shape)
    row = rng.standard_normal(case.E, dtype=np.float32) * np.float32(2.0) + np.float32(0.3)
    w["wte"][TOK_MEAN] = synth.round_bf16(row)
    row = w["wte"][TOK_OUT].copy()
    row[rng.choice(case.E, 4, replace=False)] *= np.float32(30.0)
    w["wte"][TOK_OUT] = synth.round_bf16(row)
    if case.regime:
        assert case.layers == 1 and case.wt == "bf16", case.id
        score_regimes.apply(w, case.regime, case.E, case.seq_len, seed=case.seq_len)
    return w


def make_tokens(case):
    """(prompt [B][max(seq_len - 1, 1)], the tokens the tapped step feeds [B])."""
    B, T = case.batch, case.seq_len
    rng = np.random.default_rng(77 + T + B)
    prompt = rng.integers(TOK_LO, VOCAB - 1, size=(B, max(T - 1, 1))).astype(np.uint64)
    toks = rng.integers(TOK_LO, VOCAB - 1, size=B).astype(np.uint64)
    toks[0] = TOK_MEAN if case.off == 0 or B > 1 else TOK_OUT
    if B > 1:
        toks[1] = TOK_OUT
    name = score_regimes.parse(case.regime)[0]
    return score_regimes.same_token_rows(name, prompt, TOK_MEAN, TOK_OUT), score_regimes.same_token_rows(name, toks, TOK_MEAN, TOK_OUT)


def plan(off, M, N, K, pro, epi, wt, ops, sk_tiles, t_hi):
    """zg_debug_gemv_plan as a dict of FIELDS, with ZGPT2_DECODE_PATHS_OFF = off for the call."""
    lib = _lib.load()
    out = (C.c_int * len(FIELDS))()
    saved = os.environ.get("ZGPT2_DECODE_PATHS_OFF")
    os.environ["ZGPT2_DECODE_PATHS_OFF"] = str(off)
    try:
        _lib.check(lib.zg_debug_gemv_plan(M, N, K, pro, epi, wt, ops, sk_tiles, t_hi, out, len(FIELDS)))
    finally:
        if saved is None:
            del os.environ["ZGPT2_DECODE_PATHS_OFF"]
        else:
            os.environ["ZGPT2_DECODE_PATHS_OFF"] = saved
    return dict(zip(FIELDS, out))


def t_hi_of(case):
    return min((case.seq_len + 63) // 64 * 64, case.ctx)


def launch_rows(case, pl, st, t_hi):
    """The arguments of the five Linear launches of a step (api_gpt_step.hip *_args; base_gemv gives every launch the split-K
    workspace of n_embed / 16 tiles and the folded-LayerNorm vectors) as rows of zg_debug_gemv_plan, by launch class."""
    E, M, wt, skt = case.E, case.batch, WT[case.wt], (case.E + 15) // 16
    fed = SPLIT_K | (PLANES_IN if pl else 0)
    ln = fed | LN_FOLDED | (STATS_IN if st else 0)
    return {1: (M, 3 * E, E, PRO_LN, EPI_QKV, wt, ln, skt, t_hi),
            3: (M, E, E, PRO_NONE if pl else PRO_MERGE, EPI_RESID, wt, fed, skt, t_hi),
            4: (M, 4 * E, E, PRO_LN, EPI_GELU, wt, ln, skt, t_hi),
            5: (M, E, 4 * E, PRO_NONE, EPI_RESID, wt, fed, skt, t_hi),
            6: (M, VOCAB, E, PRO_LN, EPI_ARGMAX, wt, SPLIT_K | LN_FOLDED, skt, 0)}


def plan_case(case):
    """(modes, plans): modes = dict planes / stats / tags / fused as zg_gpt_create decides them; plans = {class: plan dict}."""
    off, E = case.off, case.E
    pl = st = False
    if case.wt == "bf16" and case.batch >= 2 and not off & 1 and E % 32 == 0:
        cand = launch_rows(case, True, False, 0)
        lin = [plan(off, *cand[k]) for k in (1, 3, 4, 5)]
        pl = all(p["can_take_planes"] for p in lin)
        st = pl and not off & 8 and E % 16 == 0 and E // 16 <= 128 and all(p["pl4_with_planes"] for p in lin)
    tags = pl and not off & 4
    rows = launch_rows(case, pl, st, t_hi_of(case))
    plans = {k: plan(off, *r) for k, r in rows.items()}
    fused = case.batch == 1 and not off & 64 and case.kv == "f32" and ROUTES[plans[1]["route"]] == "GR_LNK"
    return {"planes": int(pl), "stats": int(st), "tags": int(tags), "fused": int(fused)}, plans


def instantiation(p):
    """What of a plan names a kernel instantiation: a list of (kind, ...) keys."""
    r = ROUTES[p["route"]]
    if r in ("GR_VALU", "GR_KSPLIT", "GR_LNK"):
        keys = [("lpr_cpl", r, p["lpr"], p["cpl"])]
        return keys + [("mt", p["mt"])] if r == "GR_VALU" else keys
    if r in ("GR_MFMA16", "GR_MFMA16_KS"):
        return [("mfma16", r, p["nw"], p["ks"], p["line"], p["gpl"], p["alias"])]
    if r in ("GR_PL4", "GR_PL4_KS"):
        return [("pairs", r, p["pairs"])]
    if r == "GR_LM_WPT":
        return [("steps", p["steps"])]
    return []


def attention_operands(case):
    """float64 q [B][H][1][64] of the tapped step, K / V [B][H][T][64] and past = T - 1 from the case's own one-layer model."""
    from zig_gpt2_amd.synth import GPTConfig
    assert case.layers == 1 and case.wt == "bf16", case.id
    prompt, toks = make_tokens(case)
    T = case.seq_len
    w = make_weights(case, GPTConfig(VOCAB, case.ctx, 1, case.heads, case.E))
    q, K, V = score_regimes.qkv_of(w, np.concatenate([prompt[:, :T - 1], toks[:, None]], axis=1))
    return q[:, :, T - 1:], K, V, T - 1


def attention_how(case, modes=None):
    """How the attention of the case's step is merged, as test_decode_stages_gpu.py reports it."""
    modes = modes or plan_case(case)[0]
    if modes["planes"]:
        return "attention, merged by its last split (" + ("tagged" if modes["tags"] else "tickets") + ")"
    n_splits = (t_hi_of(case) + 255) // 256
    consumer = " (fused launch)" if modes["fused"] else ", attn c_proj's two-pass merge behind" if n_splits > 4 else ""
    return "attention partials, merged in float64" + consumer
