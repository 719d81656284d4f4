"""The cases of the pass-stage tests and what the library plans for them, without a GPU.

A case is one small model, one batch, one storage choice, one route pin (zg_debug_prefill_route), one ZGPT2_GEMM_WGS value and one
whole-prompt pass: n new positions behind past_len cached ones, plain or with the score stage.  plan_case() predicts every GEMM
launch of the pass with zg_debug_prefill_plan from the arguments enqueue_prefill / enqueue_score of api_gpt_pass.hip lay out, and the
attention's kernel and key-range geometry from launch_attn_prefill's rule; test_pass_stages_gpu.py holds the plans the tapped pass
reports (zg_debug_gpt_pass_taps) to these predictions, so the coverage test_pass_stage_cases_cpu.py asserts on the CPU is the
coverage the GPU test runs."""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from test_prefill_plan_cpu import FIELDS, LN, PF_F32, PF_GELU_SPLIT, PF_QKV, PF_RESID, QKV, SK_FLAGS, SK_WS, WEIGHT_PLANES, WS

import score_regimes
from zig_gpt2_amd import _lib, synth

VOCAB = 333      # on the score GEMM's grid: 320 rows of wte in place and a strip of 13
V64 = 384
TOK_MEAN, TOK_OUT = VOCAB - 3, VOCAB - 4  # wte rows with mean 0.3 / std 2, and with a few 30 x outlier channels
TOK_LO = VOCAB // 2
SCORE_ROWS = 256
FAMILY = {1: "S4", 2: "T128", 3: "T128_WP"}
TAIL = {0: "NO_TAIL", 1: "LN_SPLIT", 2: "REDUCE", 3: "REDUCE_LN_SPLIT", 4: "REDUCE_RESID_LN"}
CLASS_NAMES = {2: "c_attn", 4: "attn c_proj", 5: "c_fc + GELU", 6: "mlp c_proj", 7: "lm_head"}


@dataclass(frozen=True)
class Case:
    E: int
    batch: int
    n: int              # new positions per sequence
    past: int = 0       # cached positions in front (a plain extend of the front part runs first)
    layers: int = 1
    wt: str = "bf16"    # weights: bf16, f32, b24
    kv: str = "f32"     # cache: f32, f16, b24
    planes: int = 3     # activation planes multiplied (2: ZG_GPT_PREFILL_2PLANE)
    pin: tuple = (0, 0)  # zg_debug_prefill_route(kernel, slices)
    wgs: int = 0        # ZGPT2_GEMM_WGS, 0 = unset
    score: bool = False
    logits: bool = True  # compute_logits (False: the last Block stops behind its cache append)
    ctx: int = 0        # 0: past + n + 8
    twice: bool = False  # the tapped pass runs a second time on the same handle (the stream-K flags carry an epoch)
    regime: str = ""     # the attention scores' regime (score_regimes): "" = N(0, 0.02) weights, "trained", "one-key@P", "far-below"

    @property
    def id(self):
        tail = ("-score" if self.score else "") + ("" if self.logits else "-nologits") + (f"-wgs{self.wgs}" if self.wgs else "") + ("-x2" if self.twice else "")
        tail += f"-{self.regime}" if self.regime else ""
        return f"E{self.E}-L{self.layers}-b{self.batch}-n{self.n}-p{self.past}-{self.wt}-kv{self.kv}-pl{self.planes}-pin{self.pin[0]}.{self.pin[1]}{tail}"

    @property
    def heads(self):
        return self.E // 64

    @property
    def M(self):
        return self.batch * self.n

    @property
    def context(self):
        return self.ctx or self.past + self.n + 8


def _cases():
    c = []
    # E 128: both families for every role, the row counts around the 128- and 256-row tiles, the attention's ranges
    c += [Case(128, 2, 64, layers=2, pin=(1, 0)),                       # M 128; the persistent kernel, sliced by its rule
          Case(128, 2, 64, layers=2, pin=(2, 0), logits=False),         # ... the 128-row kernel; the last Block stops behind its append
          Case(128, 3, 43, layers=2, pin=(2, 0)),                       # M 129
          Case(128, 1, 1),                                              # M 1, the library's rule
          Case(128, 1, 127, pin=(2, 0), kv="f16"),                      # M 127; a whole prompt on an fp16 cache
          Case(128, 3, 85, pin=(1, 4)),                                 # M 255; mlp c_proj in four slices
          Case(128, 2, 128, layers=2, pin=(2, 0), wt="f32"),            # M 256; the three-pass kernel
          Case(128, 2, 128, pin=(1, 1)),                                # M 256; one slice
          Case(128, 1, 257, layers=2, pin=(1, 0), kv="b24"),            # M 257; split key ranges + merge; a whole prompt on a B24 cache
          Case(128, 1, 320, layers=2, ctx=320),                         # the whole context, split key ranges on the fp32 cache
          Case(128, 5, 51, pin=(2, 0), wt="b24", kv="f16")]             # M 255, B24 weights
    # continuations on each cache format: n = 1, the end of the context, ranges that cross into the second group
    c += [Case(128, 2, 1, past=127, layers=2, kv="f16", ctx=128),
          Case(128, 2, 70, past=60, pin=(1, 0), ctx=160),
          Case(384, 3, 43, past=33, pin=(2, 0), kv="b24", ctx=76),
          Case(128, 1, 120, past=200, layers=2, kv="f16", ctx=320),
          Case(128, 2, 1, past=5, kv="b24", wt="f32")]
    # E 384: K slices 2 and 3, fp32 / B24 weights on the persistent kernel, the stream-K hand-over, two planes
    c += [Case(384, 2, 64, layers=2, pin=(1, 0), wt="b24", kv="b24"),
          Case(384, 3, 43, pin=(1, 2)),
          Case(384, 2, 64, pin=(1, 3)),
          Case(384, 1, 257, pin=(2, 0), kv="f16"),
          Case(384, 4, 256, pin=(1, 0), wgs=16, twice=True),            # 24 tiles of c_attn on 16 workgroups: the hand-over
          Case(384, 2, 64, pin=(2, 0), planes=2),
          Case(384, 2, 100, pin=(1, 0), planes=2)]
    # E 768 under both pins and with fp32 weights; E 1600 once: 8.33 column tiles of 192
    c += [Case(768, 2, 64, pin=(1, 0)), Case(768, 3, 43, pin=(2, 0)), Case(768, 2, 30, pin=(2, 0), wt="f32"), Case(768, 2, 65, pin=(1, 0), wt="f32", kv="f16"),
          Case(768, 1, 128, pin=(1, 4)), Case(1600, 1, 70, pin=(1, 0))]
    # the score stage: below one block, crossing a block, each weight type, behind cached positions
    c += [Case(128, 2, 40, score=True), Case(128, 2, 130, layers=2, score=True, pin=(2, 0)), Case(128, 1, 50, score=True, wt="f32", pin=(1, 0)),
          Case(384, 2, 130, score=True, wt="b24", kv="f16"), Case(128, 3, 20, past=10, score=True, kv="b24", planes=2)]
    return c


CASES = _cases()


def plan(wgs, *args):
    """zg_debug_prefill_plan as a dict of FIELDS, with ZGPT2_GEMM_WGS = wgs (0: unset) for the call."""
    lib = _lib.load()
    out = (C.c_int * len(FIELDS))()
    saved = os.environ.get("ZGPT2_GEMM_WGS")
    if wgs:
        os.environ["ZGPT2_GEMM_WGS"] = str(wgs)
    else:
        os.environ.pop("ZGPT2_GEMM_WGS", None)
    try:
        _lib.check(lib.zg_debug_prefill_plan(*args, out, len(FIELDS)))
    finally:
        if saved is None:
            os.environ.pop("ZGPT2_GEMM_WGS", None)
        else:
            os.environ["ZGPT2_GEMM_WGS"] = saved
    return dict(zip(FIELDS, out))


def pf_ws_floats(case):
    """zg_gpt_create: 16 M floats for bf16 weights, else room for three weight-plane passes of [B ctx][4 E] at the least."""
    return 16 << 20 if case.wt == "bf16" else max(16 << 20, 3 * case.batch * case.context * 4 * case.E)


def nsplit(case):
    return WEIGHT_PLANES if case.wt != "bf16" else case.planes


def gemm_rows(case):
    """The GEMM launches of the pass in launch order: [(class, layer or score block, role, zg_debug_prefill_plan arguments)]."""
    E, M, L, ws, np_, pin = case.E, case.M, case.layers, pf_ws_floats(case), nsplit(case), case.pin
    sk = case.wt == "bf16"  # the stream-K operands: the workspace itself and 512 flag words
    rows = []
    for l in range(L):
        rows.append((2, l, "c_attn", (M, 3 * E, E, 3 * E, PF_QKV, np_, ws, WS | QKV | (SK_WS | SK_FLAGS if sk else 0), ws * 4 if sk else 0, 512 if sk else 0, *pin)))
        if l + 1 == L and not (case.logits or case.score):
            break
        rows.append((4, l, "attn c_proj", (M, E, E, E, PF_RESID, np_, ws, WS | LN, 0, 0, *pin)))
        rows.append((5, l, "c_fc", (M, 4 * E, E, 0, PF_GELU_SPLIT, np_, ws, WS, 0, 0, *pin)))
        rows.append((6, l, "mlp c_proj", (M, E, 4 * E, E, PF_RESID, np_, ws, WS | (LN if l + 1 < L else 0), 0, 0, *pin)))
    if case.score:
        for blk, r0 in enumerate(range(0, M, SCORE_ROWS)):
            r = min(SCORE_ROWS, M - r0)
            if case.wt != "bf16":
                rows.append((7, blk, "lm_head", (r, V64, E, V64, PF_F32, WEIGHT_PLANES, 3 * SCORE_ROWS * V64, WS, 0, 0, *pin)))
            else:
                rows.append((7, blk, "lm_head", (r, VOCAB // 64 * 64, E, V64, PF_F32, case.planes, ws, WS, 0, 0, *pin)))
                rows.append((7, blk, "lm_head strip", (r, 64, E, V64, PF_F32, case.planes, ws, WS, 0, 0, *pin)))
    return rows


def attention_plan(case):
    """launch_attn_prefill's rule (attn_prefill.hip): (kernel, key tiles per range, max splits, query groups).  kernel 0: the
    whole-prompt kernel (nothing cached in front, and the K / V rows readable as fp32: the fp32 cache, or the qkv columns on a 16- /
    24-bit cache); 1 / 2 / 3: the continuation kernel on an fp32 / fp16 / B24 cache."""
    B, H, P, pos0 = case.batch, case.heads, case.n, case.past
    kernel = 0 if pos0 == 0 else 1 + ("f32", "f16", "b24").index(case.kv)
    ng, nkt = ((P + 31) // 32 + 3) // 4, (pos0 + P + 31) // 32
    tiles = lambda g: (pos0 + min(128 * (g + 1), P) + 31) >> 5
    splits = lambda g, nts: (tiles(g) + nts - 1) // nts
    nts = cand = 32 * ((nkt + 31) // 32)
    while cand >= 4:
        nts = cand
        if sum(splits(g, cand) for g in range(ng)) * B * H >= 512 or B * H * ng >= 256:
            break
        cand //= 2
    nts = min(nts, 255)
    max_s = splits(ng - 1, nts)
    assert max_s == 1 or B * H * P * max_s * 66 <= pf_ws_floats(case)
    return kernel, nts, max_s, ng


def first_range_last_key(case):
    """The last key of the attention's first key range: its ranges are attention_plan's key tiles per range of 32 keys each."""
    return 32 * attention_plan(case)[1] - 1


def _regime_cases():
    """The attention paths again where exp(s - m) is not 1 (score_regimes): one layer, E = 128 unless the route pin asks for more.
    Hot keys of one-key: position 0 (every row's sink), the last key of the first key range, a key among the cached ones."""
    c = []

    def add(base, *regimes):
        for r in regimes:
            hot = {"one-key@range": f"one-key@{first_range_last_key(base)}"}.get(r, r)
            c.append(Case(**{**base.__dict__, "regime": hot}))

    add(Case(128, 2, 64, pin=(1, 0)), "trained", "one-key@0", "far-below")                          # one range
    add(Case(128, 1, 257, pin=(1, 0)), "trained", "one-key@0", "one-key@range", "one-key@200")      # split ranges + merge (200: in the second range)
    add(Case(128, 1, 320, ctx=320), "trained", "one-key@range")                                     # ... the whole context
    add(Case(128, 2, 70, past=60, pin=(1, 0), ctx=160), "trained", "one-key@30")                    # the continuation kernel, fp32 cache
    add(Case(128, 1, 120, past=200, kv="f16", ctx=320), "trained", "one-key@0", "one-key@range")    # ... fp16 cache, ranges merged
    add(Case(128, 2, 43, past=33, pin=(2, 0), kv="b24", ctx=76), "trained", "one-key@10")           # ... B24 cache
    add(Case(128, 2, 1, past=127, kv="f16", ctx=128), "trained", "one-key@0")                       # n = 1 at the end of the context
    add(Case(384, 2, 64, pin=(1, 0)), "trained")                                                    # six heads under each route pin
    add(Case(384, 3, 43, pin=(2, 0)), "trained")
    return c


REGIME_CASES = _regime_cases()


def make_weights(case, cfg):
    """As make_weights of decode_stage_cases.py: the tensor set, shapes and init scale of synth.make_weights from numpy's
    generator; bf16-representable for bf16 handles, full fp32 otherwise; an outlier row and a mean-shifted row of wte; then what
    the case's score regime changes (score_regimes.apply)."""
    rng = np.random.default_rng(2000 + case.E + 7 * case.batch + 31 * case.n + case.past)
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
        score_regimes.apply(w, case.regime, case.E, case.past + case.n, seed=case.past + case.n)
    return w


def make_tokens(case):
    """(the tokens of positions 0 .. past + n - 1 [B][past + n], the generator the GPU test draws its step on top from)."""
    B, n, past = case.batch, case.n, case.past
    rng = np.random.default_rng(99 + n + B)
    toks = rng.integers(TOK_LO, VOCAB - 1, size=(B, past + n)).astype(np.uint64)
    toks[0, past] = TOK_MEAN
    toks[B - 1, past + n - 1] = TOK_OUT if B * n > 1 else TOK_MEAN
    return score_regimes.same_token_rows(score_regimes.parse(case.regime)[0], toks, TOK_MEAN, TOK_OUT), rng


def plan_case(case):
    """([(class, layer, role, plan dict)] of every GEMM launch in launch order, the attention's plan)."""
    return [(cls, l, role, plan(case.wgs, *args)) for cls, l, role, args in gemm_rows(case)], attention_plan(case)


def outcome(role, p):
    """What the coverage assertion counts of a planned launch, as test_prefill_plan_cpu.outcome names it."""
    if p["family"] == 1:
        return ("S4", p["s4_kind"], p["stream_k"], p["slices"], TAIL[p["tail"]])
    return (FAMILY[p["family"]], "partial" if p["partial"] else "whole", p["ns"], p["nspl"], TAIL[p["tail"]])


def pass_route(p):
    """The name a planned launch goes by in stage_ref.BOUND_Y and in the GPU test's report."""
    if p["family"] == 1:
        return f"PF_S4 ({p['npairs']} plane pairs, {p['slices']} K slice(s){', stream-K' if p['stream_k'] else ''})"
    return f"PF_{FAMILY[p['family']]} ({'through the workspace' if p['partial'] else 'whole'}" + (f", {p['nspl']} planes)" if p["nspl"] else ")")


def attention_operands(case):
    """float64 q [B][H][n][64] of the pass's new positions, K / V [B][H][past + n][64] and past from the case's own one-layer model."""
    from zig_gpt2_amd.synth import GPTConfig
    assert case.layers == 1 and case.wt == "bf16", case.id
    w = make_weights(case, GPTConfig(VOCAB, case.context, 1, case.heads, case.E))
    q, K, V = score_regimes.qkv_of(w, make_tokens(case)[0])
    return q[:, :, case.past:], K, V, case.past


def attention_how(case, att=None):
    """The attention's kernel and ranges, as test_pass_stages_gpu.py reports them."""
    att = att or attention_plan(case)
    return ("whole-prompt kernel" if att[0] == 0 else f"continuation kernel, {case.kv} cache") + (f", {att[2]} ranges merged" if att[2] > 1 else ", one range")
