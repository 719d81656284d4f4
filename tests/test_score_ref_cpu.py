"""CPU checks behind zg_gpt_score: the float64 reference tests/score_ref.py the GPU tests hold the records to, and
the plan of every lm_head launch the scoring stage makes (zg_debug_prefill_plan: pure host code).

The reference: on the oracle's teacher-forced logits of a tiny model every position's log-probabilities are a distribution, and
column p + 1 is made from row p and token p + 1 — pinned by a three-token case computed by hand, against which a mapping shifted by
one either way fails.

The plans: the stage multiplies blocks of R = 256 rows (and the remainder M mod R) of ln_f(x) with wte.  bf16 weights: the first
64 floor(V / 64) rows of wte in place and a 64-row tail strip, C rows V64 = 64 ceil(V / 64) floats apart, split-K partials through
the pass's 16 M-float workspace; fp32 / B24 weights: one three-pass launch over wte's planes [3][V64][E] through a workspace of
3 R V64 floats of its own.  Every one of them must be a launch the whole-prompt Linear accepts."""
import ctypes as C
import math

import numpy as np

import oracle
from logprob_ref import logprob_all
from score_ref import score_ref
from zig_gpt2_amd import _lib, synth

PF_F32, WS, WEIGHT_PLANES = 0, 1, 33
T128, T128_WP = 2, 3
R = 256  # kScoreRows of csrc/api_gpt.h


def test_every_position_is_a_distribution():
    cfg = synth.CONFIGS["tiny"]
    w = synth.make_weights(cfg, seed=5, bf16=True)
    toks = synth.rand_tokens(17, 24, cfg.vocab_size)
    logits = oracle.GPT(cfg, w).forced_logits(toks, 0)
    assert logits.shape == (24, cfg.vocab_size)
    for p in range(24):
        assert abs(np.exp(logprob_all(logits[p])).sum() - 1.0) <= 1e-12, p
    lp, ids, top = score_ref(logits, toks, 5)
    assert np.isnan(lp[0]) and np.isfinite(lp[1:]).all() and (lp[1:] < 0).all()
    for p in range(23):
        assert lp[p + 1] == logprob_all(logits[p])[int(toks[p + 1])]
        assert np.array_equal(top[p + 1], logprob_all(logits[p])[ids[p + 1]])


def test_column_p_plus_1_uses_row_p_by_hand():
    logits = np.array([[0.0, 1.0, 2.0], [3.0, 0.0, 0.0], [0.0, 5.0, 0.0]], np.float32)
    tokens = [2, 0, 1]
    lse0 = math.log(1.0 + math.e + math.e ** 2)      # row 0
    lse1 = math.log(math.e ** 3 + 2.0)               # row 1
    want = [float(logits[0, tokens[1]]) - lse0, float(logits[1, tokens[2]]) - lse1]   # column 1: token 0 under row 0; column 2: token 1 under row 1
    lp, ids, top = score_ref(logits, tokens, 2)
    assert np.isnan(lp[0])
    assert abs(lp[1] - want[0]) <= 1e-12 and abs(lp[2] - want[1]) <= 1e-12
    assert abs(lp[1] - (0.0 - lse0)) <= 1e-12 and abs(lp[2] - (0.0 - lse1)) <= 1e-12   # the numbers themselves
    assert ids[1].tolist() == [2, 1] and ids[2].tolist() == [0, 1]                      # row 0: 2.0, 1.0; row 1: 3.0, then the tie by index
    # a mapping shifted by one either way gives other numbers: row p for column p, or row p + 1 for column p + 1
    lse2 = math.log(math.e ** 5 + 2.0)
    late = [float(logits[1, tokens[1]]) - lse1, float(logits[2, tokens[2]]) - lse2]     # column p + 1 from row p + 1
    early = [float(logits[0, tokens[2]]) - lse0]                                 # column 2 from row 0
    assert abs(lp[1] - late[0]) > 0.1 and abs(lp[2] - late[1]) > 0.1 and abs(lp[2] - early[0]) > 0.1


def plan(M, N, K, ldc, nsplit, ws_floats):
    out = (C.c_int * 21)()
    rc = _lib.load().zg_debug_prefill_plan(M, N, K, ldc, PF_F32, nsplit, ws_floats, WS, 0, 0, 0, 0, out, 21)
    assert rc == 0
    return list(out)


def test_every_lm_head_launch_of_the_scoring_stage_is_planned():
    V = 50257
    head, V64 = V // 64 * 64, (V + 63) // 64 * 64
    assert (head, V64, V - head) == (50240, 50304, 17)
    for E in (768, 1600):                                   # 124M, XL
        for tokens in (1 * 1023, 8 * 1023, 260, 130, 2, 1):      # M = batch x n_tokens rows in blocks of R
            for M in {min(R, tokens), tokens % R} - {0}:
                # bf16 weights: the pass's workspace (16 M floats; api_gpt.hip carve)
                for (N, what) in ((head, "wte in place"), (64, "the tail strip")):
                    p = plan(M, N, E, V64, 3, 16 << 20)
                    assert p[0] == 0 and p[1] == T128, (E, M, what, p)
                    if p[3]:  # split-K partials: they fit the workspace
                        assert p[9] * M * N <= 16 << 20, (E, M, what, p)
                # fp32 / B24 weights: the planes with their zero rows, one launch, the stage's own workspace
                p = plan(M, V64, E, V64, WEIGHT_PLANES, 3 * R * V64)
                assert p[0] == 0 and p[1] == T128_WP and p[3] == 1 and p[9] * M * V64 <= 3 * R * V64, (E, M, p)
    # the pass's own workspace would not do for the three-pass launch at R rows: the reason the stage has one of its own
    assert 3 * R * V64 > 16 << 20
    out = (C.c_int * 21)()
    assert _lib.load().zg_debug_prefill_plan(R, V64, 768, V64, PF_F32, WEIGHT_PLANES, 16 << 20, WS, 0, 0, 0, 0, out, 21) == 0 and out[0] != 0
