"""zg_gpt_extend on a real MI355X: the whole-prompt pass behind `past` cached positions.

prefill(toks[:p]) then extend(p, toks[p:p+n]) must leave the handle where p + n calls of GPT.forward would (src/main.zig:331-334):
the logits of position p + n - 1 and — pinning the cache rows written at the offset — the next decode step are held to the CPU
oracle with the model tolerance of golden_io.assert_model_close, the fp16 / B24 caches to the bounds tests/test_prefill_gpu.py and
tests/test_kv_b24_gpu.py apply to them.  Then the session rules: chunks in a row, a past made by the decode loop, rollback (a NaN in
a discarded row must not come back), extend(0, ...) == prefill bit for bit, and the argument errors."""
import numpy as np
import pytest

import oracle
from golden_io import assert_model_close
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu


def make(cfg, seed, **kw):
    w = synth.make_weights(cfg, seed=seed, bf16=True)
    m = zgpt.GPT(cfg, **kw)
    m.load_weights(w)
    return m, w


def rel_to_rms(expected, actual):
    rms = float(np.sqrt(np.mean(np.asarray(expected, np.float64) ** 2)))
    return float(np.abs(np.asarray(actual, np.float64) - np.asarray(expected, np.float64)).max()) / rms


def check_against_oracle(m, cfg, w, toks, end, lg, what, bound=None):
    """lg: logits [batch, V] of position end - 1; then one decode step on top of the caches.  toks [batch, >= end (+ 1)]."""
    toks = np.atleast_2d(toks)
    nxt = m.forward(end + 1, toks[:, end]) if end < cfg.context_size else None
    for b in range(toks.shape[0]):
        ref = oracle.GPT(cfg, w).forced_logits(toks[b, : min(end + 1, cfg.context_size)], end - 1)
        for got, exp, tag in ((lg, ref[0], "logits"), (nxt, ref[1] if nxt is not None else None, "next decode step")):
            if got is None:
                continue
            if bound is None:
                assert_model_close(exp, got[b], f"{what} row {b} {tag}")
            else:
                err = rel_to_rms(exp, got[b])
                assert np.isfinite(got[b]).all() and err <= bound, f"{what} row {b} {tag}: {err:.2e} of the logit scale"


@pytest.mark.parametrize("name,shapes", [("tiny", [(1, 1), (5, 4), (31, 2), (32, 32), (33, 31), (7, 25), (1, 63), (40, 24)]), ("tiny3", [(7, 41)]),
                                         ("nano-char", [(100, 156), (3, 200)]), ("xl-slice", [(40, 55)])])
def test_extend_logits_and_cache_match_oracle(zg, name, shapes):
    cfg = synth.CONFIGS[name]
    m, w = make(cfg, 171)
    for p, n in shapes:
        toks = synth.rand_tokens(1700 + 3 * p + n, min(p + n + 1, cfg.context_size), cfg.vocab_size)
        m.prefill([toks[:p]], compute_logits=False)
        lg = m.extend(p, [toks[p:p + n]])
        assert m.cached_len() == p + n
        assert int(m.argmax()[0]) == int(np.argmax(lg[0]))
        check_against_oracle(m, cfg, w, toks, p + n, lg, f"{name} extend({p}, {n})")
    m.close()


def test_three_chunks_in_a_row(zg):
    cfg = synth.CONFIGS["tiny"]
    m, w = make(cfg, 172)
    toks = synth.rand_tokens(1720, 64, cfg.vocab_size)
    m.extend(0, [toks[:9]], compute_logits=False)
    m.extend(9, [toks[9:32]], compute_logits=False)
    lg = m.extend(32, [toks[32:64]])
    assert m.cached_len() == 64
    check_against_oracle(m, cfg, w, toks, 64, lg, "9 + 23 + 32")
    m.close()


def test_extend_behind_a_past_made_by_the_decode_loop(zg):
    cfg = synth.CONFIGS["tiny"]
    m, w = make(cfg, 173)
    toks = synth.rand_tokens(1730, 50, cfg.vocab_size)
    for s in range(19):
        m.forward(s + 1, [toks[s]], compute_logits=False)
    assert m.cached_len() == 19
    lg = m.extend(19, [toks[19:49]])
    check_against_oracle(m, cfg, w, toks, 49, lg, "decode-loop past")
    m.close()


def test_extend_batched_rows_are_independent(zg):
    cfg = synth.CONFIGS["tiny"]
    m, w = make(cfg, 174, batch=3)
    toks = np.stack([synth.rand_tokens(1740 + b, 45, cfg.vocab_size) for b in range(3)])
    m.prefill(toks[:, :13], compute_logits=False)
    lg = m.extend(13, toks[:, 13:44])
    check_against_oracle(m, cfg, w, toks, 44, lg, "batch 3")
    m.close()


@pytest.mark.parametrize("route", [1, 2])
def test_extend_cache_append_epilogues_at_an_offset(zg, monkeypatch, route):
    """route 1: every Linear on the persistent GEMM (S4_QKV epilogue, with ZGPT2_GEMM_WGS=16 its hand-over between workgroups);
    route 2: the 128-row GEMM's epilogue."""
    monkeypatch.setenv("ZGPT2_GEMM_WGS", "16")
    cfg = synth.CONFIGS["nano-char"]
    m, w = make(cfg, 175, batch=4)
    toks = np.stack([synth.rand_tokens(1750 + b, 256, cfg.vocab_size) for b in range(4)])
    _lib.check(zg.zg_debug_prefill_route(route, 0))
    try:
        m.prefill(toks[:, :128], compute_logits=False)
        before = zg.zg_debug_gemm_launches()
        lg = m.extend(128, toks[:, 128:])
        took = zg.zg_debug_gemm_launches() - before
    finally:
        _lib.check(zg.zg_debug_prefill_route(0, 0))
    if route == 1:
        assert took >= 4 * cfg.n_layer, "the whole-prompt Linears did not run on gemm_s4"
    else:
        assert took == 0, "the 128-row GEMM family was expected"
    check_against_oracle(m, cfg, w, toks, 256, lg, f"route {route}")
    m.close()


def test_extend_fp32_weights(zg):
    cfg = synth.CONFIGS["tiny"]
    w = synth.make_weights(cfg, seed=176, bf16=False)
    m = zgpt.GPT(cfg, weights_f32=True)
    m.load_weights(w)
    toks = synth.rand_tokens(1760, 64, cfg.vocab_size)
    m.prefill([toks[:33]], compute_logits=False)
    lg = m.extend(33, [toks[33:64]])
    check_against_oracle(m, cfg, w, toks, 64, lg, "fp32 weights")
    m.close()


# the bounds those cache modes are held to today: fp16 1e-3 of the logit scale (test_prefill_gpu.py), B24 1e-4 (test_kv_b24_gpu.py)
@pytest.mark.parametrize("mode,bound", [("kv_f16", 1e-3), ("kv_b24", 1e-4)])
@pytest.mark.parametrize("name,p,n", [("tiny", 33, 30), ("nano-char", 100, 155)])
def test_extend_reads_the_past_from_fp16_and_b24_caches(zg, name, p, n, mode, bound):
    """Two lengths each: n + 1 = (33, 31) / (100, 156) ends at the context's last position (logits only), n is one row shorter so that
    the decode step behind the pass exists too."""
    cfg = synth.CONFIGS[name]
    m, w = make(cfg, 177, **{mode: True})
    for nn in (n, n + 1):
        toks = synth.rand_tokens(1770 + nn, min(p + nn + 1, cfg.context_size), cfg.vocab_size)
        m.prefill([toks[:p]], compute_logits=False)
        lg = m.extend(p, [toks[p:p + nn]])
        check_against_oracle(m, cfg, w, toks, p + nn, lg, f"{name} {mode} extend({p}, {nn})", bound)
    m.close()


def test_rollback_discards_the_tail(zg):
    cfg = synth.CONFIGS["tiny"]
    m, w = make(cfg, 178)
    toks = synth.rand_tokens(1780, 40, cfg.vocab_size)
    other = synth.rand_tokens(1781, 12, cfg.vocab_size)
    seq = np.concatenate([toks[:20], other[:11]])
    m.prefill([toks], compute_logits=False)
    lg = m.extend(20, [other[:10]])
    assert m.cached_len() == 30
    fresh, _ = make(cfg, 178)
    lg_fresh = fresh.prefill([seq[:30]])
    assert_model_close(lg_fresh[0], lg[0], "rollback against prefill of the 30-token sequence")
    assert_model_close(fresh.forward(31, [seq[30]])[0], m.forward(31, [seq[30]])[0], "decode step behind the rollback")
    fresh.close()
    check_against_oracle(m, cfg, w, seq, 30, lg, "rollback")
    m.close()


def test_a_nan_in_a_discarded_row_does_not_come_back(zg):
    """The NaN is made by the model itself: on an fp32-weight handle, 35 clean positions, then ONE decode step at position 35 with a
    wpe whose row 35 is NaN — the step appends a NaN row 35 to every layer's caches and touches no other row (a whole-prompt pass
    over the NaN would not do: a masked 0 x NaN in its attention spoils the rows in front of it as well).  With the weights repaired, a
    rollback to 20 and ten other tokens must clear the rows behind position 29: the decode attention reads its whole 64-position
    bucket, and 0 x NaN would poison every later step — checked up to the bucket's (and the context's) end."""
    cfg = synth.CONFIGS["tiny"]
    w = synth.make_weights(cfg, seed=179, bf16=False)
    bad = dict(w)
    bad["wpe"] = np.array(w["wpe"], np.float32, copy=True).reshape(cfg.context_size, cfg.n_embed)
    bad["wpe"][35] = np.nan
    m = zgpt.GPT(cfg, weights_f32=True)
    m.load_weights(w)
    toks = synth.rand_tokens(1790, 40, cfg.vocab_size)
    m.prefill([toks[:35]], compute_logits=False)
    m.load_weights(bad)
    assert not np.isfinite(m.forward(36, [toks[35]])).any(), "the planted NaN did not reach the model"
    m.load_weights(w)
    assert not np.isfinite(m.forward(37, [toks[36]])).any(), "the NaN is not in the cache"
    assert m.cached_len() == 37
    seq = np.concatenate([toks[:20], synth.rand_tokens(1791, 44, cfg.vocab_size)])
    lg = m.extend(20, [seq[20:30]])
    assert m.cached_len() == 30
    ref = oracle.GPT(cfg, w).forced_logits(seq, 29)
    assert_model_close(ref[0], lg[0], "logits behind the rollback")
    for s in range(30, 64):
        out = m.forward(s + 1, [seq[s]], compute_logits=s in (30, 35, 62, 63))
        if out is not None:
            assert_model_close(ref[s - 29], out[0], f"decode step at position {s}")
    m.close()


def test_extend_at_zero_is_prefill(zg):
    cfg = synth.CONFIGS["tiny"]
    m, _ = make(cfg, 180, batch=2)
    toks = np.stack([synth.rand_tokens(1800 + b, 37, cfg.vocab_size) for b in range(2)])
    a = m.prefill(toks).copy()
    b = m.extend(0, toks)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    m.close()


def test_extend_errors_leave_the_handle_usable(zg):
    cfg = synth.CONFIGS["tiny"]
    m, w = make(cfg, 181)
    toks = synth.rand_tokens(1810, 31, cfg.vocab_size)
    m.prefill([toks[:10]], compute_logits=False)
    for past, new in ((11, toks[10:12]), (10, np.zeros(55, np.uint64)), (10, np.zeros(0, np.uint64)), (10, np.array([1, cfg.vocab_size], np.uint64))):
        with pytest.raises(_lib.ZgError):
            m.extend(past, [new])
        assert m.cached_len() == 10
    lg = m.extend(10, [toks[10:30]])
    check_against_oracle(m, cfg, w, toks, 30, lg, "after the refused calls")
    m.close()
    m, _ = make(cfg, 181, prefill=False)
    m.forward(1, [toks[0]], compute_logits=False)
    with pytest.raises(_lib.ZgError) as e:
        m.extend(1, [toks[1:9]])
    assert e.value.code == -5 and "NO_PREFILL" in str(e.value)
    assert np.isfinite(m.forward(2, [toks[1]])).all()
    m.close()
