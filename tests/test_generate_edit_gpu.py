"""zg_gpt_generate_request_enqueue with edits: the device loop with the edit stage in its captured step equals, token for token, the
host loop over zg_gpt_sample_edit (include/zgpt2.h), in all four sampler forms — plain, one filter, two filters, min-p alone — and
combined with penalties, log-probabilities and stop conditions; without edits it is zg_gpt_generate_stop_enqueue bit for bit.

The model has gpt_tiny's shapes with a context of 96, so that 80 steps cross a 64-position bucket; ragged prompts of 1 + 2 (b mod 3)
tokens make the loop leave and re-enter the alignment of its multi-step graphs.  The log-probability record is held to
logprob_ref on edit_ref.edit_row of the device's own raw logits (zg_gpt_forward at the same position), within DESIGN §3.7's bound."""
import ctypes as C

import numpy as np
import pytest

from edit_ref import edit_row
from logprob_ref import check_values, logprob_ref
from penalty_ref import penalize_row
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu
CFG = synth.GPTConfig(257, 96, 2, 2, 128)
V = CFG.vocab_size
N_STEPS = 80
PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.15)
# temp, top_k, top_p, min_p: plain, one filter, two filters (+ min-p), min-p alone
FORMS = [(0.8, 0, 1.0, 0.0), (0.8, 7, 1.0, 0.05), (1.1, 12, 0.8, 0.02), (0.8, 0, 1.0, 0.05)]
EDITS = dict(logit_bias={3: 2.5, 100: -4.0, 0: 1.0, V - 1: 0.5, 41: 3.0}, banned_token_ids=[7, 41, 200, 7])


@pytest.fixture(scope="module")
def weights():
    return synth.make_weights(CFG, seed=81, bf16=True)


def make(w, batch, **kw):
    m = zgpt.GPT(CFG, batch=batch, **kw)
    m.load_weights(w)
    return m


def ragged(batch, seed):
    return [synth.rand_tokens(seed + b, 1 + 2 * (b % 3), V) for b in range(batch)]


def host_loop(m, prompts, n_steps, temp, seed, top_k, top_p, min_p, edits, pen=None, past=0, prior=None, rows=None):
    """generate's token logic around zg_gpt_sample_edit (test_generate_pen_gpu.host_loop with the edits): the row's own prompt token
    is fed while the prompt lasts, its last one twice.  rows (a dict): step -> the reference's edited row of every sequence, from
    the device's own raw logits at that step."""
    B = len(prompts)
    out = np.zeros((B, n_steps), np.uint64)
    draws = [0] * B
    min_np = min(len(p) for p in prompts)
    for i in range(n_steps):
        toks = [int(p[i]) if i < len(p) else (int(p[-1]) if i == len(p) else int(draws[b])) for b, p in enumerate(prompts)]
        if i >= min_np:
            hist = [np.r_[np.asarray([] if prior is None else prior[b], np.uint64), out[b, :i]] for b in range(B)]
            if rows is not None:
                raw = m.forward(past + i + 1, toks)
                base = [penalize_row(raw[b], hist[b], 1.3, 0.4, 0.15)[0] if pen else raw[b] for b in range(B)]
                rows[i] = [edit_row(base[b], edits.get("logit_bias"), edits.get("allowed_token_ids"), edits.get("banned_token_ids")) for b in range(B)]
            draws = m.sample(past + i + 1, toks, temp, seed=seed, top_k=top_k, top_p=top_p, min_p=min_p, history=hist if pen else None, **(pen or {}), **edits)
        else:
            m.forward(past + i + 1, toks, compute_logits=False)
        for b, p in enumerate(prompts):
            out[b, i] = toks[b] if i < len(p) else draws[b]
    return out


@pytest.mark.parametrize("batch,graph,at_create", [(1, True, False), (1, False, False), (3, True, True)])
def test_device_loop_equals_host_loop(zg, weights, batch, graph, at_create):
    prompts = ragged(batch, 910)
    m = make(weights, batch, use_graph=graph, edited_generate=at_create)
    plain = m.generate_sample(prompts, N_STEPS, 0.8, seed=5)
    for (temp, k, p, mp), seed in zip(FORMS, (5, 123456789, 9, 77)):
        got = m.generate_sample(prompts, N_STEPS, temp, seed=seed, top_k=k, top_p=p, min_p=mp, **EDITS)
        want = host_loop(m, prompts, N_STEPS, temp, seed, k, p, mp, EDITS)
        again = m.generate_sample(prompts, N_STEPS, temp, seed=seed, top_k=k, top_p=p, min_p=mp, **EDITS)
        assert np.array_equal(got, want), (k, p, mp, np.argwhere(got != want)[:4])
        assert np.array_equal(got, again)
        for b, pr in enumerate(prompts):
            assert np.array_equal(got[b, : len(pr)], pr)
            assert not set(int(t) for t in got[b, len(pr):]) & {7, 41, 200}, "a banned token was picked"
    # min-p alone, no edit stage
    got = m.generate_sample(prompts, N_STEPS, 0.8, seed=6, min_p=0.3)
    assert np.array_equal(got, host_loop(m, prompts, N_STEPS, 0.8, 6, 0, 1.0, 0.3, {}))
    assert not np.array_equal(m.generate_sample(prompts, N_STEPS, 0.8, seed=5, **EDITS), plain), "the edits changed nothing"
    assert np.array_equal(m.generate_sample(prompts, N_STEPS, 0.8, seed=5), plain), "an ordinary generation behind edited ones"
    m.close()


def test_no_prefill_handle_and_a_continuation(zg, weights):
    B, past, n = 2, 13, 60
    first = np.stack([synth.rand_tokens(920 + b, past, V) for b in range(B)])
    turns = [synth.rand_tokens(930 + b, 2 + 3 * b, V) for b in range(B)]
    allowed = sorted(int(t) for t in np.random.default_rng(5).choice(V, 30, replace=False))
    edits = dict(logit_bias={allowed[0]: 1.5, allowed[3]: -2.0}, allowed_token_ids=allowed, banned_token_ids=[allowed[1]])
    for kw in (dict(), dict(prefill=False)):
        m = make(weights, B, **kw)
        feed = (lambda: m.extend(0, first, compute_logits=False)) if not kw else (lambda: m.generate(list(first), past))
        feed()
        got = m.generate_from(past, turns, n, temp=0.8, seed=21, top_k=9, top_p=0.9, min_p=0.05, **edits)
        assert m.cached_len() == past + n
        feed()
        want = host_loop(m, turns, n, 0.8, 21, 9, 0.9, 0.05, edits, past=past)
        assert np.array_equal(got, want), (kw, np.argwhere(got != want)[:4])
        for b, t in enumerate(turns):
            assert set(int(x) for x in got[b, len(t):]) <= set(allowed) - {allowed[1]}, "a pick outside the allow-list"
        # a fresh generation on the same handle, long prompts (the whole-prompt pass where the handle has one)
        prompts = [synth.rand_tokens(940 + b, 6 + b, V) for b in range(B)]
        got = m.generate_sample(prompts, 50, 0.8, seed=4, min_p=0.05, **edits)
        assert np.array_equal(got, host_loop(m, prompts, 50, 0.8, 4, 0, 1.0, 0.05, edits))
        m.close()


def test_with_penalties_logprobs_and_stop_conditions(zg, weights):
    B, n, top_n = 3, 40, 8
    prompts = ragged(B, 950)
    allowed = [5, 17, 60, 130, 255]
    edits = dict(logit_bias={17: 1.0, 130: -1.0, 99: 5.0}, allowed_token_ids=allowed)  # (99 is biased and not allowed: it stays -inf)
    m = make(weights, B)
    got, lp, ids, top = m.generate_sample(prompts, n, 1.3, seed=8, top_k=4, min_p=0.02, logprobs=top_n, **PEN, **edits)
    rows = {}
    want = host_loop(m, prompts, n, 1.3, 8, 4, 1.0, 0.02, edits, pen=PEN, rows=rows)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    worst = 0.0
    for b, p in enumerate(prompts):
        assert np.isnan(lp[b, : len(p)]).all()
        for s in range(len(p), n):
            assert int(got[b, s]) in allowed
            r_lp, r_ids, r_top = logprob_ref(rows[s][b], got[b, s], top_n)
            worst = max(worst, check_values(lp[b, s], r_lp), check_values(top[b, s], r_top))
            assert np.array_equal(ids[b, s].astype(np.int64), r_ids), (b, s, ids[b, s], r_ids)
            assert sorted(int(i) for i in ids[b, s, :5]) == allowed and np.isneginf(top[b, s, 5:]).all()  # -inf where not kept
    assert worst <= 1.0
    # stop conditions on top: the same tokens, cut at the end; the record too
    stop_tok = int(got[0, len(prompts[0]) + 3])
    cut, lp2, ids2, top2 = m.generate_sample(prompts, n, 1.3, seed=8, top_k=4, min_p=0.02, logprobs=top_n, stop_token_ids=[stop_tok, allowed[0]], stop=[[allowed[1], allowed[2]]],
                                             **PEN, **edits)
    end, fin, _ = m.stop_result()
    assert cut.shape[1] == end and np.array_equal(cut, got[:, :end])
    assert np.array_equal(lp2.view(np.uint32), lp[:, :end].view(np.uint32)) and np.array_equal(ids2, ids[:, :end]) and np.array_equal(
        top2.view(np.uint32), top[:, :end].view(np.uint32))
    assert fin[0] is not None and fin[0] <= len(prompts[0]) + 3
    m.close()


def raw_request(zg, m, prompts, n, opt, pen, logprobs, top_n, conds, edits, seed=3, past=0):
    mat, lens, stride = m._prompts(prompts)
    r = _lib.generate_request(past_len=past, prompts=_lib.ptr(mat), prompt_stride=stride, prompt_lens=_lib.ptr(lens), n_steps=n,
                              options=None if opt is None else C.addressof(opt), penalties=None if pen is None else C.addressof(pen), seed=seed,
                              logprobs=logprobs, top_n=top_n, stop=None if conds is None else C.addressof(conds), edits=None if edits is None else C.addressof(edits))
    return zg.zg_gpt_generate_request_enqueue(m.h, C.addressof(r))


def test_without_edits_it_is_generate_stop_enqueue_bit_for_bit(zg, weights):
    B, n, top_n = 3, N_STEPS, 3
    prompts = ragged(B, 960)
    m = make(weights, B)
    mat, lens, stride = m._prompts(prompts)
    pen, off = _lib.LogitPenalties(1.3, 0.4, 0.15), _lib.LogitEdits()
    probe = m.generate_sample(prompts, n, 0.8, seed=3, top_k=7, top_p=0.9, **PEN)
    conds, keep = _lib.stop_conditions([int(probe[b, 20 + 5 * b]) for b in range(B)], None, 0)
    for opt, pn in ((_lib.SampleOptions(0.8, 7, 0.9), pen), (_lib.SampleOptions(0.8, 0, 1.0), None), (None, None)):
        res = []
        for edits in ("twin", None, off):
            if edits == "twin":
                rc = zg.zg_gpt_generate_stop_enqueue(m.h, 0, _lib.ptr(mat), stride, _lib.ptr(lens), n, None if opt is None else C.addressof(opt),
                                                     None if pn is None else C.addressof(pn), None, 0, None, 3, 1, top_n, C.addressof(conds))
            else:
                rc = raw_request(zg, m, prompts, n, opt, pn, 1, top_n, conds, edits)
            assert rc == 0
            end, fin, why = m.stop_result()
            res.append((end, fin, why, m.generate_fetch_range(0, end)) + m.generate_fetch_logprobs(0, end, top_n))
        for other in res[1:]:
            # (`end` may differ from run to run inside its bound, nothing else may: compare what both hold)
            e = min(res[0][0], other[0])
            assert res[0][1] == other[1] and res[0][2] == other[2]
            assert np.array_equal(res[0][3][:, :e], other[3][:, :e])
            assert np.array_equal(res[0][4][:, :e].view(np.uint32), other[4][:, :e].view(np.uint32))
            picked = ~np.isnan(res[0][4][:, :e])  # (the ids of a column that records a prompt token mean nothing)
            assert np.array_equal(res[0][5][:, :e][picked], other[5][:, :e][picked])
            assert np.array_equal(res[0][6][:, :e][picked].view(np.uint32), other[6][:, :e][picked].view(np.uint32))
    # no conditions either: the plain calls
    opt = _lib.SampleOptions(0.8, 7, 0.9)
    want = m.generate_sample(prompts, n, 0.8, seed=3, top_k=7, top_p=0.9)
    assert raw_request(zg, m, prompts, n, opt, None, 0, 0, None, off) == 0
    assert np.array_equal(m.generate_fetch(n), want)
    assert raw_request(zg, m, prompts, n, None, None, 0, 0, None, None) == 0
    assert np.array_equal(m.generate_fetch(n), m.generate(prompts, n))
    del keep
    m.close()


def test_refusals_leave_the_handle_and_the_record_alone(zg, weights):
    B, n = 2, 24
    prompts = ragged(B, 970)
    m = make(weights, B)
    got, lp, ids, top = m.generate_sample(prompts, n, 0.8, seed=2, top_k=5, logprobs=2, banned_token_ids=[1])
    assert m.cached_len() == n
    opt = _lib.SampleOptions(0.8, 5, 1.0)
    big = np.arange(600, dtype=np.uint64)
    vals = np.ones(600, np.float32)
    dup = np.array([4, 9, 4], np.uint64)
    nonfin = np.array([1.0, np.inf, 0.0], np.float32)
    over = np.array([V], np.uint64)
    every = np.arange(V, dtype=np.uint64)
    P = _lib.ptr
    cases = [
        (_lib.LogitEdits(P(big), P(vals), 513, None, 0, None, 0, 0.0), opt, -6),
        (_lib.LogitEdits(P(dup), P(vals), 3, None, 0, None, 0, 0.0), opt, -6),
        (_lib.LogitEdits(P(big), P(nonfin), 3, None, 0, None, 0, 0.0), opt, -6),
        (_lib.LogitEdits(None, None, 0, None, 0, None, 0, 1.0), opt, -6),
        (_lib.LogitEdits(None, None, 0, None, 0, None, 0, float("nan")), opt, -6),
        (_lib.LogitEdits(None, None, 0, None, 3, None, 0, 0.0), opt, -6),
        (_lib.LogitEdits(None, None, 0, None, 0, P(every), V, 0.0), opt, -6),
        (_lib.LogitEdits(None, None, 0, P(dup), 3, P(dup), 3, 0.0), opt, -6),
        (_lib.LogitEdits(None, None, 0, None, 0, P(dup), 3, 0.0), None, -6),       # greedy with an edit on
        (_lib.LogitEdits(None, None, 0, None, 0, None, 0, 0.1), None, -6),
        (_lib.LogitEdits(P(over), P(vals), 1, None, 0, None, 0, 0.0), opt, -2),
        (_lib.LogitEdits(None, None, 0, P(over), 1, None, 0, 0.0), opt, -2),
        (_lib.LogitEdits(None, None, 0, None, 0, P(over), 1, 0.0), opt, -2),
    ]
    for e, o, code in cases:
        assert raw_request(zg, m, prompts, 30, o, None, 0, 0, None, e) == code, (code, zg.zg_last_error())
        assert m.cached_len() == n
    r = _lib.generate_request()
    r.size -= 8
    assert zg.zg_gpt_generate_request_enqueue(m.h, C.addressof(r)) == -6 and zg.zg_gpt_generate_request_enqueue(m.h, None) == -6
    lp1, ids1, top1 = m.generate_fetch_logprobs(0, n, 2)  # the record of the last good generation is still there, untouched
    assert np.array_equal(lp.view(np.uint32), lp1.view(np.uint32)) and np.array_equal(ids, ids1) and np.array_equal(m.generate_fetch_range(0, n), got)
    again = m.generate_sample(prompts, n, 0.8, seed=2, top_k=5, logprobs=2, banned_token_ids=[1])  # and the handle still works
    assert np.array_equal(again[0], got)
    m.close()
