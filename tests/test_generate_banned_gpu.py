"""zg_gpt_generate_banned_enqueue on a real MI355X: the device loop with the ban stage in its captured step against
the oracle include/zgpt2.h names — for row b, the host loop over the per-token call (zg_gpt_sample_edit; per-row parameters:
zg_gpt_sample_each) that passes banned_ids = the call's own list united with ban_ref.ban_set of the row's history.  The per-token
call takes one ban list for all rows, so at batch 3 that loop runs once per row on the same handle and only that row is compared:
sequences never interact.

The model has test_generate_edit_gpu.py's shapes (vocab 257, context 96, two layers); 80 steps behind ragged prompts of 1 + 2 (b mod
3) tokens replay the multi-step graphs, leave and re-enter their alignment and cross a 64-position bucket.

The tests bite by construction: the suppress ids are the tokens the unbanned call picks first in every row, and one bad word is
(row 0's last prompt token, row 0's first unbanned pick) — a match that reaches into the prompt.  The host loop also draws every
step once WITHOUT the history's bans and counts the steps at which the ban set held that token."""
import ctypes as C

import numpy as np
import pytest

from ban_ref import ban_row, ban_set
from logprob_ref import check_values, logprob_ref
from penalty_ref import penalize_row
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu
CFG = synth.GPTConfig(257, 96, 2, 2, 128)
V = CFG.vocab_size
N_STEPS = 80
ARG, SHAPE = -6, -2
PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.15)
# (temp, top_k, top_p, min_p), the n-gram size, the seed: plain, one filter (top_k = 1: the synthetic weights loop), two filters, min-p alone
FORMS = [((0.8, 0, 1.0, 0.0), 1, 5), ((0.8, 1, 1.0, 0.0), 3, 123456789), ((1.1, 12, 0.8, 0.02), 2, 9), ((0.8, 0, 1.0, 0.05), 2, 77)]
STATIC = [7, 41]   # the call's own ban list beside the rules
MIN_TOKENS = 3


@pytest.fixture(scope="module")
def weights():
    return synth.make_weights(CFG, seed=81, bf16=True)


def make(w, batch, **kw):
    m = zgpt.GPT(CFG, batch=batch, **kw)
    m.load_weights(w)
    return m


def ragged(batch, seed):
    return [synth.rand_tokens(seed + b, 1 + 2 * (b % 3), V) for b in range(batch)]


def host_loop_row(m, b, prompts, n_steps, draw, n=0, words=(), min_tokens=0, suppress=(), static=(), past=0, prior=None, pen=False, rows=None):
    """Row b of the oracle: generate's token logic (the row's own prompt token while the prompt lasts, its last one twice) around the
    per-token call draw(T, toks, banned, history).  Returns (the row's tokens, the steps at which the ban set held the token the
    unbanned row would have picked).  rows (a dict): step -> the reference row of sequence b behind penalties and bans, from the
    device's own raw logits at that step."""
    B = len(prompts)
    out = np.zeros((B, n_steps), np.uint64)
    draws = [0] * B
    bites = 0
    min_np = min(len(p) for p in prompts)
    for i in range(n_steps):
        toks = [int(p[i]) if i < len(p) else (int(p[-1]) if i == len(p) else int(draws[r])) for r, p in enumerate(prompts)]
        if i >= min_np:
            hist = [np.r_[np.asarray([] if prior is None else prior[r], np.uint64), out[r, :i]] for r in range(B)]
            picked = i - len(prompts[b])
            now = ban_set(hist[b], picked, n, words, min_tokens, suppress, vocab=V)
            if picked >= 0:
                free = draw(past + i + 1, toks, sorted(static), hist)
                bites += int(free[b]) in now
            if rows is not None:
                raw = m.forward(past + i + 1, toks)[b]
                base = penalize_row(raw, hist[b], 1.3, 0.4, 0.15)[0] if pen else raw
                rows[i] = ban_row(base, now, banned=sorted(static) if static else None)
            draws = draw(past + i + 1, toks, sorted(set(static) | set(now)), hist)
            assert picked < 0 or int(draws[b]) not in now
        else:
            m.forward(past + i + 1, toks, compute_logits=False)
        for r, p in enumerate(prompts):
            out[r, i] = toks[r] if i < len(p) else draws[r]
    return out[b], bites


def sampler(m, temp, seed, k, p, mp, pen=False):
    return lambda T, toks, banned, hist: m.sample(T, toks, temp, seed=seed, top_k=k, top_p=p, min_p=mp, banned_token_ids=banned or None,
                                                  history=hist if pen else None, **(PEN if pen else {}))


def check_properties(row, n_prompt, n, words, min_tokens, suppress, prior=()):
    """No n-gram ending at a picked column occurred before, no bad word ends at a picked column, no suppress id among the first
    min_tokens picks."""
    h = [int(t) for t in prior] + [int(t) for t in row]
    off = len(prior)
    for s in range(off + n_prompt, len(h)):
        if n >= 1 and s >= n - 1:
            gram = h[s - n + 1: s + 1]
            assert all(h[i: i + n] != gram for i in range(0, s - n + 1)), (s - off, gram, "an n-gram repeats")
        for w in words:
            assert s + 1 < len(w) or h[s + 1 - len(w): s + 1] != [int(t) for t in w], (s - off, w, "a bad word appears")
    assert not set(h[off + n_prompt: off + n_prompt + min_tokens]) & set(int(t) for t in suppress), "a suppress id before min_tokens picks"


@pytest.mark.parametrize("batch,graph,at_create", [(1, True, False), (1, False, False), (3, True, True)])
def test_device_loop_equals_host_loop(zg, weights, batch, graph, at_create):
    prompts = ragged(batch, 910)
    flags = dict(sampled_generate=True, truncated_generate=True, edited_generate=True, banned_generate=True) if at_create else {}
    m = make(weights, batch, use_graph=graph, **flags)
    plain = m.generate_sample(prompts, N_STEPS, 0.8, seed=5)
    for (temp, k, p, mp), n, seed in FORMS:
        free = m.generate_sample(prompts, N_STEPS, temp, seed=seed, top_k=k, top_p=p, min_p=mp, banned_token_ids=STATIC)
        suppress = sorted({int(free[b, len(pr)]) for b, pr in enumerate(prompts)})
        words = [[int(prompts[0][-1]), int(free[0, len(prompts[0])])], [200], [3, 9, 4]]
        rules = dict(no_repeat_ngram_size=n, bad_words_ids=words, min_tokens=MIN_TOKENS, suppress_token_ids=suppress)
        got = m.generate_sample(prompts, N_STEPS, temp, seed=seed, top_k=k, top_p=p, min_p=mp, banned_token_ids=STATIC, **rules)
        again = m.generate_sample(prompts, N_STEPS, temp, seed=seed, top_k=k, top_p=p, min_p=mp, banned_token_ids=STATIC, **rules)
        assert np.array_equal(got, again), "the same call twice"
        assert m.cached_len() == N_STEPS
        for b, pr in enumerate(prompts):
            want, bites = host_loop_row(m, b, prompts, N_STEPS, sampler(m, temp, seed, k, p, mp), n, words, MIN_TOKENS, suppress, STATIC)
            assert np.array_equal(got[b], want), (k, p, mp, b, np.flatnonzero(got[b] != want)[:4])
            assert bites >= 1, (k, p, mp, b, "the rules never forbade what the unbanned row would have picked")
            assert np.array_equal(got[b, : len(pr)], pr)
            assert not np.array_equal(got[b], free[b]), "the tokens are the unbanned call's"
            check_properties(got[b], len(pr), n, words, MIN_TOKENS, suppress)
            assert not set(int(t) for t in got[b, len(pr):]) & set(STATIC)
    assert np.array_equal(m.generate_sample(prompts, N_STEPS, 0.8, seed=5), plain), "a plain generation behind banned ones"
    m.close()


def test_with_penalties_logprobs_and_stop_conditions(zg, weights):
    B, n_steps, top_n, n, min_tokens = 3, 40, 8, 2, 6
    prompts = ragged(B, 950)
    m = make(weights, B)
    kw = dict(seed=8, top_k=6, min_p=0.02, **PEN)
    probe = m.generate_sample(prompts, n_steps, 1.3, **kw)
    stop_ids = sorted({int(probe[b, len(p) + 1]) for b, p in enumerate(prompts)})  # every row of the unbanned call finishes by its second pick
    words = [[int(prompts[1][-1]), int(probe[1, len(prompts[1])])]]
    rules = dict(no_repeat_ngram_size=n, bad_words_ids=words, min_tokens=min_tokens)
    got, lp, ids, top = m.generate_sample(prompts, n_steps, 1.3, logprobs=top_n, **kw, **rules)
    for b, p in enumerate(prompts):
        rows = {}
        want, bites = host_loop_row(m, b, prompts, n_steps, sampler(m, 1.3, 8, 6, 1.0, 0.02, pen=True), n, words, pen=True, rows=rows)
        assert np.array_equal(got[b], want), (b, np.flatnonzero(got[b] != want)[:4])
        assert bites >= 1 or b != 1
        check_properties(got[b], len(p), n, words, 0, ())
        worst = 0.0
        assert np.isnan(lp[b, : len(p)]).all()
        for s in range(len(p), n_steps):
            r_lp, r_ids, r_top = logprob_ref(rows[s], got[b, s], top_n)
            worst = max(worst, check_values(lp[b, s], r_lp), check_values(top[b, s], r_top))
            assert np.array_equal(ids[b, s].astype(np.int64), r_ids), (b, s, ids[b, s], r_ids)
        assert worst <= 1.0
    # stop tokens on top, suppressed (the Python default: suppress_token_ids = stop_token_ids) until min_tokens picks are made
    m.generate_sample(prompts, n_steps, 1.3, stop_token_ids=stop_ids, **kw)
    _, fin0, _ = m.stop_result()
    assert all(f is not None and f <= len(p) + 1 for f, p in zip(fin0, prompts)), "unbanned, every row stops by its second pick"
    cut, lp2, ids2, top2 = m.generate_sample(prompts, n_steps, 1.3, logprobs=top_n, stop_token_ids=stop_ids, **kw, **rules)
    end, fin, _ = m.stop_result()
    assert cut.shape[1] == end
    for b, p in enumerate(prompts):
        assert fin[b] is None or fin[b] >= len(p) + min_tokens, (b, fin[b], "finish_col >= first picked column + min_tokens")
        want, bites = host_loop_row(m, b, prompts, end, sampler(m, 1.3, 8, 6, 1.0, 0.02, pen=True), n, words, min_tokens, stop_ids, pen=True)
        assert np.array_equal(cut[b], want), (b, np.flatnonzero(cut[b] != want)[:4])
        assert bites >= 1, b
        check_properties(cut[b], len(p), n, words, min_tokens, stop_ids)
    m.close()


def test_generate_from_with_a_prior_and_a_handle_without_the_whole_prompt_pass(zg, weights):
    """n = 3 and the history ... a b c a | b: the suffix (a, b) straddles the prior and the new prompt, and bans c at the first pick —
    which a +30 bias makes the pick of the unbanned call."""
    B, past, n_steps, n = 2, 13, 60, 3
    a, b_, c = 50, 60, 70
    first = np.stack([synth.rand_tokens(920 + b, past, V) for b in range(B)])
    first[:, past - 4:] = [a, b_, c, a]
    turns = [np.array([b_], np.uint64), np.array([b_, 5, 6], np.uint64)]
    prior = [first[r] for r in range(B)]
    kw = dict(temp=0.8, seed=21, top_k=9, logit_bias={c: 30.0})
    for hkw in (dict(), dict(prefill=False)):
        m = make(weights, B, **hkw)
        feed = (lambda: m.extend(0, first, compute_logits=False)) if not hkw else (lambda: m.generate(list(first), past))
        feed()
        free = m.generate_from(past, turns, n_steps, prior=prior, **kw)
        assert int(free[0, 1]) == c, "unbanned, the biased token is the first pick"
        feed()
        got = m.generate_from(past, turns, n_steps, prior=prior, no_repeat_ngram_size=n, **kw)
        assert m.cached_len() == past + n_steps
        assert int(got[0, 1]) != c and ban_set(np.r_[prior[0], turns[0]], 0, n) == [c]
        draw = lambda T, toks, banned, hist: m.sample(T, toks, 0.8, seed=21, top_k=9, logit_bias={c: 30.0}, banned_token_ids=banned or None)
        for r in range(B):
            feed()
            want, bites = host_loop_row(m, r, turns, n_steps, draw, n, past=past, prior=prior)
            assert np.array_equal(got[r], want), (hkw, r, np.flatnonzero(got[r] != want)[:4])
            assert bites >= 1
            check_properties(got[r], len(turns[r]), n, (), 0, (), prior=prior[r])
        m.close()


ROWS3 = [dict(temp=0.8, seed=11, no_repeat_ngram_size=1, min_tokens=2), dict(temp=0.7, top_k=9, top_p=0.9, seed=12, **PEN),
         dict(temp=1.2, min_p=0.05, seed=13, no_repeat_ngram_size=3, min_tokens=5)]


def test_generate_each_row_b_is_row_b_of_the_uniform_call(zg, weights):
    B = 3
    prompts = ragged(B, 960)
    m = make(weights, B)
    plain_rows = [{k: v for k, v in r.items() if k not in ("no_repeat_ngram_size", "min_tokens")} for r in ROWS3]
    free = m.generate_each(prompts, N_STEPS, plain_rows)
    suppress = sorted({int(free[b, len(p)]) for b, p in enumerate(prompts)})
    words = [[int(prompts[1][-1]), int(free[1, len(prompts[1])])]]
    got = m.generate_each(prompts, N_STEPS, ROWS3, bad_words_ids=words, suppress_token_ids=suppress)
    assert not np.array_equal(got, free)
    for b, r in enumerate(ROWS3):
        r = dict(r)
        temp, seed = r.pop("temp"), r.pop("seed")
        uni = m.generate_sample(prompts, N_STEPS, temp, seed=seed, bad_words_ids=words, suppress_token_ids=suppress, **r)
        assert np.array_equal(got[b], uni[b]), (b, np.flatnonzero(got[b] != uni[b])[:4])
        assert not np.array_equal(got[b], free[b]), (b, "the rules changed nothing")
        check_properties(got[b], len(prompts[b]), r.get("no_repeat_ngram_size", 0), words, r.get("min_tokens", 0), suppress)
    m.close()


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def banned_call(zg, m, prompts, n, opt, bans, edits=None, rows=None, seed=3, past=0):
    mat, lens, stride = m._prompts(prompts)
    r = _lib.generate_request(past_len=past, prompts=_lib.ptr(mat), prompt_stride=stride, prompt_lens=_lib.ptr(lens), n_steps=n,
                              options=None if opt is None else C.addressof(opt), seed=seed, edits=None if edits is None else C.addressof(edits))
    return zg.zg_gpt_generate_banned_enqueue(m.h, C.addressof(r), None if rows is None else C.addressof(rows), 0 if rows is None else len(rows),
                                             None if bans is None else C.addressof(bans))


def test_all_rules_off_is_the_call_without_them_bit_for_bit(zg, weights):
    B = 3
    m = make(weights, B)
    prompts = ragged(B, 970)
    want = m.generate_sample(prompts, N_STEPS, 0.8, seed=3, top_k=9, logprobs=4, **PEN)
    got = m.generate_sample(prompts, N_STEPS, 0.8, seed=3, top_k=9, logprobs=4, no_repeat_ngram_size=0, bad_words_ids=[], min_tokens=4, **PEN)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    assert np.array_equal(u32(got[1]), u32(want[1])) and np.array_equal(u32(got[3]), u32(want[3]))
    # through the entry itself: null rules, rules that are all off (min_tokens without a suppress id), greedy included
    off, keep = _lib.ban_rules(B, 0, None, 7, None)
    opt = _lib.SampleOptions(0.8, 9, 1.0)
    plain = m.generate_sample(prompts, N_STEPS, 0.8, seed=3, top_k=9)
    for bans in (None, off):
        assert banned_call(zg, m, prompts, N_STEPS, opt, bans) == 0, zg.zg_last_error()
        assert np.array_equal(m.generate_fetch(N_STEPS), plain)
        assert banned_call(zg, m, prompts, N_STEPS, None, bans) == 0, zg.zg_last_error()
        assert np.array_equal(m.generate_fetch(N_STEPS), m.generate(prompts, N_STEPS))
    del keep
    m.close()


def test_refusals_leave_the_handle_and_the_records_alone(zg, weights):
    B, n = 2, 24
    prompts = ragged(B, 980)
    m = make(weights, B)
    got, lp, ids, top = m.generate_sample(prompts, n, 0.8, seed=2, top_k=5, logprobs=2, no_repeat_ngram_size=2)
    opt = _lib.SampleOptions(0.8, 5, 1.0)
    good, k0 = _lib.ban_rules(B, 2, [[1, 2]], 3, [4])
    wrong_size, k1 = _lib.ban_rules(B, 2)
    wrong_size.size -= 8
    big_n, k2 = _lib.ban_rules(B, [2, 17])
    over, k3 = _lib.ban_rules(B, 0, [[1, V]])
    few, k4 = _lib.ban_rules(B, 1)                    # n = 1 over 80 steps beside an allow-list of 30 tokens: a row could be emptied
    allow, k5 = _lib.logit_edits(None, list(range(30)), None, 0.0)
    table = _lib.row_sampling([dict(temp=0.8, seed=1)] * B)
    cases = [(opt, wrong_size, None, None, 30, ARG), (opt, big_n, None, None, 30, ARG), (opt, over, None, None, 30, SHAPE),
             (None, good, None, None, 30, ARG),        # greedy with a rule on
             (opt, few, allow, None, 80, ARG), (opt, good, None, table, 30, ARG)]  # ... and options beside rows: the each call's own rule
    for o, bans, e, rows, steps, code in cases:
        assert banned_call(zg, m, prompts, steps, o, bans, e, rows) == code, (code, zg.zg_last_error())
        assert m.cached_len() == n
    assert banned_call(zg, m, prompts, 20, opt, few, allow) == 0, "20 steps ban at most 20 of the 30"
    m.generate_sample(prompts, n, 0.8, seed=2, top_k=5, logprobs=2, no_repeat_ngram_size=2)
    r = _lib.generate_request()
    r.size -= 8
    assert zg.zg_gpt_generate_banned_enqueue(m.h, C.addressof(r), None, 0, C.addressof(good)) == ARG
    assert zg.zg_gpt_generate_banned_enqueue(m.h, None, None, 0, None) == ARG
    lp1, ids1, top1 = m.generate_fetch_logprobs(0, n, 2)  # the records of the last good generation are still there
    assert np.array_equal(u32(lp), u32(lp1)) and np.array_equal(ids, ids1) and np.array_equal(m.generate_fetch_range(0, n), got)
    del k0, k1, k2, k3, k4, k5
    m.close()
