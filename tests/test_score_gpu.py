"""zg_gpt_score: the whole-prompt pass of zg_gpt_extend that also records, for every position it feeds, the
log-probability of the token there and the top-N alternatives.

The records are held to the float64 reference tests/score_ref.py ON THE PASS'S OWN LOGITS (logits_out: the bits the statistics
kernels read, so ids are exact and values lie within logprob_ref.bound), and the logits to the oracle with the project's
model-level bound (golden_io.assert_model_close, rtol 1e-3).  The model has gpt_tiny's shapes with a vocabulary of 257 — on the
GEMMs' 64-column grid that is 256 rows of wte in place and a tail strip of one row — and a context of 96; the real vocabulary runs
once, inside one block of 256 rows and across two, with its 17-row strip."""
import ctypes as C

import numpy as np
import pytest

import oracle
from golden_io import assert_model_close
from logprob_ref import bound, check_values
from score_ref import score_ref
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu
CFG = synth.GPTConfig(257, 96, 2, 2, 128)
ERR_SHAPE, ERR_UNSUPPORTED, ERR_ARG = -2, -5, -6
PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.15)


@pytest.fixture(scope="module")
def weights():
    return synth.make_weights(CFG, seed=81, bf16=True)


@pytest.fixture(scope="module")
def models(zg, weights):
    """one scoring handle per batch, made on first use and shared by the tests of this file"""
    made = {}

    def get(batch):
        if batch not in made:
            made[batch] = make(CFG, weights, batch, score=True)
        return made[batch]

    yield get
    for m in made.values():
        m.close()


def make(cfg, w, batch, **kw):
    m = zgpt.GPT(cfg, batch=batch, **kw)
    m.load_weights(w)
    return m


def rows_of(batch, n, seed, vocab=CFG.vocab_size):
    return np.stack([synth.rand_tokens(seed + b, n, vocab) for b in range(batch)])


def check_records(got, logits, tokens, top_n, tag):
    """(logprobs, top_ids, top_logprobs) of columns past .. past + n - 1 against score_ref on the pass's own logits: NaN exactly at
    the first column, ids exact, values within the bound.  Returns the largest |got - ref| / bound."""
    lp, ids, top = got[:3]
    B, n = tokens.shape
    assert lp.shape == (B, n) and ids.shape == (B, n, top_n) and top.shape == (B, n, top_n)
    worst = 0.0
    for b in range(B):
        rlp, rids, rtop = score_ref(logits[b], tokens[b], top_n)
        assert np.isnan(lp[b, 0]) and not np.isnan(lp[b, 1:]).any(), (tag, b, lp[b])
        assert np.array_equal(ids[b, 1:].astype(np.int64), rids[1:]), (tag, b, np.argwhere(ids[b, 1:].astype(np.int64) != rids[1:])[:4])
        if n > 1:
            worst = max(worst, check_values(lp[b, 1:], rlp[1:]))
            if top_n:
                worst = max(worst, check_values(top[b, 1:], rtop[1:]))
        for p in range(1, n):  # where an id is the token: bit for bit its log-probability
            for j in np.flatnonzero(ids[b, p] == tokens[b, p]):
                assert top[b, p, j].view(np.uint32) == lp[b, p].view(np.uint32), (tag, b, p)
    return worst


def check_logits(cfg, w, logits, tokens, tag):
    worst = 0.0
    for b in range(tokens.shape[0]):
        ref = oracle.GPT(cfg, w).forced_logits(tokens[b], 0)
        for p in range(tokens.shape[1]):
            worst = max(worst, assert_model_close(ref[p], logits[b, p], f"{tag} row {b} position {p}", rtol=1e-3))
    return worst


# 1 + 2: the records against the pass's own logits, the logits against the reference
@pytest.mark.parametrize("n", [2, 80])
@pytest.mark.parametrize("batch", [1, 3, 8])
def test_records_and_logits(models, weights, batch, n):
    m = models(batch)
    tokens = rows_of(batch, n, 1000 * batch + n)
    first = None
    for top_n in (0, 5, 20):
        out = m.score(tokens, top_n=top_n, want_logits=True)
        logits = out[3]
        worst = check_records(out, logits, tokens, top_n, (batch, n, top_n))
        if first is None:
            first = logits
            lw = check_logits(CFG, weights, logits, tokens, (batch, n))
        assert np.array_equal(logits.view(np.uint32), first.view(np.uint32))  # the same pass, the same bits
        assert m.cached_len() == n
        print(f"score batch={batch} n={n} top_n={top_n}: records {worst:.3f} of the bound, logits within {lw:.2e} relative (limit 1e-3)")


# 3: against the device loop
def test_against_the_device_loop(models):
    """A greedy generate(prompts, 60, logprobs=5) records column i >= len(prompt) from the logits of the step at position i, which
    fed: the prompt, the last prompt token once more (main.zig:334,337), then the picks.  Scoring that FED sequence with the last
    pick appended, column i + 1 of score is the log-probability of the same token under the same history as column i of the
    generation — through the whole-prompt pass instead of the decode kernels.  With delta = max |score's logits - the decode
    logits| over those positions (taken here by forward over the fed tokens), every picked column satisfies |lp_score - lp_generate|
    <= 2 delta + 2 bound: |change of LSE| <= max |dx|, plus the target's own dx, plus each side's fp32 error of the expression."""
    B, N = 3, 60
    m = models(B)
    prompts = [synth.rand_tokens(40 + b, 1 + 2 * b, CFG.vocab_size) for b in range(B)]
    toks, glp, gids, gtop = m.generate(prompts, N, logprobs=5)
    fed = np.zeros((B, N + 1), np.uint64)
    for b, p in enumerate(prompts):
        fed[b] = np.r_[p, p[-1:], toks[b, len(p):]]
    dec = np.stack([m.forward(T, fed[:, T - 1], want_logits=True) for T in range(1, N + 1)], axis=1)  # [B, N, V]: row i predicts what column i records
    slp, sids, stop, slog = m.score(fed, top_n=5, want_logits=True)
    delta, worst = 0.0, 0.0
    for b, p in enumerate(prompts):
        delta = max(delta, float(np.abs(slog[b, len(p): N].astype(np.float64) - dec[b, len(p):]).max()))
    for b, p in enumerate(prompts):
        for i in range(len(p), N):
            assert fed[b, i + 1] == toks[b, i]
            a, g = float(slp[b, i + 1]), float(glp[b, i])
            lim = 2 * delta + 2 * bound(g)
            assert abs(a - g) <= lim, (b, i, a, g, delta)
            worst = max(worst, abs(a - g) / lim)
    print(f"score against the device loop: delta = {delta:.3e}, largest |lp_score - lp_generate| / (2 delta + 2 bound) = {worst:.3f}")


# 4: the same cache effect as extend
def test_same_cache_effect_as_extend(models):
    B = 3
    m = models(B)
    tokens = rows_of(B, 30, 77)
    new = [synth.rand_tokens(90 + b, 1 + b, CFG.vocab_size) for b in range(B)]
    got = {}
    for how in ("extend", "score"):
        if how == "extend":
            m.extend(0, tokens)
        else:
            m.score(tokens, top_n=5)
        assert m.cached_len() == 30
        arg = m.argmax()
        gen = m.generate_from(30, new, 40, temp=0.8, seed=3, top_k=9)
        got[how] = (arg, gen, m.cached_len())
    assert np.array_equal(got["extend"][0], got["score"][0])
    assert np.array_equal(got["extend"][1], got["score"][1]) and got["extend"][2] == got["score"][2] == 70
    # and the record goes on behind a score: the generation's columns follow the scored ones
    m.score(tokens, top_n=5)
    m.generate_from(30, new, 40, logprobs=5)
    lp, _, _ = m.generate_fetch_logprobs(0, 70, 5)
    for b in range(B):
        assert np.isnan(lp[b, 0]) and not np.isnan(lp[b, 1:30]).any()
        assert np.isnan(lp[b, 30: 30 + len(new[b])]).all() and not np.isnan(lp[b, 30 + len(new[b]):]).any()


# 5: continuation and rollback
@pytest.mark.parametrize("kv", ["f32", "f16", "b24"])
def test_continuation_and_rollback(zg, weights, kv):
    B, top_n = 2, 5
    m = make(CFG, weights, B, score=True, kv_f16=kv == "f16", kv_b24=kv == "b24")
    tokens = rows_of(B, 70, 7)
    flp, fids, ftop, flog = m.score(tokens, top_n=top_n, want_logits=True)
    alp, aids, atop, alog = m.score(tokens[:, :30], top_n=top_n, want_logits=True)
    before = m.generate_fetch_logprobs(0, 29, top_n)
    blp, bids, btop, blog = m.score(tokens[:, 29:], past_len=29, top_n=top_n, want_logits=True)
    assert m.cached_len() == 70
    after = m.generate_fetch_logprobs(0, 29, top_n)
    for x, y in zip(before, after):  # columns below past_len: bitwise what the first call recorded
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert np.isnan(blp[:, 0]).all() and np.isnan(m.generate_fetch_logprobs(29, 1, 0)[0]).all()
    check_records((blp, bids, btop), blog, tokens[:, 29:], top_n, (kv, "second chunk"))
    lp = np.concatenate([alp[:, :30], blp[:, 1:]], axis=1)      # columns 0 .. 29 of the first call, 30 .. 69 of the second
    log2 = np.concatenate([alog, blog[:, 1:]], axis=1)
    delta = float(np.abs(log2.astype(np.float64) - flog).max())
    worst = 0.0
    for b in range(B):
        for c in range(1, 70):
            lim = 2 * bound(float(flp[b, c])) + (0.0 if kv == "f32" else 2 * delta)
            assert abs(float(lp[b, c]) - float(flp[b, c])) <= lim, (kv, b, c, lp[b, c], flp[b, c], delta)
            worst = max(worst, abs(float(lp[b, c]) - float(flp[b, c])) / lim)
    print(f"score in two chunks, kv {kv}: delta = {delta:.3e}, largest difference / limit = {worst:.3f}")
    m.close()


# 6: weight storage
@pytest.mark.parametrize("storage", ["f32", "b24"])
def test_weight_storage(zg, storage):
    w = synth.make_weights(CFG, seed=82, bf16=False)
    wref = w if storage == "f32" else {k: (synth.round_b24(v) if np.ndim(v) == 2 else v) for k, v in w.items()}
    m = make(CFG, w, 2, score=True, weights_f32=storage == "f32", weights_b24=storage == "b24")
    for n, top_n in ((2, 5), (80, 20)):
        tokens = rows_of(2, n, 300 + n)
        out = m.score(tokens, top_n=top_n, want_logits=True)
        worst = check_records(out, out[3], tokens, top_n, (storage, n))
        lw = check_logits(CFG, wref, out[3], tokens, (storage, n))
        print(f"score weights {storage} n={n}: records {worst:.3f} of the bound, logits within {lw:.2e} relative (limit 1e-3)")
    m.close()


# 7: loglikelihood
def test_loglikelihood(models):
    B = 3
    m = models(B)
    V = CFG.vocab_size
    contexts = [synth.rand_tokens(60 + b, k, V) for b, k in enumerate((1, 4, 9))]
    n_cont = (1, 7, 3)
    # greedy continuations by the decode loop, row by row in lock step (a finished row feeds padding)
    seqs = [list(int(t) for t in c) for c in contexts]
    for T in range(1, max(len(c) + k for c, k in zip(contexts, n_cont))):
        logits = m.forward(T, [s[T - 1] if T - 1 < len(s) else 0 for s in seqs], want_logits=True)
        for b in range(B):
            if T == len(seqs[b]) and len(seqs[b]) < len(contexts[b]) + n_cont[b]:
                seqs[b].append(int(np.argmax(logits[b])))
    greedy = [np.array(s[len(c):], np.uint64) for s, c in zip(seqs, contexts)]
    assert [len(g) for g in greedy] == list(n_cont)
    for replace in (None, 0, 1, 2):
        conts = [g.copy() for g in greedy]
        if replace is not None:
            conts[replace][-1] = (conts[replace][-1] + 1) % V
        got = m.loglikelihood(contexts, conts)
        mat, _, _ = zgpt._pack_prompts([np.r_[c, k] for c, k in zip(contexts, conts)], B)
        logits = m.score(mat, top_n=1, want_logits=True)[3]
        for b in range(B):
            rlp, rids, _ = score_ref(logits[b], mat[b], 1)
            cols = slice(len(contexts[b]), len(contexts[b]) + n_cont[b])
            ref_sum, ref_greedy = rlp[cols].sum(), bool(np.array_equal(rids[cols, 0], mat[b, cols].astype(np.int64)))
            assert abs(got[b][0] - ref_sum) <= n_cont[b] * bound(rlp[cols]).max(), (replace, b, got[b], ref_sum)
            assert got[b][1] == ref_greedy == (replace != b), (replace, b, got[b], ref_greedy)


# 8: the flag and the errors
def state_of(m, n):
    return (m.cached_len(),) + tuple(a.tobytes() for a in m.generate_fetch_logprobs(0, n, 5))


def test_without_the_flag(zg, weights):
    m = make(CFG, weights, 2)
    prompts = [synth.rand_tokens(5 + b, 2 + b, CFG.vocab_size) for b in range(2)]
    m.generate(prompts, 20, logprobs=5)
    before = state_of(m, 20)
    with pytest.raises(_lib.ZgError) as e:
        m.score(rows_of(2, 10, 3), top_n=5)
    assert e.value.code == ERR_UNSUPPORTED
    assert state_of(m, 20) == before
    m.close()


def test_errors_leave_the_state(models, zg, weights):
    m = models(2)
    tokens = rows_of(2, 20, 11)
    m.score(tokens, top_n=5)
    before = state_of(m, 20)

    def refused(code, *a, **kw):
        with pytest.raises(_lib.ZgError) as e:
            m.score(*a, **kw)
        assert e.value.code == code, (e.value, a, kw)
        assert state_of(m, 20) == before

    refused(ERR_ARG, tokens, top_n=21)
    refused(ERR_ARG, tokens[:, :5], past_len=21, top_n=5)                     # beyond the 20 cached positions
    bad = tokens.copy()
    bad[1, 7] = CFG.vocab_size
    refused(ERR_SHAPE, bad, top_n=5)
    short = np.zeros(2 * 20 * CFG.vocab_size - 1, np.float32)                 # logits_out one element short
    rc = zg.zg_gpt_score(m.h, 0, _lib.ptr(tokens), 20, 20, 5, _lib.ptr(short), short.size)
    assert rc == ERR_SHAPE and state_of(m, 20) == before
    small = synth.GPTConfig(7, 16, 1, 2, 128)                                 # top_n within 20 but above the vocabulary
    s = make(small, synth.make_weights(small, seed=3, bf16=True), 1, score=True)
    with pytest.raises(_lib.ZgError) as e:
        s.score(rows_of(1, 5, 1, vocab=7), top_n=8)
    assert e.value.code == ERR_ARG and s.cached_len() == 0
    out = s.score(rows_of(1, 5, 1, vocab=7), top_n=7, want_logits=True)       # (a vocabulary below 64: the strip alone)
    check_records(out, out[3], rows_of(1, 5, 1, vocab=7), 7, "vocab 7")
    s.close()


def test_a_handle_with_the_flag_that_never_scores_generates_the_same(zg, weights):
    prompts = [synth.rand_tokens(20 + b, 1 + 2 * b, CFG.vocab_size) for b in range(3)]
    got = {}
    for flag in (False, True):
        m = make(CFG, weights, 3, score=flag)
        got[flag] = (m.generate(prompts, 80), m.generate_sample(prompts, 80, 0.8, seed=7, top_k=7, **PEN))
        m.close()
    assert np.array_equal(got[False][0], got[True][0]) and np.array_equal(got[False][1], got[True][1])


# 9: the real vocabulary, once
def test_the_real_vocabulary(zg):
    """50257 = 64 x 785 + 17: the 17-row strip.  130 positions cross a block of 128 rows; the block has 256 (the measured choice,
    profiles/NOTEBOOK.md §16), so 260 positions run too: a whole block and a remainder of four rows."""
    cfg = synth.GPTConfig(50257, 1024, 2, 12, 768)  # 124M's shapes, two layers
    w = synth.make_weights(cfg, seed=9, bf16=True)
    m = make(cfg, w, 1, score=True)
    tokens = rows_of(1, 260, 500, vocab=cfg.vocab_size)
    ref = oracle.GPT(cfg, w).forced_logits(tokens[0], 0)  # (causal: its first 130 rows are the shorter text's)
    for n in (130, 260):
        out = m.score(tokens[:, :n], top_n=20, want_logits=True)
        worst = check_records(out, out[3], tokens[:, :n], 20, ("124M x 2 layers", n))
        lw = max(assert_model_close(ref[p], out[3][0, p], f"124M x 2 layers, n {n}, position {p}", rtol=1e-3) for p in range(n))
        print(f"score V=50257 n={n}: records {worst:.3f} of the bound, logits within {lw:.2e} relative (limit 1e-3)")
    m.close()
