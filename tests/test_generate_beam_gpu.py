"""zg_gpt_generate_beam_enqueue: beam search in the device loop.

1. Decisions: from the device's own fetched top-2W lists, tests/beam_ref.py reproduces every recorded token, parent, score, chosen
   log-probability, pool entry and zg_gpt_generate_fetch_beams result bit for bit.
2. Numbers: a host replay that follows the recorded parents with GPT.fork_rows and the recorded tokens with GPT.forward on the same
   row indices gives, at every picked column, logits whose float64 top-2W (tests/logprob_ref.py) match the recorded lists: ids
   exactly, values within 1e-5 + 2.5e-7 |ref|.  This is what holds the cache fork inside the captured step to the caches.
3. W = 1 without eos is GPT.generate's greedy decode, its score the fp32 running sum of the recorded log-probabilities.
4. eos chosen from the no-eos trace (a token among the rank < W candidates of the first ten picks): the pools fill, the done tests
   fire and `end` obeys f + 1 <= end <= min(n_steps, f + 1 + lookahead + 64), at length penalties 0, 1 and 2.
5. Two groups on one handle (W = 4, batch 8) each equal the same group alone on a handle of 4.
6. The traces these tests run on hold a step (behind the first) where two beams share a parent and one where a slot changes owner.

gpt_tiny's shapes with a context of 96 and 80 steps: the multi-step graphs replay and a 64-position bucket is crossed.  Prompts of
three tokens go through the decode steps, as the host replay's do."""
import numpy as np
import pytest

import beam_ref
from beam_ref import bits
from logprob_ref import check_values, logprob_ref
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu
CFG = synth.GPTConfig(257, 96, 2, 2, 128)
N_STEPS, N_P = 80, 3
ERR_ARG = -6


@pytest.fixture(scope="module")
def weights():
    return synth.make_weights(CFG, seed=81, bf16=True)


def make(w, batch, **kw):
    m = zgpt.GPT(CFG, batch=batch, **kw)
    m.load_weights(w)
    return m


def group_prompts(n_groups, seed):
    return [synth.rand_tokens(seed + g, N_P, CFG.vocab_size) for g in range(n_groups)]


def run(m, prompts, W, n_return=None, **opt):
    """One beam generation and everything it recorded: dict(res, end, tokens, parents, scores, lp, ids, top), columns 0 .. end - 1."""
    res = m.beam_search(prompts, N_STEPS, W, num_return_sequences=n_return or W, **opt)
    end = m.cached_len()
    par, sc = m.generate_fetch_beam_trace(0, end)
    lp, ids, top = m.generate_fetch_logprobs(0, end, 2 * W)
    return dict(res=res, end=end, tokens=m.generate_fetch_range(0, end), parents=par, scores=sc, lp=lp, ids=ids.astype(np.int64), top=top)


def check_decisions(r, B, W, eos=None, length_penalty=1.0, early_stopping=True, n_return=None, tag=None):
    """beam_ref over the device's own lists against everything the device recorded; returns the reference state."""
    ref = beam_ref.Beams(B, W, eos, length_penalty, early_stopping, c0=N_P, n_lenpow=CFG.context_size + 1)
    for c in range(N_P, r["end"]):
        tok, par, sc, lp = ref.step(r["ids"][:, c], r["top"][:, c], c)
        assert np.array_equal(r["tokens"][:, c].astype(np.int64), tok), (tag, c, r["tokens"][:, c], tok)
        assert np.array_equal(r["parents"][:, c], par), (tag, c, r["parents"][:, c], par)
        assert np.array_equal(bits(r["scores"][:, c]), bits(sc)), (tag, c, r["scores"][:, c], sc)
        assert np.array_equal(bits(r["lp"][:, c]), bits(lp)), (tag, c)
    want = ref.finalize(r["end"], r["tokens"].astype(np.int64), r["parents"], n_return or W)
    assert len(want) == len(r["res"]) == B // W
    for g, (hw, hg) in enumerate(zip(want, r["res"])):
        assert len(hw) == len(hg), (tag, g, len(hw), len(hg))
        for (seq, norm, total), (gseq, gnorm, gtotal) in zip(hw, hg):
            assert seq == [int(t) for t in gseq], (tag, g, seq, gseq)
            assert np.array_equal(bits([norm, total]), bits([gnorm, gtotal])), (tag, g, norm, gnorm, total, gtotal)
    return ref


def forks_and_moves(r):
    """(steps behind the first in which two beams of the handle share a parent, (slot, column) pairs whose beam came from another slot)."""
    par, B = r["parents"][:, N_P + 1: r["end"]], r["parents"].shape[0]
    return sum(len(set(par[:, c])) < B for c in range(par.shape[1])), int((par != np.arange(B)[:, None]).sum())


@pytest.fixture(scope="module")
def trace48(zg, weights):
    """W = 4 on a handle of 8 (two groups), no eos: the trace tests 1, 2, 4, 5 and 6 share."""
    m = make(weights, 8, beam_generate=True)
    prompts = group_prompts(2, 700)
    r = run(m, prompts, 4)
    m.close()
    return prompts, r


def test_decisions_bit_for_bit(zg, weights, trace48):
    prompts, r = trace48
    assert r["end"] == N_STEPS
    check_decisions(r, 8, 4, tag="W4 B8")
    forks, moves = forks_and_moves(r)
    assert forks > 0 and moves > 0, "the trace holds no fork: it proves nothing about one"
    assert np.isnan(r["lp"][:, :N_P]).all() and not np.isnan(r["lp"][:, N_P:]).any()
    for W, B, opt in [(2, 2, dict(length_penalty=2.0)), (3, 3, dict(length_penalty=0.0, early_stopping=False)), (8, 8, dict())]:
        m = make(weights, B, use_graph=(W != 3))   # (W = 3: the eager steps)
        r2 = run(m, group_prompts(B // W, 710 + W), W, **opt)
        m.close()
        check_decisions(r2, B, W, None, opt.get("length_penalty", 1.0), opt.get("early_stopping", True), tag=(W, B))
        assert forks_and_moves(r2)[1] > 0


def test_numbers_against_a_host_replay(zg, weights, trace48):
    prompts, r = trace48
    W, B, end = 4, 8, r["end"]
    rows = [prompts[b // W] for b in range(B)]
    m = make(weights, B)
    worst = 0.0
    for s in range(end):
        fed = [int(rows[b][s]) if s < N_P else (int(rows[b][-1]) if s == N_P else int(r["tokens"][b, s - 1])) for b in range(B)]
        if s < N_P:
            m.forward(s + 1, fed, compute_logits=False)
            continue
        logits = m.forward(s + 1, fed)
        for b in range(B):  # (also the slots that are dead at c0: their lists are recorded all the same)
            _, ids, top = logprob_ref(logits[b], 0, 2 * W)
            assert np.array_equal(r["ids"][b, s], ids), (s, b, r["ids"][b, s], ids)
            worst = max(worst, check_values(r["top"][b, s], top))
        m.fork_rows(r["parents"][:, s])
    m.close()
    print(f"beam replay: largest |got - ref64| / bound = {worst:.3f}")


def test_one_beam_without_eos_is_greedy(zg, weights):
    B = 3
    prompts = group_prompts(B, 720)
    m = make(weights, B)
    greedy = m.generate(prompts, N_STEPS)
    r = run(m, prompts, 1)
    again = m.generate(prompts, N_STEPS)
    m.close()
    assert np.array_equal(greedy, again), "a greedy generation behind a beam generation"
    assert r["end"] == N_STEPS and np.array_equal(r["tokens"], greedy)
    check_decisions(r, B, 1, tag="W1")
    for g in range(B):
        (seq, score, total), = r["res"][g]
        assert np.array_equal(seq, greedy[g, N_P:])
        run_sum = np.float32(0.0)
        for c in range(N_P, N_STEPS):
            run_sum = np.float32(run_sum + r["lp"][g, c])
        assert np.array_equal(bits(total), bits(run_sum))
        assert np.array_equal(bits(score), bits(np.float32(run_sum / np.float32(N_STEPS - N_P))))


def pick_eos(r, B, W):
    """The token most often among the rank < W candidates of the first ten picks of a no-eos trace."""
    ref = beam_ref.Beams(B, W, None, 1.0, True, c0=N_P, n_lenpow=CFG.context_size + 1)
    count = {}
    for c in range(N_P, N_P + 10):
        ref.step(r["ids"][:, c], r["top"][:, c], c)
        for g in range(B // W):
            for _, _, _, tok in ref.ranked[g][:W]:
                count[(g, tok)] = count.get((g, tok), 0) + 1
    per_tok = {}
    for (g, tok), n in count.items():
        per_tok.setdefault(tok, {})[g] = n
    # a token every group offers, as often as possible in the group that offers it least
    return max(per_tok, key=lambda t: (min(per_tok[t].get(g, 0) for g in range(B // W)), sum(per_tok[t].values())))


@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.0])
def test_eos_fills_the_pools_and_ends_early(zg, weights, length_penalty):
    """One beam: eos is the token the no-eos trace picks at its sixth column (rank 0 < W) and at no earlier one, so the generation
    with eos is the same up to that column, where the pool of one fills.  Early stopping is done there; without it the best new beam
    is the rank-1 candidate of the same column — a lower sum at the same length — so the second test fires there too.  Two beams on
    the most frequent rank < W token: whatever happens is the reference's, and an end obeys the bound."""
    look = 4
    m = make(weights, 1, beam_generate=True)
    prompts = group_prompts(1, 730)
    plain = run(m, prompts, 1)
    picks = [int(t) for t in plain["tokens"][0, N_P: N_P + 10]]
    at = max(i for i in range(10) if picks[i] not in picks[:i] and i <= 5)
    eos, f = picks[at], N_P + at
    for early in (True, False):
        r = run(m, prompts, 1, eos_token_id=eos, length_penalty=length_penalty, early_stopping=early, lookahead=look)
        ref = check_decisions(r, 1, 1, eos, length_penalty, early, tag=("eos", length_penalty, early))
        assert ref.done_col == [f] and len(ref.pools[0]) == 1 and ref.host_done_col() == f + 1
        assert m.cached_len() == r["end"] and f + 1 <= r["end"] <= min(N_STEPS, f + 1 + look + 64)
        assert r["end"] < N_STEPS                      # (f + 1 + 4 + 64 <= 78: the generation did end early)
        (seq, score, total), = r["res"][0]
        assert [int(t) for t in seq] == picks[:at] + [eos]
        assert np.array_equal(bits(score), bits(np.float32(total) / np.float32(beam_ref.lenpow(at + 2, length_penalty)[at + 1])))
    m.close()
    m = make(weights, 2)
    eos = pick_eos(run(m, prompts, 2), 2, 2)
    for early in (True, False):
        r = run(m, prompts, 2, eos_token_id=eos, length_penalty=length_penalty, early_stopping=early, lookahead=look)
        ref = check_decisions(r, 2, 2, eos, length_penalty, early, tag=("eos W2", length_penalty, early))
        assert len(ref.pools[0]) >= 1                  # (the token was offered: it came from the rank < W candidates)
        f1 = ref.host_done_col()
        assert (f1 <= r["end"] <= min(N_STEPS, f1 + look + 64)) if f1 else r["end"] == N_STEPS
    m.close()


def test_groups_do_not_interact(zg, weights, trace48):
    prompts, r = trace48
    for g in range(2):
        m = make(weights, 4)
        alone = run(m, [prompts[g]], 4)
        m.close()
        rows = slice(4 * g, 4 * g + 4)
        assert np.array_equal(alone["tokens"], r["tokens"][rows])
        assert np.array_equal(alone["parents"][:, N_P:] + 4 * g, r["parents"][rows][:, N_P:])
        assert np.array_equal(alone["ids"][:, N_P:], r["ids"][rows][:, N_P:])
        for (seq, score, total), (seq2, score2, total2) in zip(alone["res"][0], r["res"][g]):
            assert np.array_equal(seq, seq2)
            assert abs(float(score) - float(score2)) <= 1e-4 * max(1.0, abs(float(score2))) and abs(float(total) - float(total2)) <= 1e-4 * max(1.0, abs(float(total2)))


def test_fetch_and_argument_errors(zg, weights):
    m = make(weights, 4)
    prompts = group_prompts(2, 740)
    par = np.zeros((4, 8), np.int32)
    sc = np.zeros((4, 8), np.float32)
    assert zg.zg_gpt_generate_fetch_beam_trace(m.h, 0, 8, _lib.ptr(par), _lib.ptr(sc), par.size) == ERR_ARG   # no beam generation yet
    m.generate([prompts[0]] * 4, 20)
    with pytest.raises(_lib.ZgError):
        m.beam_search([prompts[0]] * 4, N_STEPS, 3)   # 4 % 3
    assert m.cached_len() == 20                       # the refused call touched nothing
    res = m.beam_search(prompts, 30, 2, num_return_sequences=2)
    assert m.cached_len() == 30 and len(res) == 2 and all(len(h) == 2 and len(h[0][0]) == 30 - N_P for h in res)
    with pytest.raises(_lib.ZgError):
        m.generate_fetch_beams(3)                     # n_return above num_beams
    with pytest.raises(_lib.ZgError):
        m.generate_fetch_beams(1, max_len=5)          # a stride below the hypothesis
    m.generate([prompts[0]] * 4, 20)
    with pytest.raises(_lib.ZgError):
        m.generate_fetch_beams(1)                     # a generation without beams since
    m.close()
