"""zg_gpt_generate_guided_enqueue on a real MI355X: the device loop with the guide's mask and advance in its
captured step against the oracle include/zgpt2.h names — for row b, the host loop over the existing per-token call (zg_gpt_sample_edit;
per-row parameters: zg_gpt_sample_each) that passes allowed_ids = the guide's set of the row's state and walks the automaton on the
host.  At batch 3 that loop runs once per row on the same handle and only that row is compared: sequences never interact.

The model has one layer, a vocabulary of 257 and a context of 192; 80 steps behind ragged prompts replay the multi-step graphs, leave
and re-enter their alignment and cross a 64-position bucket.  One union table holds a random automaton of six states (each allowing
about 40 % of the vocabulary), three states that allow the SAME set but lead to one another (the log-probability record of such a
row must equal, bit for bit, the static allow-list's), and a trie of multi-token choices."""
import ctypes as C

import numpy as np
import pytest

import guide_ref
from guide_ref import NONE
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth
from zig_gpt2_amd.guide import DEAD, Guide

pytestmark = pytest.mark.gpu
CFG = synth.GPTConfig(257, 192, 1, 2, 128)
V = CFG.vocab_size
N_STEPS = 80
END = V - 1
ARG, UNSUPPORTED = -6, -5
PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.15)
CHOICES = [[10, 20, 30], [10, 20], [10, 21, 5, 6], [200], [201, 2]]


def random_automaton(seed, n):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, n, (n, V)).astype(np.uint16)
    t[rng.random((n, V)) >= 0.4] = DEAD
    t[:, [7, 41, 200]] = DEAD  # (room for a ban list and a bias on dropped tokens)
    return Guide(t)


def same_set_automaton():
    """three states allowing the tokens 3 mod 4 below 120, token t leading to state t mod 3"""
    t = np.full((3, V), DEAD, np.uint16)
    ids = np.arange(3, 120, 4)
    t[:, ids] = ids % 3
    return Guide(t), [int(i) for i in ids]


RAND = random_automaton(7, 6)
SAME, SAME_IDS = same_set_automaton()
CHOICE = Guide.from_choices(CHOICES, V, END)
UNION, (OFF_RAND, OFF_SAME, OFF_CHOICE) = Guide.union([RAND, SAME, CHOICE])


@pytest.fixture(scope="module")
def weights():
    return synth.make_weights(CFG, seed=83, bf16=True)


def make(w, batch, **kw):
    m = zgpt.GPT(CFG, batch=batch, guided=True, **kw)
    m.load_weights(w)
    m.load_guide(UNION)
    return m


def ragged(batch, seed):
    return [synth.rand_tokens(seed + b, 1 + 2 * (b % 3), V) for b in range(batch)]


def host_loop_row(m, b, prompts, n_steps, start, draw, past=0, banned=()):
    """Row b of the oracle: generate's token logic around the per-token call `draw(T, toks, allowed, history)`, the automaton walked
    here.  allowed = the state's set (minus nothing: a ban list stays the call's own argument) while row b stands at a picked column
    of a guided row, else None.  The other rows are fed their own draws: whatever they hold, row b does not see it."""
    B = len(prompts)
    out = np.zeros((B, n_steps), np.uint64)
    draws = [0] * B
    st = start
    states = np.full(n_steps, NONE, np.uint64)
    min_np = min(len(p) for p in prompts)
    for i in range(n_steps):
        toks = [int(p[i]) if i < len(p) else (int(p[-1]) if i == len(p) else int(draws[r])) for r, p in enumerate(prompts)]
        if i >= min_np:
            picked = i >= len(prompts[b])
            allowed = [int(t) for t in UNION.allowed(st)] if picked and st != NONE else None
            draws = draw(past + i + 1, toks, allowed, [out[r, :i] for r in range(B)])
            if picked and st != NONE:
                assert int(draws[b]) in allowed and int(draws[b]) not in banned
                states[i] = st
                st = UNION.step(st, int(draws[b]))
        else:
            m.forward(past + i + 1, toks, compute_logits=False)
        for r, p in enumerate(prompts):
            out[r, i] = toks[r] if i < len(p) else draws[r]
    return out[b], states


SETTINGS = ["plain", "filters_penalties_edits", "per_row"]
ROWS3 = [dict(temp=0.8, seed=11), dict(temp=0.7, top_k=9, top_p=0.9, seed=12, **PEN), dict(temp=1.2, min_p=0.05, seed=13)]
EDITS = dict(logit_bias={3: 2.5, 100: -4.0, 41: 3.0, END: 0.5}, banned_token_ids=[7, 41, 200])


def run_setting(m, setting, prompts, n, starts, **more):
    """(what the device loop returns, the per-token call of the same setting as draw(T, toks, allowed, history))"""
    B = len(prompts)
    if setting == "plain":
        got = m.generate_sample(prompts, n, 0.8, seed=5, guide_states=starts, **more)
        return got, lambda T, toks, allowed, hist: m.sample(T, toks, 0.8, seed=5, allowed_token_ids=allowed)
    if setting == "filters_penalties_edits":
        got = m.generate_sample(prompts, n, 0.9, seed=6, top_k=12, top_p=0.8, guide_states=starts, **PEN, **EDITS, **more)
        return got, lambda T, toks, allowed, hist: m.sample(T, toks, 0.9, seed=6, top_k=12, top_p=0.8, history=hist, allowed_token_ids=allowed, **PEN, **EDITS)
    rows = ROWS3[:B]
    got = m.generate_each(prompts, n, rows, guide_states=starts, **more)
    return got, lambda T, toks, allowed, hist: m.sample_each(T, toks, rows, history=hist, allowed_token_ids=allowed)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("batch,graph,at_create", [(1, True, False), (3, True, True), (3, False, False)])
def test_device_loop_equals_host_loop(zg, weights, batch, graph, at_create, setting):
    flags = dict(sampled_generate=True, truncated_generate=True, edited_generate=True) if at_create else {}
    m = make(weights, batch, use_graph=graph, **flags)
    prompts = ragged(batch, 910)
    starts = [OFF_RAND + 2] if batch == 1 else [OFF_RAND, None, OFF_RAND + 4]  # different start states of one table, one row without
    got, draw = run_setting(m, setting, prompts, N_STEPS, starts)
    assert m.cached_len() == N_STEPS
    rec = m.generate_fetch_guide_states(0, N_STEPS)
    banned = EDITS["banned_token_ids"] if setting == "filters_penalties_edits" else ()
    for b in range(batch):
        st = NONE if starts[b] is None else starts[b]
        want, states = host_loop_row(m, b, prompts, N_STEPS, st, draw, banned=banned)
        assert np.array_equal(got[b], want), (setting, b, np.flatnonzero(got[b] != want)[:4])
        assert np.array_equal(rec[b], states), (setting, b, "the state record is the host's walk")
        ref_rec, _ = guide_ref.record(UNION.next, [st], got[b: b + 1], [len(prompts[b])])
        assert np.array_equal(rec[b], ref_rec[0])
        for p in range(len(prompts[b]), N_STEPS):
            assert st == NONE or UNION.next[int(rec[b, p]), int(got[b, p])] != DEAD, "a pick its recorded state does not allow"
        assert np.array_equal(got[b, : len(prompts[b])], prompts[b])
    again, _ = run_setting(m, setting, prompts, N_STEPS, starts)
    assert np.array_equal(again, got), "the same call twice"
    free, _ = run_setting(m, setting, prompts, N_STEPS, [None] * batch)
    assert not np.array_equal(free[0], got[0]), "the guide changed nothing"
    m.close()


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_all_rows_without_a_guide_is_the_unguided_call_bit_for_bit(zg, weights):
    B = 3
    m = make(weights, B)
    prompts = ragged(B, 920)
    for kw in (dict(), dict(top_k=9, top_p=0.9, **PEN, **EDITS)):
        want = m.generate_sample(prompts, N_STEPS, 0.8, seed=3, logprobs=4, **kw)
        got = m.generate_sample(prompts, N_STEPS, 0.8, seed=3, logprobs=4, guide_states=[None] * B, **kw)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
        assert np.array_equal(u32(got[1]), u32(want[1])) and np.array_equal(u32(got[3]), u32(want[3]))
        assert (m.generate_fetch_guide_states(0, N_STEPS) == NONE).all()
    # greedy too: with no guided row nothing asks for a sampler
    want = m.generate(prompts, N_STEPS)
    mat, lens, stride = m._prompts(prompts)
    r = _lib.generate_request(prompts=_lib.ptr(mat), prompt_stride=stride, prompt_lens=_lib.ptr(lens), n_steps=N_STEPS)
    none = np.full(B, NONE, np.uint64)
    assert zg.zg_gpt_generate_guided_enqueue(m.h, C.addressof(r), None, 0, _lib.ptr(none)) == 0
    assert np.array_equal(m.generate_fetch(N_STEPS), want)
    m.close()


def test_states_of_one_keep_set_equal_the_static_allow_list_bit_for_bit(zg, weights):
    """The three states of SAME allow one set: the generation is the static allow-list's — tokens and the log-probability record, bit
    for bit — while the state walks (token t leads to state t mod 3), one row beside it without a guide being what it is alone."""
    B, top_n = 3, 6
    m = make(weights, B, logprobs_generate=True, edited_generate=True, sampled_generate=True)
    prompts = ragged(B, 930)
    want = m.generate_sample(prompts, N_STEPS, 0.8, seed=9, logprobs=top_n, allowed_token_ids=SAME_IDS)
    free = m.generate_sample(prompts, N_STEPS, 0.8, seed=9, logprobs=top_n)
    got = m.generate_sample(prompts, N_STEPS, 0.8, seed=9, logprobs=top_n, guide_states=[OFF_SAME, None, OFF_SAME + 2])
    rec = m.generate_fetch_guide_states(0, N_STEPS)
    for b, ref in ((0, want), (1, free), (2, want)):
        picked = ~np.isnan(ref[1][b])
        assert np.array_equal(got[0][b], ref[0][b]), (b, "tokens")
        assert np.array_equal(np.isnan(got[1][b]), ~picked)
        assert np.array_equal(u32(got[1][b][picked]), u32(ref[1][b][picked])), (b, "logprob")
        assert np.array_equal(got[2][b][picked], ref[2][b][picked]), (b, "top ids")
        assert np.array_equal(u32(got[3][b][picked]), u32(ref[3][b][picked])), (b, "top logprobs")
    for b in (0, 2):
        np_b = len(prompts[b])
        walk = [OFF_SAME + (0 if b == 0 else 2)] + [OFF_SAME + int(t) % 3 for t in got[0][b, np_b: N_STEPS - 1]]
        assert [int(s) for s in rec[b, np_b:]] == walk and (rec[b, :np_b] == NONE).all()
        assert len(set(walk)) == 3, "the row visited every state"
    assert (rec[1] == NONE).all()
    m.close()


def test_choices_end_at_the_end_token(zg, weights):
    B = 3
    m = make(weights, B)
    prompts = ragged(B, 940)
    seen = set()
    for seed in range(6):
        out = m.generate_sample(prompts, 40, 1.5, seed=seed, stop_token_ids=[END], guide_states=[OFF_CHOICE] * B)
        end, fin, why = m.stop_result()
        assert out.shape[1] == end
        for b in range(B):
            assert fin[b] is not None and why[b] == 0 and int(out[b, fin[b]]) == END
            label = [int(t) for t in out[b, len(prompts[b]): fin[b]]]
            assert label in CHOICES, (b, label)
            seen.add(tuple(label))
            assert (out[b, fin[b]:] == END).all(), "a finished row keeps decoding in lock step, on the end token"
    assert len(seen) >= 2, seen
    m.close()


def fed_tokens(prompt, out, n1):
    prompt = [int(t) for t in prompt]
    return np.array([prompt[s] if s < len(prompt) else prompt[-1] if s == len(prompt) else int(out[s - 1]) for s in range(n1)], np.uint64)


def test_second_turn_continues_from_the_fetched_record(zg, weights):
    """Handles without the whole-prompt pass: every position goes through the decode step in both runs, so the caches — and with them
    the draws — are the same bits."""
    B, n1, n2 = 3, 30, 45
    prompts = ragged(B, 950)
    turns = [synth.rand_tokens(960 + b, 1 + b, V) for b in range(B)]
    starts = [OFF_RAND + 1, None, OFF_RAND + 5]
    m = make(weights, B, prefill=False)
    out1 = m.generate_sample(prompts, n1, 0.8, seed=4, top_k=20, guide_states=starts)
    rec1 = m.generate_fetch_guide_states(0, n1)
    nxt = [None if rec1[b, n1 - 1] == NONE else UNION.step(int(rec1[b, n1 - 1]), int(out1[b, n1 - 1])) for b in range(B)]
    assert nxt[1] is None and nxt[0] is not None
    out2 = m.generate_from(n1, turns, n2, temp=0.8, seed=4, top_k=20, guide_states=nxt)
    assert m.cached_len() == n1 + n2
    rec = m.generate_fetch_guide_states(0, n1 + n2)
    assert np.array_equal(rec[:, :n1], rec1), "the first turn's record stays"
    m.close()
    full = [np.concatenate([fed_tokens(prompts[b], out1[b], n1), np.asarray(turns[b], np.uint64)]) for b in range(B)]
    fresh = make(weights, B, prefill=False)
    whole = fresh.generate_sample(full, n1 + n2, 0.8, seed=4, top_k=20, guide_states=nxt)
    rec_whole = fresh.generate_fetch_guide_states(0, n1 + n2)
    fresh.close()
    assert np.array_equal(whole[:, n1:], out2)
    assert np.array_equal(rec_whole[:, n1:], rec[:, n1:])
    for b in (0, 2):
        assert (rec[b, n1 + len(turns[b]):] != NONE).all() and (rec[b, n1: n1 + len(turns[b])] == NONE).all()


def guided(zg, m, prompts, n, opt, starts, edits=None, rows=None, past=0):
    mat, lens, stride = m._prompts(prompts)
    r = _lib.generate_request(past_len=past, prompts=_lib.ptr(mat), prompt_stride=stride, prompt_lens=_lib.ptr(lens), n_steps=n,
                              options=None if opt is None else C.addressof(opt), seed=3, edits=None if edits is None else C.addressof(edits))
    st = None if starts is None else np.array([NONE if s is None else s for s in starts], np.uint64)
    return zg.zg_gpt_generate_guided_enqueue(m.h, C.addressof(r), None if rows is None else C.addressof(rows), 0 if rows is None else len(rows), _lib.ptr(st))


def test_refusals_leave_the_handle_and_the_records_alone(zg, weights):
    B, n = 2, 24
    prompts = ragged(B, 970)
    m = make(weights, B)
    starts = [OFF_RAND, OFF_CHOICE]
    got, lp, ids, top = m.generate_sample(prompts, n, 0.8, seed=2, top_k=5, logprobs=2, guide_states=starts)
    rec = m.generate_fetch_guide_states(0, n)
    opt = _lib.SampleOptions(0.8, 5, 1.0)
    P = _lib.ptr
    only7 = np.array([7], np.uint64)          # no state of RAND allows token 7
    ends = np.array([END], np.uint64)         # the done state of CHOICE allows the end token alone
    table = _lib.row_sampling([dict(temp=0.8, seed=1)] * B)
    cases = [
        (opt, [OFF_RAND, UNION.n_states], None, None, ARG),                                    # a state the table does not have
        (None, starts, None, None, ARG),                                                       # greedy with a guided row
        (opt, None, None, None, ARG),                                                          # null start states
        (opt, starts, _lib.LogitEdits(None, None, 0, P(only7), 1, None, 0, 0.0), None, ARG),   # an empty kept set in every state
        (opt, [OFF_RAND, None], _lib.LogitEdits(None, None, 0, None, 0, P(ends), 1, 0.0), None, ARG),  # ... in a state no row can reach
        (None, starts, _lib.LogitEdits(None, None, 0, None, 0, None, 0, 0.1), table, ARG),     # the each call's own rule: min_p beside rows
        (opt, starts, None, table, ARG),                                                       # ... and options beside rows
    ]
    for o, st, e, rows, code in cases:
        assert guided(zg, m, prompts, 30, o, st, e, rows) == code, (code, zg.zg_last_error())
        assert m.cached_len() == n
    r = _lib.generate_request()
    r.size -= 8
    st = np.zeros(B, np.uint64)
    assert zg.zg_gpt_generate_guided_enqueue(m.h, C.addressof(r), None, 0, P(st)) == ARG and zg.zg_gpt_generate_guided_enqueue(m.h, None, None, 0, P(st)) == ARG
    # a bad table is refused and the loaded one stays; without a table a guided row is refused, an unguided call is not
    dead = np.full((2, V), DEAD, np.uint16)
    bad = _lib.Guide(2, P(dead))
    assert zg.zg_gpt_guide_load(m.h, C.addressof(bad)) == ARG and b"state 0 allows no token" in zg.zg_last_error()
    assert m.cached_len() == n
    lp1, ids1, top1 = m.generate_fetch_logprobs(0, n, 2)  # the records of the last good generation are still there, untouched
    assert np.array_equal(u32(lp), u32(lp1)) and np.array_equal(ids, ids1) and np.array_equal(m.generate_fetch_range(0, n), got)
    assert np.array_equal(m.generate_fetch_guide_states(0, n), rec)
    again = m.generate_sample(prompts, n, 0.8, seed=2, top_k=5, logprobs=2, guide_states=starts)  # and the handle still works
    assert np.array_equal(again[0], got) and np.array_equal(m.generate_fetch_guide_states(0, n), rec)
    m.generate_sample(prompts, n, 0.8, seed=2)
    with pytest.raises(_lib.ZgError) as err:  # the last generation was not a guided one
        m.generate_fetch_guide_states(0, n)
    assert err.value.code == ARG
    m.load_guide(None)
    assert guided(zg, m, prompts, n, opt, starts) == ARG and b"no guide is loaded" in zg.zg_last_error()
    assert guided(zg, m, prompts, n, opt, [None, None]) == 0
    assert np.array_equal(m.generate_fetch(n), m.generate_sample(prompts, n, 0.8, seed=3, top_k=5))
    m.close()


def test_a_handle_without_the_flag(zg, weights):
    m = zgpt.GPT(CFG, batch=1)
    m.load_weights(weights)
    g = UNION.c_struct()
    assert zg.zg_gpt_guide_load(m.h, C.addressof(g)) == UNSUPPORTED and zg.zg_gpt_guide_load(m.h, None) == UNSUPPORTED
    opt = _lib.SampleOptions(0.8, 0, 1.0)
    prompts = ragged(1, 980)
    assert guided(zg, m, prompts, 10, opt, [0]) == UNSUPPORTED and guided(zg, m, prompts, 10, opt, [None]) == UNSUPPORTED
    out = np.zeros(10, np.uint64)
    assert zg.zg_gpt_generate_fetch_guide_states(m.h, 0, 10, _lib.ptr(out), 10) == UNSUPPORTED
    assert np.array_equal(m.generate_sample(prompts, 10, 0.8, seed=1), m.generate_sample(prompts, 10, 0.8, seed=1))
    m.close()
