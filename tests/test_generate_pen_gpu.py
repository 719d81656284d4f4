"""zg_gpt_generate_pen_enqueue: the device loop with the penalty stage in its captured step equals, token for token, the host loop over
zg_gpt_sample_pen whose history is the caller's prior followed by the tokens recorded from past_len on (include/zgpt2.h).

The model has gpt_tiny's shapes with a context of 96, so that 80 steps cross a 64-position bucket; ragged prompts of 1 + 2 (b mod 3)
tokens make the loop leave and re-enter the alignment of its multi-step graphs."""
import ctypes as C

import numpy as np
import pytest

from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu
CFG = synth.GPTConfig(257, 96, 2, 2, 128)
N_STEPS = 80
PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.15)
MODES = [(0.8, 0, 1.0), (0.8, 7, 1.0), (1.1, 12, 0.8)]  # plain, top-k only, top-k + top-p


@pytest.fixture(scope="module")
def weights():
    return synth.make_weights(CFG, seed=81, bf16=True)


def make(w, batch, **kw):
    m = zgpt.GPT(CFG, batch=batch, **kw)
    m.load_weights(w)
    return m


def ragged(batch, seed):
    return [synth.rand_tokens(seed + b, 1 + 2 * (b % 3), CFG.vocab_size) for b in range(batch)]


def host_loop(m, prompts, n_steps, temp, seed, top_k, top_p, pen, past=0, prior=None):
    """generate's token logic around zg_gpt_sample_pen: at step s the history of a row is its prior and what positions past .. s - 1
    recorded; the row's own prompt token is fed while the prompt lasts, its last one twice."""
    B = len(prompts)
    out = np.zeros((B, n_steps), np.uint64)
    draws = [0] * B
    min_np = min(len(p) for p in prompts)
    for i in range(n_steps):
        toks = [int(p[i]) if i < len(p) else (int(p[-1]) if i == len(p) else int(draws[b])) for b, p in enumerate(prompts)]
        if i >= min_np:
            hist = [np.r_[np.asarray([] if prior is None else prior[b], np.uint64), out[b, :i]] for b in range(B)]
            draws = m.sample(past + i + 1, toks, temp, seed=seed, top_k=top_k, top_p=top_p, history=hist, **pen)
        else:
            m.forward(past + i + 1, toks, compute_logits=False)
        for b, p in enumerate(prompts):
            out[b, i] = toks[b] if i < len(p) else draws[b]
    return out


@pytest.mark.parametrize("batch,graph", [(1, True), (1, False), (3, True)])
def test_device_loop_equals_host_loop(zg, weights, batch, graph):
    prompts = ragged(batch, 810)
    m = make(weights, batch, use_graph=graph)
    plain = m.generate_sample(prompts, N_STEPS, 0.8, seed=5)
    for (temp, k, p), seed in zip(MODES, (5, 123456789, 9)):
        got = m.generate_sample(prompts, N_STEPS, temp, seed=seed, top_k=k, top_p=p, **PEN)
        want = host_loop(m, prompts, N_STEPS, temp, seed, k, p, PEN)
        again = m.generate_sample(prompts, N_STEPS, temp, seed=seed, top_k=k, top_p=p, **PEN)
        assert np.array_equal(got, want), (k, p, np.argwhere(got != want)[:4])
        assert np.array_equal(got, again)
        for b, pr in enumerate(prompts):
            assert np.array_equal(got[b, : len(pr)], pr)
    assert not np.array_equal(m.generate_sample(prompts, N_STEPS, 0.8, seed=5, **PEN), plain), "the penalties changed nothing"
    assert np.array_equal(m.generate_sample(prompts, N_STEPS, 0.8, seed=5), plain), "an ordinary generation behind penalised ones"
    m.close()


@pytest.mark.parametrize("with_prior", [False, True])
def test_behind_an_extend_with_and_without_a_prior(zg, weights, with_prior):
    B, past, n = 2, 13, 60
    first = np.stack([synth.rand_tokens(820 + b, past, CFG.vocab_size) for b in range(B)])
    turns = [synth.rand_tokens(830 + b, 2 + 3 * b, CFG.vocab_size) for b in range(B)]  # 2 and 5 new tokens: through the decode loop and ragged
    prior = [first[0], first[1][:5]] if with_prior else None  # (ragged; row 1 passes only some of its past)
    m = make(weights, B)
    m.extend(0, first, compute_logits=False)
    got = m.generate_from(past, turns, n, temp=0.8, seed=21, top_k=9, top_p=0.9, prior=prior, **PEN)
    assert m.cached_len() == past + n
    m.extend(0, first, compute_logits=False)
    want = host_loop(m, turns, n, 0.8, 21, 9, 0.9, PEN, past=past, prior=prior)
    # the tokens recorded below past_len are not read: a record of other tokens there changes nothing
    m.generate(list(first[::-1]), past)
    m.extend(0, first, compute_logits=False)
    again = m.generate_from(past, turns, n, temp=0.8, seed=21, top_k=9, top_p=0.9, prior=prior, **PEN)
    m.close()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert np.array_equal(got, again)


def test_prior_changes_the_tokens_and_a_long_turn_takes_the_whole_prompt_pass(zg, weights):
    B, n = 2, 50
    prompts = [synth.rand_tokens(840 + b, 6 + b, CFG.vocab_size) for b in range(B)]  # >= 4 tokens each: the whole-prompt pass feeds them
    m = make(weights, B)
    got = m.generate_sample(prompts, n, 0.8, seed=4, top_k=20, **PEN)
    want = host_loop(m, prompts, n, 0.8, 4, 20, 1.0, PEN)
    prior = [got[b, 6 + b: 6 + b + 8] for b in range(B)]  # tokens the rows are about to pick
    other = m.generate_sample(prompts, n, 0.8, seed=4, top_k=20, prior=prior, **PEN)
    want_other = host_loop(m, prompts, n, 0.8, 4, 20, 1.0, PEN, prior=prior)
    m.close()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert np.array_equal(other, want_other), np.argwhere(other != want_other)[:4]
    assert not np.array_equal(got, other)


@pytest.mark.parametrize("at_create", [True, False])
def test_graphs_at_create_or_at_the_first_generation(zg, weights, at_create):
    prompts = ragged(3, 850)
    m = make(weights, 3, penalized_generate=at_create)
    first = m.generate_sample(prompts, N_STEPS, 0.8, seed=7, top_k=7, **PEN)
    second = m.generate_sample(prompts, N_STEPS, 0.8, seed=7, top_k=7, **PEN)
    m.close()
    ref = make(weights, 3, use_graph=False)
    want = ref.generate_sample(prompts, N_STEPS, 0.8, seed=7, top_k=7, **PEN)
    ref.close()
    assert np.array_equal(first, second) and np.array_equal(first, want)


@pytest.mark.parametrize("batch", [1, 3])
def test_a_huge_presence_penalty_never_repeats_a_token(zg, weights, batch):
    """presence = 1e9 with top_k = 1: every token a row picks is distinct from everything the row held before it."""
    prompts = ragged(batch, 860)
    m = make(weights, batch)
    got = m.generate_sample(prompts, N_STEPS, 1.0, seed=1, top_k=1, presence_penalty=1.0e9)
    m.close()
    assert N_STEPS <= CFG.vocab_size
    for b, p in enumerate(prompts):
        for s in range(len(p), N_STEPS):
            assert int(got[b, s]) not in set(int(t) for t in got[b, :s]), (b, s, got[b, : s + 1])


def test_all_off_is_generate_sample_ex(zg, weights):
    prompts = ragged(3, 870)
    m = make(weights, 3)
    mat, lens, stride = m._prompts(prompts)
    off = _lib.LogitPenalties(1.0, 0.0, 0.0)
    prior = np.ascontiguousarray(np.arange(12).reshape(3, 4), np.uint64)
    plens = np.ascontiguousarray([4, 1, 0], np.uint64)
    for k, p in ((0, 1.0), (7, 0.9)):
        want = m.generate_sample(prompts, N_STEPS, 0.8, seed=3, top_k=k, top_p=p)
        opt = _lib.SampleOptions(0.8, k, p)
        _lib.check(zg.zg_gpt_generate_pen_enqueue(m.h, 0, _lib.ptr(mat), stride, _lib.ptr(lens), N_STEPS, C.addressof(opt), C.addressof(off), _lib.ptr(prior), 4,
                                                  _lib.ptr(plens), 3))
        assert np.array_equal(m.generate_fetch(N_STEPS), want), (k, p)
    m.close()
