"""Every zg_gpt_generate*_enqueue entry point that zg_gpt_generate_request_enqueue subsumes against the request call with exactly
the same fields: identical token arrays and, where log-probabilities are recorded, identical bytes of
zg_gpt_generate_fetch_logprobs.  The other twin tests hold the request call to zg_gpt_generate_stop_enqueue and that to the host
loops; this one closes the chain from the older entry points.

gpt_tiny's golden weights at batch 3 and a context of 48.  Ragged prompts of 5, 7 and 9 tokens and 30 positions: the whole-prompt
pass takes the first 5, single steps follow up to position 8, two replays of the 8-step graph up to 24, single steps again to the
end.  Once with graphs and once on a ZG_GPT_NO_GRAPH handle, whose every step is enqueued launch by launch."""
import ctypes as C

import numpy as np
import pytest

from golden_io import load_gpt
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu
B, CTX, N, PAST = 3, 48, 30, 6
P = _lib.ptr
PEN = (1.3, 0.4, 0.15)


@pytest.fixture(scope="module")
def model_weights():
    cfg, g = load_gpt("tiny")
    w = dict(synth.make_weights(cfg, seed=int(g["weight_seed"]), bf16=True))
    w["wpe"] = np.ascontiguousarray(w["wpe"][:CTX])
    return synth.GPTConfig(cfg.vocab_size, CTX, cfg.n_layer, cfg.n_heads, cfg.n_embed), w


@pytest.fixture(scope="module", params=[True, False], ids=["graphs", "no_graph"])
def model(zg, model_weights, request):
    cfg, w = model_weights
    m = zgpt.GPT(cfg, batch=B, use_graph=request.param)
    m.load_weights(w)
    yield m
    m.close()


def prompts_of(m, seed):
    return m._prompts([synth.rand_tokens(seed + b, 5 + 2 * b, m.config.vocab_size) for b in range(B)])


def by_request(zg, m, mat, lens, stride, n, past=0, opt=None, pen=None, prior=None, seed=0, logprobs=0, top_n=0):
    pm, plens, pstride = prior if prior is not None else (None, None, 0)
    r = _lib.generate_request(past_len=past, prompts=P(mat), prompt_stride=stride, prompt_lens=P(lens), n_steps=n,
                              options=None if opt is None else C.addressof(opt), penalties=None if pen is None else C.addressof(pen), prior=P(pm),
                              prior_stride=pstride, prior_lens=P(plens), seed=seed, logprobs=logprobs, top_n=top_n)
    _lib.check(zg.zg_gpt_generate_request_enqueue(m.h, C.addressof(r)))


def record(m, past, n, top_n=None):
    """What a generation left: its tokens and (top_n given) the bytes of its log-probability record"""
    out = (m.generate_fetch_range(past, n),)
    if top_n is not None:
        out += tuple(a.tobytes() for a in m.generate_fetch_logprobs(past, n, top_n))
    return out


def assert_same(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, np.argwhere(a[0] != b[0])[:4])
    assert a[1:] == b[1:], (what, "the log-probability records differ")


def test_greedy_and_sampled(zg, model):
    m = model
    mat, lens, stride = prompts_of(m, 700)
    head = (P(mat), stride, P(lens), N)
    _lib.check(zg.zg_gpt_generate_enqueue(m.h, *head))
    old = record(m, 0, N)
    by_request(zg, m, mat, lens, stride, N)
    assert_same(old, record(m, 0, N), "generate_enqueue")
    _lib.check(zg.zg_gpt_generate_sample_enqueue(m.h, *head, 0.8, 11))
    sampled = record(m, 0, N)
    by_request(zg, m, mat, lens, stride, N, opt=_lib.SampleOptions(0.8, 0, 1.0), seed=11)
    assert_same(sampled, record(m, 0, N), "generate_sample_enqueue")
    assert not np.array_equal(sampled[0], old[0]), "the sampler drew the greedy tokens"
    for opt in (_lib.SampleOptions(0.8, 7, 1.0), _lib.SampleOptions(1.1, 12, 0.8)):  # one filter, two filters
        _lib.check(zg.zg_gpt_generate_sample_ex_enqueue(m.h, *head, C.addressof(opt), 12))
        got = record(m, 0, N)
        by_request(zg, m, mat, lens, stride, N, opt=opt, seed=12)
        assert_same(got, record(m, 0, N), ("generate_sample_ex_enqueue", opt.top_k, opt.top_p))
        assert not np.array_equal(got[0], sampled[0]), "the filters changed nothing"


def test_continuations(zg, model):
    m = model
    first = m._prompts([synth.rand_tokens(720 + b, 2 + b, m.config.vocab_size) for b in range(B)])
    mat, lens, stride = prompts_of(m, 730)
    n = N - PAST
    for opt in (None, _lib.SampleOptions(0.9, 9, 0.9)):
        res = []
        for twin in (False, True):
            _lib.check(zg.zg_gpt_generate_enqueue(m.h, P(first[0]), first[2], P(first[1]), PAST))
            if twin:
                by_request(zg, m, mat, lens, stride, n, past=PAST, opt=opt, seed=13)
            else:
                _lib.check(zg.zg_gpt_generate_from_enqueue(m.h, PAST, P(mat), stride, P(lens), n, None if opt is None else C.addressof(opt), 13))
            assert m.cached_len() == N
            res.append(record(m, 0, N))
        assert_same(res[0], res[1], ("generate_from_enqueue", opt is not None))


def test_penalties_with_a_prior(zg, model):
    m = model
    mat, lens, stride = prompts_of(m, 740)
    prior = m._prompts([synth.rand_tokens(750 + b, 4 + 3 * b, m.config.vocab_size) for b in range(B)])
    opt, pen = _lib.SampleOptions(0.8, 7, 0.9), _lib.LogitPenalties(*PEN)
    _lib.check(zg.zg_gpt_generate_pen_enqueue(m.h, 0, P(mat), stride, P(lens), N, C.addressof(opt), C.addressof(pen), P(prior[0]), prior[2], P(prior[1]), 14))
    old = record(m, 0, N)
    by_request(zg, m, mat, lens, stride, N, opt=opt, pen=pen, prior=prior, seed=14)
    assert_same(old, record(m, 0, N), "generate_pen_enqueue")
    _lib.check(zg.zg_gpt_generate_sample_ex_enqueue(m.h, P(mat), stride, P(lens), N, C.addressof(opt), 14))
    assert not np.array_equal(record(m, 0, N)[0], old[0]), "the penalties changed nothing"


@pytest.mark.parametrize("top_n", [0, 5])
def test_logprobs(zg, model, top_n):
    m = model
    mat, lens, stride = prompts_of(m, 760)
    prior = m._prompts([synth.rand_tokens(770 + b, 3 + b, m.config.vocab_size) for b in range(B)])
    for opt, pen, pr in ((None, None, None), (_lib.SampleOptions(0.8, 7, 0.9), _lib.LogitPenalties(*PEN), prior)):
        pm, plens, pstride = pr if pr is not None else (None, None, 0)
        _lib.check(zg.zg_gpt_generate_logprobs_enqueue(m.h, 0, P(mat), stride, P(lens), N, None if opt is None else C.addressof(opt),
                                                       None if pen is None else C.addressof(pen), P(pm), pstride, P(plens), 15, top_n))
        old = record(m, 0, N, top_n)
        by_request(zg, m, mat, lens, stride, N, opt=opt, pen=pen, prior=pr, seed=15, logprobs=1, top_n=top_n)
        assert_same(old, record(m, 0, N, top_n), ("generate_logprobs_enqueue", opt is not None, top_n))
        lp = np.frombuffer(old[1], np.float32).reshape(B, N)
        for b in range(B):  # the record is a record: NaN on the prompt columns, a log-probability on every pick
            assert np.isnan(lp[b, : int(lens[b])]).all() and (lp[b, int(lens[b]):] <= 0.0).all()
