"""Bad arguments of the penalised entry points: each returns its status before anything is enqueued — zg_gpt_cached_len and a
following ordinary generation are what they were — and a handle beyond the context cap is refused by the new entry points only."""
import ctypes as C

import numpy as np
import pytest

from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu
ARG, SHAPE, UNSUPPORTED = -6, -2, -5
NAN, INF = float("nan"), float("inf")
BAD_PENALTIES = [(0.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (NAN, 0.0, 0.0), (1.2, NAN, 0.0), (1.2, INF, 0.0), (1.2, -INF, 0.0), (1.2, 0.0, NAN),
                 (1.2, 0.0, INF)]


def u64(a):
    return np.ascontiguousarray(a, np.uint64)


def test_bad_arguments_are_refused_and_the_handle_is_untouched(zg):
    cfg = synth.CONFIGS["tiny"]
    V, Cx, B = cfg.vocab_size, cfg.context_size, 2
    m = zgpt.GPT(cfg, batch=B)
    m.load_weights(synth.make_weights(cfg, seed=91, bf16=True))
    prompts = [synth.rand_tokens(910 + b, 2 + b, V) for b in range(B)]
    want = m.generate_sample(prompts, 30, 0.8, seed=2, top_k=5, top_p=0.9)
    m.extend(0, np.stack([synth.rand_tokens(920 + b, 9, V) for b in range(B)]), compute_logits=False)
    assert m.cached_len() == 9
    mat, lens, stride = m._prompts(prompts)
    tok, one = np.zeros(B, np.uint64), u64([3, 4])
    opt, pen = _lib.SampleOptions(0.8, 5, 0.9), _lib.LogitPenalties(1.2, 0.1, 0.1)
    hist, hlen = u64(np.arange(2 * Cx).reshape(2, Cx) % V), u64([3, 0])

    def sample(o=opt, p=pen, h=hist, hs=Cx, hl=hlen):
        return zg.zg_gpt_sample_pen(m.h, 10, _lib.ptr(one), B, None if o is None else C.addressof(o), None if p is None else C.addressof(p), _lib.ptr(h), hs,
                                    _lib.ptr(hl), None, 2, _lib.ptr(tok), None, 0)

    def generate(o=opt, p=pen, pr=hist, ps=Cx, pl=hlen, n=30, past=9):
        return zg.zg_gpt_generate_pen_enqueue(m.h, past, _lib.ptr(mat), stride, _lib.ptr(lens), n, None if o is None else C.addressof(o),
                                              None if p is None else C.addressof(p), _lib.ptr(pr), ps, _lib.ptr(pl), 2)

    x, xo = np.zeros((B, V), np.float32), np.zeros((B, V), np.float32)

    def rows(p=pen, h=hist, hs=Cx, hl=hlen):
        return zg.zg_debug_penalize_rows(_lib.ptr(x), B, V, None if p is None else C.addressof(p), _lib.ptr(h), hs, _lib.ptr(hl), _lib.ptr(xo), None)

    calls = []
    for f in (sample, generate, rows):
        calls.append((f(p=None), ARG, f.__name__, "NULL penalties"))
        for r, pr, fr in BAD_PENALTIES:
            calls.append((f(p=_lib.LogitPenalties(r, pr, fr)), ARG, f.__name__, (r, pr, fr)))
    for f in (sample, generate):
        calls.append((f(o=None), ARG, f.__name__, "NULL options"))
        calls.append((f(o=_lib.SampleOptions(0.0, 5, 0.9)), ARG, f.__name__, "temperature 0"))
    too_big = hist.copy()
    too_big[0, 2] = V
    calls.append((sample(h=too_big), SHAPE, "sample", "history token >= vocab"))
    calls.append((generate(pr=too_big), SHAPE, "generate", "prior token >= vocab"))
    calls.append((rows(h=too_big), SHAPE, "rows", "history token >= vocab"))
    calls.append((sample(hs=2, hl=u64([3, 0])), SHAPE, "sample", "length beyond its stride"))
    calls.append((generate(ps=2, pl=u64([3, 0])), SHAPE, "generate", "length beyond its stride"))
    calls.append((rows(hs=2, hl=u64([3, 0])), SHAPE, "rows", "length beyond its stride"))
    wide = u64(np.zeros((2, Cx + 8)))
    calls.append((sample(h=wide, hs=Cx + 8, hl=u64([Cx + 1, 0])), SHAPE, "sample", "length beyond context_size"))
    calls.append((generate(pr=wide, ps=Cx + 8, pl=u64([0, Cx + 1])), SHAPE, "generate", "length beyond context_size"))
    calls.append((generate(pl=u64([Cx - 29, 0])), SHAPE, "generate", "prior + n_steps beyond context_size"))
    calls.append((generate(pr=hist, pl=None), ARG, "generate", "a prior without its lengths"))
    calls.append((generate(past=10), ARG, "generate", "past_len beyond the cached positions"))
    calls.append((generate(n=Cx), SHAPE, "generate", "n_steps beyond the context"))
    for rc, status, who, what in calls:
        assert rc == status, (who, what, rc, zg.zg_last_error())
        assert m.cached_len() == 9, (who, what)
    # the good calls still work: a prior that just fits, no prior at all
    assert generate(pl=u64([Cx - 30, 0])) == 0 and generate(pr=None, pl=None) == 0
    again = m.generate_sample(prompts, 30, 0.8, seed=2, top_k=5, top_p=0.9)
    m.close()
    assert np.array_equal(again, want)


def test_a_context_beyond_the_cap_is_unsupported_by_the_new_entry_points_only(zg):
    cfg = synth.GPTConfig(257, 8192 + 64, 1, 2, 128)
    m = zgpt.GPT(cfg, batch=1, use_graph=False, prefill=False)
    one, tok, lens0 = u64([3]), np.zeros(1, np.uint64), u64([0])
    opt, pen, off = _lib.SampleOptions(0.8, 5, 0.9), _lib.LogitPenalties(1.2, 0.1, 0.1), _lib.LogitPenalties(1.0, 0.0, 0.0)
    for p in (pen, off):
        assert zg.zg_gpt_sample_pen(m.h, 1, _lib.ptr(one), 1, C.addressof(opt), C.addressof(p), None, 0, _lib.ptr(lens0), None, 2, _lib.ptr(tok), None, 0) == UNSUPPORTED
        assert zg.zg_gpt_generate_pen_enqueue(m.h, 0, _lib.ptr(one), 1, _lib.ptr(u64([1])), 4, C.addressof(opt), C.addressof(p), None, 0, None, 2) == UNSUPPORTED
    assert m.cached_len() == 0
    # (the handle itself was created: nothing but the penalised calls knows the cap)
    m.close()
    with pytest.raises(_lib.ZgError) as e:
        zgpt.GPT(cfg, batch=1, prefill=False, penalized_generate=True)
    assert e.value.code == UNSUPPORTED
