"""zg_gpt_sample_pen on the tiny synthetic models: the per-token sampler with the penalty stage in front.

Probabilities, kept sets, thresholds and draws are held to trunc_ref.filter_row applied to the penalty_ref row of the device's own
raw logits (read back by zg_gpt_forward at the same position) — by test_sample_filter_gpu.check itself, so the tolerances and tie
rules are that file's: it is handed a stand-in for the library whose zg_debug_sample_rows runs zg_gpt_sample_pen on the model.  The
per-token call returns no threshold; the stand-in reports the smallest penalised logit it kept, which is the threshold whenever
the kept sets agree (and they are compared first).

The two stale-maximum cases: both samplers take the row maximum from lm_head's argmax partials, which the penalties invalidate.
lm_head's slices are contiguous index ranges, so a token at least a sixth of the vocabulary away from the old argmax lies in
another slice on every plan that has more than six of them."""
import ctypes as C

import numpy as np
import pytest

from penalty_ref import penalize_row
from test_sample_filter_gpu import check
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu
PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.15)


def make(name, batch, seed):
    cfg = synth.CONFIGS[name]
    m = zgpt.GPT(cfg, batch=batch)
    m.load_weights(synth.make_weights(cfg, seed=seed, bf16=True))
    return cfg, m


class ModelRows:
    """Answers zg_debug_sample_rows(logits, B, V, options, uniforms, tokens, probs, thresholds) with zg_gpt_sample_pen at one
    position of a model: the logits argument is the REFERENCE's penalised row and is not read."""

    def __init__(self, m, seq_len, toks, hists, pen, raw_penalised):
        self.m, self.seq_len, self.toks, self.hists, self.pen, self.rows = m, seq_len, toks, hists, pen, raw_penalised

    def zg_debug_sample_rows(self, logits, B, V, opt, u, tok, probs, thr):
        o = _lib.SampleOptions.from_address(opt)
        us = np.ctypeslib.as_array((C.c_float * B).from_address(u)).copy()
        try:
            got = self.m.sample(self.seq_len, self.toks, o.temp, uniforms=us, want_probs=True, top_k=o.top_k, top_p=o.top_p, history=self.hists, **self.pen)
        except _lib.ZgError as e:
            return e.code
        np.ctypeslib.as_array((C.c_uint64 * B).from_address(tok))[:] = got[0]
        if probs:
            np.ctypeslib.as_array((C.c_float * (B * V)).from_address(probs))[:] = got[1].ravel()
        taus = [np.float32(self.rows[b][got[1][b] != 0].min()) + np.float32(0.0) for b in range(B)]
        np.ctypeslib.as_array((C.c_float * B).from_address(thr))[:] = taus
        return 0


@pytest.mark.parametrize("name,batch", [("tiny", 1), ("tiny3", 3), ("tiny", 8)])
def test_probabilities_kept_sets_and_draws_against_the_references(zg, name, batch):
    cfg, m = make(name, batch, 71)
    V = cfg.vocab_size
    rng = np.random.default_rng(7100 + batch)
    toks = [int(t) for t in rng.integers(0, V, batch)]
    for T in (1, 2, 3):
        raw = m.forward(T, toks)  # the row the penalties act on; zg_gpt_sample_pen recomputes it at the same position
        order = np.argsort(-raw, axis=1)
        # histories over the most probable tokens (where a penalty changes the kept set), ragged, with duplicates; one row none
        hists = [np.r_[order[b, : 3 + 2 * b], order[b, :2], order[b, 0]].astype(np.uint64) if b != 1 else np.zeros(0, np.uint64) for b in range(batch)]
        want = np.stack([penalize_row(raw[b], hists[b], 1.3, 0.4, 0.15)[0] for b in range(batch)])
        shim = ModelRows(m, T, toks, hists, PEN, want)
        for temp, k, p in ((0.8, 0, 1.0), (0.8, 7, 1.0), (1.7, 0, 0.9), (0.8, 12, 0.8)):
            check(shim, want, temp, k, p, rng, f"{name} B {batch} T {T} temp {temp} k {k} p {p}", n_u=8)
        toks = [int(t) for t in m.sample(T, toks, 0.8, seed=3)]
    m.close()


@pytest.mark.parametrize("name,batch", [("tiny", 1), ("tiny3", 3)])
def test_stale_row_maximum(zg, name, batch):
    cfg, m = make(name, batch, 72)
    V = cfg.vocab_size
    toks = [5 + b for b in range(batch)]
    raw = m.forward(1, toks)
    top = raw.argmax(axis=1)
    # 1. the unpenalised argmax — and every runner-up nearer than a sixth of the vocabulary to it — is in the history and pushed far
    #    down: the new argmax lives in another slice
    hists, new_top = [], []
    for b in range(batch):
        rest, hist = raw[b].copy(), []
        while abs(int(rest.argmax()) - int(top[b])) < V // 6:
            hist.append(int(rest.argmax()))
            rest[hist[-1]] = -np.inf
        assert 1 <= len(hist) <= cfg.context_size
        hists.append(np.array(hist, np.uint64))
        new_top.append(int(rest.argmax()))
    got, probs = m.sample(1, toks, 0.8, seed=1, top_k=1, want_probs=True, presence_penalty=1.0e4, history=hists)
    assert [int(t) for t in got] == new_top, (got, new_top, top)
    assert [int(t) for t in m.argmax()] == new_top  # zg_gpt_argmax follows the penalised row
    for b in range(batch):
        assert probs[b, new_top[b]] == 1.0 and np.count_nonzero(probs[b]) == 1
    # 2. a negative presence lifts a history token (the least likely one, in another slice than the old maximum where the vocabulary
    #    allows) above the old maximum
    low = [int(np.where(np.abs(np.arange(V) - int(top[b])) >= V // 6, raw[b], np.inf).argmin()) for b in range(batch)]
    got, probs = m.sample(1, toks, 0.8, seed=1, top_k=1, want_probs=True, presence_penalty=-1.0e4, history=[[t] for t in low])
    assert [int(t) for t in got] == low, (got, low, top)
    assert [int(t) for t in m.argmax()] == low
    for b in range(batch):
        assert probs[b, low[b]] == 1.0 and np.count_nonzero(probs[b]) == 1
    # the same two through the plain sampler (no filter): all of the mass sits on the one token
    got = m.sample(1, toks, 0.8, seed=1, presence_penalty=-1.0e4, history=[[t] for t in low])
    assert [int(t) for t in got] == low
    m.close()


def test_all_off_is_sample_ex_bit_for_bit(zg):
    cfg, m = make("tiny3", 3, 73)
    V = cfg.vocab_size
    toks = np.ascontiguousarray([3, 4, 5], np.uint64)
    hist = np.ascontiguousarray(np.arange(12).reshape(3, 4), np.uint64)
    lens = np.ascontiguousarray([4, 0, 2], np.uint64)
    off = _lib.LogitPenalties(1.0, 0.0, 0.0)
    for k, p in ((0, 1.0), (7, 1.0), (9, 0.85)):
        opt = _lib.SampleOptions(0.8, k, p)
        t0, t1 = np.zeros(3, np.uint64), np.zeros(3, np.uint64)
        p0, p1 = np.empty((3, V), np.float32), np.empty((3, V), np.float32)
        _lib.check(zg.zg_gpt_sample_ex(m.h, 1, _lib.ptr(toks), 3, C.addressof(opt), None, 11, _lib.ptr(t0), _lib.ptr(p0), p0.size))
        _lib.check(zg.zg_gpt_sample_pen(m.h, 1, _lib.ptr(toks), 3, C.addressof(opt), C.addressof(off), _lib.ptr(hist), 4, _lib.ptr(lens), None, 11,
                                        _lib.ptr(t1), _lib.ptr(p1), p1.size))
        assert np.array_equal(t0, t1) and np.array_equal(p0.view(np.uint32), p1.view(np.uint32)), (k, p)
    m.close()


def test_an_ordinary_call_behind_a_penalised_one_is_unchanged(zg):
    cfg, m = make("tiny", 2, 74)
    toks = [9, 10]
    t0, p0 = m.sample(1, toks, 0.8, seed=5, top_k=6, want_probs=True)
    m.sample(1, toks, 0.8, seed=5, top_k=6, history=[[1, 2, 3], [int(t0[1])]], **PEN)
    t1, p1 = m.sample(1, toks, 0.8, seed=5, top_k=6, want_probs=True)
    g0 = m.argmax()
    m.close()
    assert np.array_equal(t0, t1) and np.array_equal(p0.view(np.uint32), p1.view(np.uint32))
    assert g0.shape == (2,)
