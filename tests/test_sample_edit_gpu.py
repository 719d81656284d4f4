"""zg_gpt_sample_edit on the tiny synthetic models: the per-token sampler with the edit stage behind the penalties.

Probabilities, kept sets, thresholds and draws are held by test_edit_rows_gpu.check to the references applied to the device's own
raw logits (read back by zg_gpt_forward at the same position): penalty_ref.penalize_row first where the call penalises, then
edit_ref.edit_row, then edit_ref.filter_row_edit.  The bias ids lie in the histories, where (x penalised) + v and (x + v) penalised
differ: that is what proves the order.  The per-token call returns neither the edited row nor a threshold (min-p's is no element of
the row, so it cannot be read off the kept set either): the kept sets are compared exactly instead.  top_p values are
taken from a short list, the first at which every reference row has test_sample_filter_gpu's 1e-4 margin (checked on the CPU)."""
import ctypes as C

import numpy as np
import pytest

from edit_ref import edit_row, filter_row_edit
from penalty_ref import penalize_row
from test_edit_rows_gpu import bits, check
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


def model_runner(m, seq_len, toks, hists, pen):
    """edit_rows' signature answered by zg_gpt_sample_edit at one position of a model (x is the reference's row in front of the edit
    stage and is not sent anywhere)."""

    def run(x, temp, top_k, top_p, u, bias=None, allowed=None, banned=None, min_p=0.0, want_probs=True, want_edited=True):
        try:
            tok, probs = m.sample(seq_len, toks, temp, uniforms=u, want_probs=True, top_k=top_k, top_p=top_p, history=hists, logit_bias=bias,
                                  allowed_token_ids=allowed, banned_token_ids=banned, min_p=min_p, **pen)
        except _lib.ZgError as e:
            return e.code, None, None, None, None
        return 0, None, tok, probs, None

    return run


def margin_top_p(rows, temp, top_k, min_p):
    for p in (0.9, 0.85, 0.8, 0.75, 0.7):
        if all(min(abs(float(np.float32(p)) - c) for c in filter_row_edit(y, temp, top_k, 1.0, min_p).cum) >= 1e-4 for y in rows):
            return p
    raise AssertionError("no top_p with the margin")


@pytest.mark.parametrize("name,batch", [("tiny", 1), ("tiny3", 3), ("tiny", 8)])
def test_probabilities_kept_sets_and_draws_against_the_references(zg, name, batch):
    cfg, m = make(name, batch, 91)
    V = cfg.vocab_size
    rng = np.random.default_rng(9100 + batch)
    toks = [int(t) for t in rng.integers(0, V, batch)]
    for T in (1, 2, 3):
        raw = m.forward(T, toks)  # the row in front of both stages; zg_gpt_sample_edit recomputes it at the same position
        order = np.argsort(-raw, axis=1)
        hists = [np.r_[order[b, : 3 + 2 * b], order[b, :2], order[b, 0]].astype(np.uint64) if b != 1 else np.zeros(0, np.uint64) for b in range(batch)]
        # one set for every row: biases on row 0's likeliest tokens (in its history) and on index 0 and V - 1, its 2nd banned
        bias = {int(order[0, 0]): -1.5, int(order[0, 2]): 2.5, 0: 0.75, V - 1: -0.5}
        bias = {k: v for k, v in bias.items() if k != int(order[0, 1])} | {int(order[0, 3]): 1.0}
        banned = [int(order[0, 1]), int(order[batch - 1, 4])]
        allowed = sorted({int(i) for i in order[:, :40].ravel()} | {0, V - 1})
        for pen in ({}, PEN):
            base = np.stack([penalize_row(raw[b], hists[b], 1.3, 0.4, 0.15)[0] for b in range(batch)]) if pen else raw
            run = model_runner(m, T, toks, hists, pen)
            for kw in (dict(bias=bias, banned=banned), dict(bias=bias, allowed=allowed, banned=banned), {}):
                y = np.stack([edit_row(base[b], kw.get("bias"), kw.get("allowed"), kw.get("banned")) for b in range(batch)])
                for temp, k, mp in ((0.8, 0, 0.0), (0.8, 7, 0.05), (0.8, 0, 0.05)):
                    if not kw and mp == 0.0:
                        continue  # (everything off: the twin test below)
                    check(run, base, temp, k, 1.0, mp, f"{name} B {batch} T {T} pen {bool(pen)} {sorted(kw)} temp {temp} k {k} min_p {mp}", n_u=40, **kw)
                if T == 2:
                    p = margin_top_p(y, 1.7, 12, 0.02)
                    check(run, base, 1.7, 12, p, 0.02, f"{name} B {batch} T {T} pen {bool(pen)} {sorted(kw)} k 12 p {p} min_p 0.02", n_u=40, **kw)
        toks = [int(t) for t in m.sample(T, toks, 0.8, seed=3)]
    m.close()


@pytest.mark.parametrize("name,batch", [("tiny", 1), ("tiny3", 3)])
def test_argmax_and_the_row_maximum_follow_the_edited_row(zg, name, batch):
    cfg, m = make(name, batch, 92)
    V = cfg.vocab_size
    toks = [5 + b for b in range(batch)]
    raw = m.forward(1, toks)
    top = raw.argmax(axis=1)
    # 1. every row's argmax, and every runner-up nearer than a sixth of the vocabulary to its own old argmax, banned
    banned, rest = set(), raw.copy()
    while True:
        nt = rest.argmax(axis=1)
        close = [b for b in range(batch) if abs(int(nt[b]) - int(top[b])) < V // 6]
        if not close:
            break
        banned.update(int(nt[b]) for b in close)
        rest[:, sorted(banned)] = -np.inf
    new_top = [int(t) for t in nt]
    got, probs = m.sample(1, toks, 0.8, seed=1, top_k=1, want_probs=True, banned_token_ids=sorted(banned))
    assert [int(t) for t in got] == new_top, (got, new_top, top)
    assert [int(t) for t in m.argmax()] == new_top  # zg_gpt_argmax follows the edited row
    for b in range(batch):
        assert probs[b, new_top[b]] == 1.0 and np.count_nonzero(probs[b]) == 1
    # 2. +1e4 on the least likely token at least V / 6 away from every row's old argmax
    far = np.abs(np.arange(V)[None, :] - top[:, None]).min(axis=0) >= V // 6
    assert far.any()
    low = int(np.where(far, raw.sum(axis=0), np.inf).argmin())
    got, probs = m.sample(1, toks, 0.8, seed=1, top_k=1, want_probs=True, logit_bias={low: 1.0e4})
    assert [int(t) for t in got] == [low] * batch and [int(t) for t in m.argmax()] == [low] * batch
    for b in range(batch):
        assert probs[b, low] == 1.0 and np.count_nonzero(probs[b]) == 1
    # the same through the plain sampler, and through min-p alone: all of the mass sits on the one token
    assert [int(t) for t in m.sample(1, toks, 0.8, seed=1, logit_bias={low: 1.0e4})] == [low] * batch
    got, probs = m.sample(1, toks, 0.8, seed=1, want_probs=True, logit_bias={low: 1.0e4}, min_p=0.05)
    assert [int(t) for t in got] == [low] * batch and all(probs[b, low] == 1.0 and np.count_nonzero(probs[b]) == 1 for b in range(batch))
    # an allow-list of one token
    one = int(np.where(far, raw.sum(axis=0), -np.inf).argmax())
    assert [int(t) for t in m.sample(1, toks, 0.8, seed=1, allowed_token_ids=[one])] == [one] * batch
    assert [int(t) for t in m.argmax()] == [one] * batch
    m.close()


def test_everything_off_is_sample_pen_and_sample_ex_bit_for_bit(zg):
    cfg, m = make("tiny3", 3, 93)
    V = cfg.vocab_size
    toks = np.ascontiguousarray([3, 4, 5], np.uint64)
    hist = np.ascontiguousarray(np.arange(12).reshape(3, 4), np.uint64)
    lens = np.ascontiguousarray([4, 0, 2], np.uint64)
    pen, off = _lib.LogitPenalties(1.3, 0.4, 0.15), _lib.LogitEdits()
    for k, p in ((0, 1.0), (7, 1.0), (9, 0.85)):
        opt = _lib.SampleOptions(0.8, k, p)
        t = [np.zeros(3, np.uint64) for _ in range(4)]
        pr = [np.empty((3, V), np.float32) for _ in range(4)]
        _lib.check(zg.zg_gpt_sample_ex(m.h, 1, _lib.ptr(toks), 3, C.addressof(opt), None, 11, _lib.ptr(t[0]), _lib.ptr(pr[0]), pr[0].size))
        _lib.check(zg.zg_gpt_sample_edit(m.h, 1, _lib.ptr(toks), 3, C.addressof(opt), None, None, 0, None, C.addressof(off), None, 11, _lib.ptr(t[1]),
                                         _lib.ptr(pr[1]), pr[1].size))
        _lib.check(zg.zg_gpt_sample_pen(m.h, 1, _lib.ptr(toks), 3, C.addressof(opt), C.addressof(pen), _lib.ptr(hist), 4, _lib.ptr(lens), None, 11,
                                        _lib.ptr(t[2]), _lib.ptr(pr[2]), pr[2].size))
        _lib.check(zg.zg_gpt_sample_edit(m.h, 1, _lib.ptr(toks), 3, C.addressof(opt), C.addressof(pen), _lib.ptr(hist), 4, _lib.ptr(lens), C.addressof(off),
                                         None, 11, _lib.ptr(t[3]), _lib.ptr(pr[3]), pr[3].size))
        assert np.array_equal(t[0], t[1]) and np.array_equal(bits(pr[0]), bits(pr[1])), (k, p)
        assert np.array_equal(t[2], t[3]) and np.array_equal(bits(pr[2]), bits(pr[3])), (k, p)
    m.close()


def test_an_ordinary_call_behind_an_edited_one_is_unchanged(zg):
    cfg, m = make("tiny", 2, 94)
    toks = [9, 10]
    t0, p0 = m.sample(1, toks, 0.8, seed=5, top_k=6, want_probs=True)
    q0, r0 = m.sample(1, toks, 0.8, seed=5, want_probs=True)
    m.sample(1, toks, 0.8, seed=5, top_k=6, logit_bias={int(t0[0]): -50.0, 3: 4.0}, banned_token_ids=[int(t0[1])], min_p=0.3, history=[[1, 2, 3], [7]], **PEN)
    m.sample(1, toks, 0.8, seed=5, min_p=0.3)
    t1, p1 = m.sample(1, toks, 0.8, seed=5, top_k=6, want_probs=True)
    q1, r1 = m.sample(1, toks, 0.8, seed=5, want_probs=True)
    m.close()
    assert np.array_equal(t0, t1) and np.array_equal(bits(p0), bits(p1))
    assert np.array_equal(q0, q1) and np.array_equal(bits(r0), bits(r1))


def test_refusals_leave_the_handle_alone(zg):
    cfg, m = make("tiny", 2, 95)
    V = cfg.vocab_size
    m.forward(1, [1, 2])
    m.forward(2, [3, 4])
    assert m.cached_len() == 2
    for kw, code in ((dict(logit_bias={V: 1.0}), -2), (dict(banned_token_ids=[V + 3]), -2), (dict(allowed_token_ids=[V]), -2), (dict(min_p=1.0), -6),
                     (dict(min_p=-0.5), -6), (dict(logit_bias={1: float("inf")}), -6), (dict(banned_token_ids=list(range(V))), -6),
                     (dict(logit_bias={i: 1.0 for i in range(257)}, min_p=float("nan")), -6)):
        with pytest.raises(_lib.ZgError) as e:
            m.sample(1, [1, 2], 0.8, **kw)
        assert e.value.code == code, kw
        assert m.cached_len() == 2
    toks, out = np.ascontiguousarray([1, 2], np.uint64), np.zeros(2, np.uint64)
    opt = _lib.SampleOptions(0.8, 0, 1.0)
    assert zg.zg_gpt_sample_edit(m.h, 1, _lib.ptr(toks), 2, C.addressof(opt), None, None, 0, None, None, None, 0, _lib.ptr(out), None, 0) == -6  # NULL edits
    assert zg.zg_gpt_sample_edit(m.h, 1, _lib.ptr(toks), 2, None, None, None, 0, None, C.addressof(_lib.LogitEdits()), None, 0, _lib.ptr(out), None, 0) == -6
    assert m.cached_len() == 2
    assert (m.sample(3, [5, 6], 0.8, min_p=0.05, banned_token_ids=[0]) < V).all()  # the handle still works
    m.close()
