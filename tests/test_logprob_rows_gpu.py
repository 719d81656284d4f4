"""zg_debug_logprob_rows: the two kernels of the log-probability stage (csrc/sample_logprob.h) on hand-made rows against the float64
reference of tests/logprob_ref.py — ids exactly in the reference's order, values within 1e-5 + 2.5e-7 |ref| (the fp32 errors of
(x - m) - log S: the subtraction |d| 2^-24, exp a few ulp, the tree sum ~25 x 2^-24, log ~1 ulp), -inf exactly.

V: one element, both sides of a wave (63, 64, 65), both sides of a chunk of the first kernel (4097 = 4 x 1024 + 1), the real row.
Every family of rows runs at every top_n; the token a row asks for rotates through the maximum, the minimum, a -inf element (where
the row has one) and the median with the row and the top_n, so that a batch of one meets them all."""
import numpy as np
import pytest

from logprob_ref import CHUNK, TOP_MAX, check_values, logprob_all, top_order
from zig_gpt2_amd import _lib

pytestmark = pytest.mark.gpu
ERR_SHAPE, ERR_ARG = -2, -6
VOCABS = [1, 63, 64, 65, 4097, 50257]
TOP_NS = [0, 1, 5, 20]


def call(zg, x, toks, top_n):
    x = np.ascontiguousarray(x, np.float32)
    B, V = x.shape
    toks = np.ascontiguousarray(toks, np.uint64)
    lp = np.full(B, 123.0, np.float32)
    ids = np.full((B, top_n), 2 ** 40, np.uint64)
    top = np.full((B, top_n), 123.0, np.float32)
    rc = zg.zg_debug_logprob_rows(_lib.ptr(x), B, V, _lib.ptr(toks), top_n, _lib.ptr(lp), _lib.ptr(ids) if top_n else None,
                                  _lib.ptr(top) if top_n else None)
    return rc, lp, ids, top


def base(rng, B, V):
    return (3.0 * rng.standard_normal((B, V))).astype(np.float32)


def fam_max_duplicated(rng, B, V, top_n):
    """the maximum at 0, 63, 64, V - 1 and on both sides of every chunk boundary: the lowest indices win, across chunks"""
    x = base(rng, B, V)
    pos = {0, 63, 64, V - 1} | {k * CHUNK - 1 for k in range(1, V // CHUNK + 1)} | {k * CHUNK for k in range(1, V // CHUNK + 1)}
    pos = np.array(sorted(p for p in pos if 0 <= p < V))
    for b in range(B):
        x[b, pos[b % 2:]] = x[b].max() + np.float32(1.0)  # (odd rows: index 0 is not among them)
    return x


def fam_run_at_the_cut(rng, B, V, top_n):
    """top_n + 3 equal values around rank top_n: the index decides the last places"""
    x = base(rng, B, V)
    for b in range(B):
        order = np.argsort(-x[b], kind="stable")
        r0 = max(top_n - 2, 0)
        run = order[r0: r0 + top_n + 3]
        if run.size:
            x[b, run] = x[b, order[r0]]
    return x


def fam_signed_zeros(rng, B, V, top_n):
    """-0.0 and +0.0 above everything else: a tie, so the index orders them"""
    x = -np.abs(base(rng, B, V)) - np.float32(0.1)
    for b in range(B):
        p = np.sort(rng.choice(V, size=min(4, V), replace=False))
        x[b, p] = np.array([-0.0, 0.0, 0.0, -0.0], np.float32)[: p.size]
    return x


def fam_minus_infinity(rng, B, V, top_n):
    """several -inf; in the short rows only three values are finite, so the top 20 reach into the -inf, in index order; in the long
    ones a whole chunk of the first kernel is -inf"""
    x = base(rng, B, V)
    if V == 1:
        return x  # (a row of nothing but -inf has no distribution)
    for b in range(B):
        n_inf = V - 3 if 3 < V <= 65 else max(1, V // 8)
        n_inf = min(n_inf, V - 1)
        x[b, rng.choice(V, size=n_inf, replace=False)] = -np.inf
        if V > 2 * CHUNK:
            x[b, CHUNK: 2 * CHUNK] = -np.inf
        if not np.isfinite(x[b]).any():
            x[b, V // 2] = 0.5
    return x


def fam_all_equal(rng, B, V, top_n):
    return np.full((B, V), 1.5, np.float32)


def fam_one_far_above(rng, B, V, top_n):
    x = base(rng, B, V)
    for b in range(B):
        x[b, rng.integers(V)] = x[b].max() + np.float32(80.0)
    return x


def fam_scaled_by_ten(rng, B, V, top_n):
    return base(rng, B, V) * np.float32(10.0)


FAMILIES = [fam_max_duplicated, fam_run_at_the_cut, fam_signed_zeros, fam_minus_infinity, fam_all_equal, fam_one_far_above, fam_scaled_by_ten]


def pick_tokens(x, turn):
    toks = np.zeros(x.shape[0], np.uint64)
    for b, row in enumerate(x):
        kind = (b + turn) % 4
        ninf = np.flatnonzero(np.isneginf(row))
        if kind == 0:
            toks[b] = np.argmax(row)
        elif kind == 1 or (kind == 2 and ninf.size == 0):
            toks[b] = np.argmin(row)
        elif kind == 2:
            toks[b] = ninf[ninf.size // 2]
        else:
            toks[b] = np.argsort(row, kind="stable")[row.size // 2]
    return toks


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("V", VOCABS)
def test_rows_against_float64(zg, V, B):
    rng = np.random.default_rng(1000 * B + V)
    worst = 0.0
    for fi, fam in enumerate(FAMILIES):
        cache = {}
        for ti, top_n in enumerate(min(t, V) for t in TOP_NS):
            x = fam(np.random.default_rng([fi, B, V, top_n if fam is fam_run_at_the_cut else 0]), B, V, top_n)
            key = x.tobytes()
            if key not in cache:  # (the float64 reference of a set of rows, once)
                cache[key] = ([logprob_all(r) for r in x], [top_order(r, min(TOP_MAX, V)) for r in x])
            ref_lp, ref_ids = cache[key]
            toks = pick_tokens(x, ti + fi)
            rc, lp, ids, top = call(zg, x, toks, top_n)
            assert rc == 0, (fam.__name__, top_n, zg.zg_last_error())
            for b in range(B):
                tag = (fam.__name__, V, B, top_n, b)
                t = int(toks[b])
                assert np.array_equal(ids[b].astype(np.int64), ref_ids[b][:top_n]), (tag, ids[b], ref_ids[b][:top_n])
                worst = max(worst, check_values(lp[b: b + 1], ref_lp[b][t: t + 1]))
                worst = max(worst, check_values(top[b], ref_lp[b][ref_ids[b][:top_n]]))
                assert len(set(ids[b].tolist())) == top_n, tag
                assert np.all(top[b][1:] <= top[b][:-1]), (tag, top[b])
                for j in np.flatnonzero(ids[b] == t):
                    assert top[b, j].view(np.uint32) == lp[b].view(np.uint32), (tag, top[b, j], lp[b])
            if top_n == min(TOP_MAX, V):  # the same inputs, the same bits
                for _ in range(2):
                    rc2, lp2, ids2, top2 = call(zg, x, toks, top_n)
                    assert rc2 == 0 and np.array_equal(ids2, ids)
                    assert np.array_equal(lp2.view(np.uint32), lp.view(np.uint32)) and np.array_equal(top2.view(np.uint32), top.view(np.uint32))
    print(f"logprob rows V={V} B={B}: largest |got - ref64| / bound = {worst:.3f}")
    del rng


@pytest.mark.parametrize("V", [65, 4097, 50257])
def test_a_nan_in_every_row_faults_nothing(zg, V):
    rng = np.random.default_rng(V)
    x = base(rng, 3, V)
    for b in range(3):
        x[b, [0, V // 2, V - 1][b]] = np.nan
    toks = np.array([0, V // 2, 1], np.uint64)  # (one of them the NaN itself)
    for top_n in (0, 5, 20):
        rc, lp, ids, top = call(zg, x, toks, top_n)
        assert rc == 0, zg.zg_last_error()
        assert np.all(ids < V)


def test_argument_errors(zg):
    x = base(np.random.default_rng(1), 2, 100)
    ok = np.array([3, 99], np.uint64)
    assert call(zg, x, ok, 20)[0] == 0
    assert call(zg, x, ok, 21)[0] == ERR_ARG
    assert call(zg, x[:, :7], np.array([3, 6], np.uint64), 8)[0] == ERR_ARG    # top_n > V
    assert call(zg, x[:, :7], np.array([3, 6], np.uint64), 7)[0] == 0
    assert call(zg, x, np.array([3, 100], np.uint64), 5)[0] == ERR_SHAPE       # token >= V
    assert call(zg, x, ok, 5)[0] == 0
