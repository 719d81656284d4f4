"""The penalty kernels alone (zg_debug_penalize_rows: the caller's rows and histories) against penalty_ref.py, bitwise: the counts
equal np.bincount, an index the history does not hold keeps its bits, a penalised one equals the float32 expression of
include/zgpt2.h evaluated by numpy in the same order (a NaN stays a NaN), and all penalties off return the input."""
import numpy as np
import pytest

from penalty_ref import penalize_row, penalize_rows, same_bits

pytestmark = pytest.mark.gpu
VOCABS = [1, 63, 64, 65, 4097, 50257]
BATCHES = [1, 3, 8]
KINDS = ["empty", "one", "copies", "distinct", "mix"]
# r above and below 1, presence and frequency of both signs; the last: everything off
PENALTIES = [(1.3, 0.5, 0.25), (0.7, -0.75, -0.125), (1.0, 0.0, 0.3), (2.5, 0.0, 0.0), (1.0, 0.0, 0.0)]
SPECIALS = np.array([0.0, -0.0, 1e30, -1e30, 3.0e38, -3.0e38, np.inf, -np.inf, 1e-30, -1e-30, 1e-40, -1e-40], np.float32)


def history(kind, V, rng):
    if kind == "empty":
        return np.zeros(0, np.uint64)
    if kind == "one":
        return rng.integers(0, V, 1).astype(np.uint64)
    if kind == "copies":  # 1024 copies of one token
        return np.full(1024, rng.integers(0, V), np.uint64)
    if kind == "distinct":  # 1024 distinct tokens (a smaller vocabulary: all of it, in a shuffled order, repeated to 1024)
        if V >= 1024:
            return rng.permutation(V)[:1024].astype(np.uint64)
        return np.resize(rng.permutation(V), 1024).astype(np.uint64)
    # heavy duplication: 700 draws from a pool of 12 tokens that holds 0 and V - 1
    pool = np.unique(np.r_[0, V - 1, rng.integers(0, V, 10)])
    return pool[rng.integers(0, pool.size, 700)].astype(np.uint64)


def rows(V, B, hists, rng):
    x = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
    for b in range(B):
        # every special value on an index of the history (where there is one) and on one outside it
        inside = np.unique(hists[b]).astype(np.int64)
        outside = np.setdiff1d(np.arange(V), inside)
        for pool in (inside, outside):
            if pool.size:
                at = pool[rng.integers(0, pool.size, SPECIALS.size)]
                x[b, at] = SPECIALS
        x[b, rng.integers(0, V)] = np.nan  # one NaN per row
    x[0, 0] = np.float32(0.0)
    x[-1, V - 1] = np.float32(-0.0)
    return x


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("V", VOCABS)
def test_counts_and_penalised_rows_are_bitwise_the_reference(zg, V, B):
    rng = np.random.default_rng(9100 + 10 * V + B)
    for rot in range(len(KINDS)):  # rows of a batch have different kinds (and lengths); every row position sees every kind
        hists = [history(KINDS[(rot + b) % len(KINDS)], V, rng) for b in range(B)]
        x = rows(V, B, hists, rng)
        for r, p, f in PENALTIES:
            what = f"V {V} B {B} rot {rot} r {r} presence {p} frequency {f}"
            rc, got, counts = penalize_rows(zg, x, hists, r, p, f)
            assert rc == 0, what
            for b in range(B):
                want, c = penalize_row(x[b], hists[b], r, p, f)
                assert np.array_equal(counts[b], c), (what, b, np.flatnonzero(counts[b] != c)[:5])
                untouched = c == 0
                assert np.array_equal(got[b].view(np.uint32)[untouched], x[b].view(np.uint32)[untouched]), (what, b, "an index outside the history changed")
                bad = np.flatnonzero(~(((got[b].view(np.uint32) == want.view(np.uint32))) | (np.isnan(got[b]) & np.isnan(want))))
                assert bad.size == 0, (what, b, bad[:5], x[b, bad[:5]], got[b, bad[:5]], want[bad[:5]], c[bad[:5]])
                assert same_bits(got[b], want)
            if (r, p, f) == (1.0, 0.0, 0.0):
                assert np.array_equal(got.view(np.uint32), x.view(np.uint32)), (what, "all off must return the input bit for bit")


def test_each_distinct_token_is_penalised_once(zg):
    """HF's gather-and-scatter: 1024 occurrences of a token divide its logit by r once, and only the frequency term sees the count."""
    V = 4097
    x = np.full((1, V), np.float32(2.0), np.float32)
    rc, got, counts = penalize_rows(zg, x, [np.full(1024, 77, np.uint64)], 2.0, 0.25, 0.001)
    assert rc == 0 and counts[0, 77] == 1024 and counts.sum() == 1024
    assert got[0, 77] == np.float32(1.0) - (np.float32(0.25) + np.float32(0.001) * np.float32(1024.0))
    assert np.array_equal(np.delete(got[0], 77), np.delete(x[0], 77))


def test_the_longest_history_and_one_beyond(zg):
    """8192 tokens (the cap of include/zgpt2.h: the table then takes 128 KB of LDS), distinct and duplicated; 8193 are refused."""
    V = 50257
    rng = np.random.default_rng(9300)
    hists = [rng.permutation(V)[:8192].astype(np.uint64), rng.integers(0, 300, 8192).astype(np.uint64), np.zeros(0, np.uint64)]
    x = (3.0 * rng.standard_normal((3, V))).astype(np.float32)
    rc, got, counts = penalize_rows(zg, x, hists, 1.2, 0.1, 0.01)
    assert rc == 0
    for b in range(3):
        want, c = penalize_row(x[b], hists[b], 1.2, 0.1, 0.01)
        assert np.array_equal(counts[b], c) and same_bits(got[b], want), b
    rc, _, _ = penalize_rows(zg, x[:1], [np.zeros(8193, np.uint64)], 1.2, 0.1, 0.01)
    assert rc == -5  # ZG_ERR_UNSUPPORTED


def test_repeated_calls_give_identical_bits(zg):
    rng = np.random.default_rng(9400)
    V, B = 4097, 3
    hists = [history("mix", V, rng) for _ in range(B)]
    x = rows(V, B, hists, rng)
    first = penalize_rows(zg, x, hists, 1.3, 0.5, 0.25)
    for _ in range(3):
        again = penalize_rows(zg, x, hists, 1.3, 0.5, 0.25)
        assert again[0] == 0 and np.array_equal(again[1].view(np.uint32), first[1].view(np.uint32)) and np.array_equal(again[2], first[2])
