"""zg_debug_pick_rows — the decode step's head kernel picking from the caller's argmax partials, in the form zg_gpt_argmax launches —
against tests/pick_ref.py, by exact integer equality.  The kernel reads a row with one wave, eight partials per lane and round
(partial p of a round sits in lane p % 64, register p // 64): the sizes cover one round, a partial round and three rounds, the batches
four and eight waves, and the tie patterns put the lower index into another lane of the same 16-lane row (distance 1), another
row (16), the same lane's next register (64) and another round (512)."""
import numpy as np
import pytest

import pick_ref
from zig_gpt2_amd import _lib

pytestmark = pytest.mark.gpu
ERR_ARG = -6
VOCAB = 50257
BATCHES = [1, 5, 8]
N_PARTS = [1, 2, 63, 64, 65, 393, 512, 513, 1100]
SHAPES = [(b, n) for b in BATCHES for n in N_PARTS]
NAN, INF = np.float32("nan"), np.float32("inf")


def pick(zg, val, idx, vocab=VOCAB, expect=0):
    val = np.ascontiguousarray(val, np.float32)
    idx = np.ascontiguousarray(idx, np.int32)
    assert val.shape == idx.shape and val.ndim == 2
    out = np.full(val.shape[0], 12345, np.uint64)
    rc = zg.zg_debug_pick_rows(_lib.ptr(val), _lib.ptr(idx), val.shape[0], val.shape[1], vocab, _lib.ptr(out))
    assert rc == expect, (rc, zg.zg_last_error())
    return [int(t) for t in out]


def check(zg, val, idx, vocab=VOCAB):
    got = pick(zg, val, idx, vocab)
    assert got == pick_ref.pick_rows(val, idx, vocab), (got, np.asarray(val).shape)
    return got


def rng_for(batch, n_part, salt):
    return np.random.default_rng([batch, n_part, salt])


def distinct(rng, batch, n_part):
    """distinct finite values in random order, distinct indices below the vocabulary in random order"""
    val = np.stack([rng.permutation(n_part) for _ in range(batch)]).astype(np.float32) * np.float32(0.25) - np.float32(100.0)
    idx = np.stack([rng.choice(VOCAB, n_part, replace=False) for _ in range(batch)]).astype(np.int32)
    return val, idx


@pytest.mark.parametrize("batch,n_part", SHAPES)
def test_distinct_values(zg, batch, n_part):
    val, idx = distinct(rng_for(batch, n_part, 1), batch, n_part)
    got = check(zg, val, idx)
    assert got == [int(idx[b, np.argmax(val[b])]) for b in range(batch)]


@pytest.mark.parametrize("batch,n_part", SHAPES)
def test_all_equal_the_lowest_index_wins_wherever_it_sits(zg, batch, n_part):
    val, idx = distinct(rng_for(batch, n_part, 2), batch, n_part)
    val[:] = np.float32(1.5)
    got = check(zg, val, idx)
    assert got == [int(idx[b].min()) for b in range(batch)]


@pytest.mark.parametrize("batch,n_part,dist", [(b, n, d) for b, n in SHAPES for d in (1, 16, 64, 512) if d < n])  # (every pair a row can hold)
def test_two_equal_maxima_the_lower_index_later(zg, batch, n_part, dist):
    rng = rng_for(batch, n_part, 100 + dist)
    val, idx = distinct(rng, batch, n_part)
    want = []
    for b in range(batch):
        p0 = int(rng.integers(0, n_part - dist))
        lo, hi = sorted((int(idx[b, p0]), int(idx[b, p0 + dist])))
        val[b, p0] = val[b, p0 + dist] = np.float32(1000.0)
        idx[b, p0], idx[b, p0 + dist] = hi, lo
        want.append(lo)
    assert check(zg, val, idx) == want


@pytest.mark.parametrize("batch,n_part", SHAPES)
def test_positive_and_negative_zero_are_one_value(zg, batch, n_part):
    rng = rng_for(batch, n_part, 4)
    val, idx = distinct(rng, batch, n_part)
    val -= np.float32(1000.0)  # everything else below zero
    want = []
    for b in range(batch):
        pos = np.sort(rng.choice(n_part, min(2, n_part), replace=False))
        zeros = [np.float32(0.0), np.float32(-0.0)] if b % 2 else [np.float32(-0.0), np.float32(0.0)]
        for p, z in zip(pos, zeros):
            val[b, p] = z
        if len(pos) == 2:  # the lower index at the later position
            a, c = sorted((int(idx[b, pos[0]]), int(idx[b, pos[1]])))
            idx[b, pos[0]], idx[b, pos[1]] = c, a
        want.append(int(min(idx[b, p] for p in pos)))
    assert check(zg, val, idx) == want


@pytest.mark.parametrize("batch,n_part", SHAPES)
def test_nan_never_wins(zg, batch, n_part):
    rng = rng_for(batch, n_part, 5)
    val, idx = distinct(rng, batch, n_part)
    mask = rng.random((batch, n_part)) < 0.4
    for b in range(batch):
        mask[b, np.argmin(val[b])] = False       # one value of every row stays
        mask[b, np.argmax(val[b])] = n_part > 1  # the would-be winner is among the NaNs
    mixed = np.where(mask, NAN, val).astype(np.float32)
    got = check(zg, mixed, idx)
    assert got == [int(idx[b, np.nanargmax(mixed[b])]) for b in range(batch)]
    assert check(zg, np.full((batch, n_part), NAN, np.float32), idx) == [0] * batch


@pytest.mark.parametrize("batch,n_part", SHAPES)
def test_all_minus_infinity_leaves_the_start_value_standing(zg, batch, n_part):
    _, idx = distinct(rng_for(batch, n_part, 6), batch, n_part)
    assert check(zg, np.full((batch, n_part), -INF, np.float32), idx) == [0] * batch


@pytest.mark.parametrize("batch,n_part", SHAPES)
def test_a_winning_index_outside_the_vocabulary_gives_zero(zg, batch, n_part):
    rng = rng_for(batch, n_part, 7)
    val, idx = distinct(rng, batch, n_part)
    idx[idx == 0] = 1  # (so that 0 can only be the clamp's)
    for b in range(batch):
        w = np.argmax(val[b])
        idx[b, w] = [VOCAB, -1, VOCAB + 7, -(2**31), 2**31 - 1][b % 5]
    assert check(zg, val, idx) == [0] * batch
    # ... and one below the bound is followed
    for b in range(batch):
        idx[b, np.argmax(val[b])] = VOCAB - 1
    assert check(zg, val, idx) == [VOCAB - 1] * batch
    assert check(zg, val, idx, vocab=VOCAB - 1) == [0] * batch


def test_refusals(zg):
    val, idx = np.zeros((9, 4), np.float32), np.zeros((9, 4), np.int32)
    out = np.zeros(9, np.uint64)
    assert zg.zg_debug_pick_rows(_lib.ptr(val), _lib.ptr(idx), 9, 4, VOCAB, _lib.ptr(out)) == ERR_ARG
    assert zg.zg_debug_pick_rows(_lib.ptr(val), _lib.ptr(idx), 0, 4, VOCAB, _lib.ptr(out)) == ERR_ARG
    assert zg.zg_debug_pick_rows(_lib.ptr(val), _lib.ptr(idx), 1, 0, VOCAB, _lib.ptr(out)) == ERR_ARG
    assert zg.zg_debug_pick_rows(_lib.ptr(val), _lib.ptr(idx), 1, 4097, VOCAB, _lib.ptr(out)) == ERR_ARG
    assert zg.zg_debug_pick_rows(_lib.ptr(val), _lib.ptr(idx), 1, 4, 0, _lib.ptr(out)) == ERR_ARG
    assert zg.zg_debug_pick_rows(_lib.ptr(val), _lib.ptr(idx), 1, 4, 2**31, _lib.ptr(out)) == ERR_ARG
    assert zg.zg_debug_pick_rows(None, _lib.ptr(idx), 1, 4, VOCAB, _lib.ptr(out)) == ERR_ARG
    assert zg.zg_debug_pick_rows(_lib.ptr(val), None, 1, 4, VOCAB, _lib.ptr(out)) == ERR_ARG
    assert zg.zg_debug_pick_rows(_lib.ptr(val), _lib.ptr(idx), 1, 4, VOCAB, None) == ERR_ARG
