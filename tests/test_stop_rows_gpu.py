"""zg_debug_stop_rows — the stop kernel alone, launched once per column over the caller's token rows — against tests/stop_ref.py:
finish column and reason of every row, and the done column the kernel stores to pinned host memory (include/zgpt2.h)."""
import ctypes as C

import numpy as np
import pytest

import stop_ref
from zig_gpt2_amd import _lib

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_SHAPE = -6, -2


def run(zg, tokens, first_cols, ids, seqs, n_cols=None, expect=0):
    tokens = np.ascontiguousarray(tokens, np.uint64)
    B, stride = tokens.shape
    first = np.ascontiguousarray(first_cols, np.uint64)
    conds, keep = _lib.stop_conditions(ids, seqs)
    cols = np.zeros(B, np.uint64)
    reasons = np.zeros(B, np.int32)
    done = C.c_size_t(12345)
    rc = zg.zg_debug_stop_rows(_lib.ptr(tokens), B, stride, _lib.ptr(first), stride if n_cols is None else n_cols, C.addressof(conds), _lib.ptr(cols),
                               _lib.ptr(reasons), C.byref(done))
    del keep
    assert rc == expect, (rc, zg.zg_last_error())
    return [None if int(c) == _lib.STOP_NONE else int(c) for c in cols], [int(r) for r in reasons], done.value


def check(zg, tokens, first_cols, ids, seqs, what):
    got_cols, got_reasons, got_done = run(zg, tokens, first_cols, ids, seqs)
    cols, reasons = stop_ref.finish(tokens, first_cols, ids, seqs)
    assert got_cols == cols and got_reasons == reasons, (what, got_cols, cols, got_reasons, reasons)
    assert got_done == stop_ref.done_col(cols), (what, got_done, cols)
    return cols


@pytest.mark.parametrize("case", stop_ref.CASES, ids=[c[0] for c in stop_ref.CASES])
def test_hand_written_cases(zg, case):
    _, tokens, first_cols, ids, seqs, want_cols, want_reasons = case
    got_cols, got_reasons, got_done = run(zg, tokens, first_cols, ids, seqs)
    assert got_cols == want_cols and got_reasons == want_reasons
    assert got_done == stop_ref.done_col(want_cols)


@pytest.mark.parametrize("batch", [1, 3, 8])
def test_seeded_random_matrices(zg, batch):
    """Vocabulary 5 over 40 columns with ragged first columns and random conditions: matches are frequent at every offset, ties
    between conditions at one column too."""
    rng = np.random.default_rng(7000 + batch)
    n_done = n_none = 0
    for trial in range(70):
        tokens = rng.integers(0, 5, (batch, 40))
        first_cols = rng.integers(0, 12, batch)
        if trial % 7 == 0:
            first_cols[rng.integers(0, batch)] = 40 + trial  # a row that never picks anything
        ids = list(rng.integers(0, 5, rng.integers(0, 3)))
        seqs = [list(rng.integers(0, 5, rng.integers(1, 6))) for _ in range(rng.integers(0, 5))]
        if trial % 5 == 0:  # rare matches: long sequences only
            ids, seqs = [], [list(rng.integers(0, 5, rng.integers(4, 9))) for _ in range(3)]
        cols = check(zg, tokens, first_cols, ids, seqs, (batch, trial))
        n_done += all(c is not None for c in cols)
        n_none += any(c is None for c in cols)
    assert n_done >= 10 and n_none >= 10, (n_done, n_none)


def test_the_limits_exactly(zg):
    """16 stop tokens and 8 sequences of 16 tokens: the last sequence alone occurs, then the last stop token alone."""
    rng = np.random.default_rng(71)
    tokens = rng.integers(100, 200, (2, 64))
    ids = list(range(1000, 1016))
    seqs = [list(range(2000 + 20 * k, 2016 + 20 * k)) for k in range(8)]
    tokens[0, 30:46] = seqs[7]
    tokens[0, 50] = ids[15]
    tokens[1, 20] = ids[15]
    tokens[1, 21:36] = seqs[0][1:]  # all but the first token
    first_cols = [3, 0]
    cols = check(zg, tokens, first_cols, ids, seqs, "limits")
    assert cols == [45, 20]
    assert run(zg, tokens, first_cols, ids, seqs)[1] == [16 + 7, 15]
    first_cols = [31, 21]  # the sequence now starts in the prompt: the stop token behind it is what finishes row 0
    assert check(zg, tokens, first_cols, ids, seqs, "limits behind a longer prompt") == [50, None]


def test_one_row_that_never_matches_gives_no_done_col(zg):
    tokens = [[1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1], [1, 1, 1, 1, 1, 1]]
    got_cols, got_reasons, got_done = run(zg, tokens, [0, 0, 0], [3], [[5, 4]])
    assert got_cols == [2, 2, None] and got_reasons == [0, 1, -1] and got_done == 0
    # ... and over fewer columns nothing has happened yet
    assert run(zg, tokens, [0, 0, 0], [3], [[5, 4]], n_cols=2) == ([None, None, None], [-1, -1, -1], 0)
    assert run(zg, tokens[:2], [0, 0], [3], [[5, 4]])[2] == 3


def test_refusals(zg):
    tokens, first = [[1, 2, 3, 4]], [0]
    assert run(zg, tokens, first, list(range(17)), [], expect=ERR_ARG)
    assert run(zg, tokens, first, [], [[1]] * 9, expect=ERR_ARG)
    assert run(zg, tokens, first, [], [list(range(17))], expect=ERR_ARG)
    assert run(zg, tokens, first, [1 << 40], [], expect=ERR_SHAPE)
    assert run(zg, tokens, first, [], [[1, 1 << 40]], expect=ERR_SHAPE)
    t = np.ascontiguousarray(tokens, np.uint64)
    f = np.ascontiguousarray(first, np.uint64)
    cols, reasons, done = np.zeros(1, np.uint64), np.zeros(1, np.int32), C.c_size_t()
    ids = np.ascontiguousarray([1, 2], np.uint64)
    lens = np.ascontiguousarray([0], np.uint64)

    def raw(conds, batch=1):
        return zg.zg_debug_stop_rows(_lib.ptr(t), batch, 4, _lib.ptr(f), 4, None if conds is None else C.addressof(conds), _lib.ptr(cols), _lib.ptr(reasons),
                                     C.byref(done))

    assert raw(None) == ERR_ARG
    assert raw(_lib.StopConditions(None, 2, None, 0, None, 0, 0)) == ERR_ARG                               # a NULL array with a count
    assert raw(_lib.StopConditions(None, 0, None, 4, _lib.ptr(lens), 1, 0)) == ERR_ARG
    assert raw(_lib.StopConditions(None, 0, _lib.ptr(ids), 2, _lib.ptr(lens), 1, 0)) == ERR_ARG            # a sequence of length 0
    lens[0] = 2
    assert raw(_lib.StopConditions(None, 0, _lib.ptr(ids), 1, _lib.ptr(lens), 1, 0)) == ERR_ARG            # ... longer than the stride
    assert raw(_lib.StopConditions(None, 0, _lib.ptr(ids), 2, _lib.ptr(lens), 1, 0)) == 0
    assert raw(_lib.StopConditions(_lib.ptr(ids), 2, None, 0, None, 0, 0), batch=9) == ERR_ARG
    assert raw(_lib.StopConditions(_lib.ptr(ids), 2, None, 0, None, 0, 0)) == 0 and int(cols[0]) == 0 and done.value == 1
