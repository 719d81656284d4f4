"""zg_debug_score_rows: the two statistics kernels of zg_gpt_score (csrc/sample_score.h) alone on hand-made rows against the float64
reference of tests/logprob_ref.py, row by row — ids exactly in the reference's order, values within logprob_ref.bound (check_values),
-inf exactly.  The kernels differ from the device loop's in where the row maximum comes from (the chunks themselves) and in reading
rows of a wider block: every case runs with row_stride = vocab and with row_stride = 64 ceil(vocab / 64) + 64 whose pad columns
[vocab, row_stride) hold +3e38 — one pad column read shows as inf, or as an id >= vocab.

vocab: one element, a part of one chunk, exactly one chunk of 1024, one element into the second, the real row.  rows: one, a few,
more than a block of 128.  The families of rows (the checklist of test_logprob_rows_gpu.py) rotate over the rows — 129 rows hold
every family at every top_n — and for fewer rows than families also over the (row_stride, top_n) combinations, so that a single
row meets every family."""
import numpy as np
import pytest

from logprob_ref import CHUNK, TOP_MAX, check_values, logprob_all, top_order
from zig_gpt2_amd import _lib

pytestmark = pytest.mark.gpu
ERR_SHAPE, ERR_ARG = -2, -6
ROWS = [1, 3, 129]
VOCABS = [1, 257, 1024, 1025, 50257]
PAD = np.float32(3e38)


def call(zg, x, V, targets, top_n):
    """x [rows, row_stride] float32, the first V columns of a row are the row"""
    x = np.ascontiguousarray(x, np.float32)
    rows, stride = x.shape
    targets = np.ascontiguousarray(targets, np.uint64)
    lp = np.full(rows, 123.0, np.float32)
    ids = np.full((rows, top_n), 2 ** 40, np.uint64)
    top = np.full((rows, top_n), 123.0, np.float32)
    rc = zg.zg_debug_score_rows(_lib.ptr(x), rows, V, stride, _lib.ptr(targets), top_n, _lib.ptr(lp), _lib.ptr(ids) if top_n else None,
                                _lib.ptr(top) if top_n else None)
    return rc, lp, ids, top


def padded(x, stride):
    out = np.full((x.shape[0], stride), PAD, np.float32)
    out[:, : x.shape[1]] = x
    return out


def fam_normal(rng, V):
    return (2.0 * rng.standard_normal(V)).astype(np.float32)   # N(0, 4)


def fam_all_equal(rng, V):
    return np.full(V, 1.5, np.float32)                         # ties resolve by index, across chunks


def fam_signed_zeros(rng, V):
    x = -np.abs(fam_normal(rng, V)) - np.float32(0.1)
    p = np.sort(rng.choice(V, size=min(4, V), replace=False))
    x[p] = np.array([-0.0, 0.0, 0.0, -0.0], np.float32)[: p.size]
    return x


def fam_minus_infinity(rng, V):
    x = fam_normal(rng, V)
    if V == 1:
        return x  # (a row of nothing but -inf has no distribution)
    x[rng.choice(V, size=max(1, V // 8), replace=False)] = -np.inf
    if V > 2 * CHUNK:
        x[CHUNK: 2 * CHUNK] = -np.inf  # a whole chunk of the first kernel: its maximum is the floor, its sum 0
    if not np.isfinite(x).any():
        x[V // 2] = 0.5
    return x


def fam_max_last(rng, V):
    x = fam_normal(rng, V)
    x[V - 1] = x.max() + np.float32(1.0)                       # the maximum in the last chunk, in the last column
    return x


def fam_max_last_chunk(rng, V):
    x = fam_normal(rng, V)
    first = (V - 1) // CHUNK * CHUNK
    x[first] = x.max() + np.float32(60.0)                      # ... at the head of the last chunk, far above: the other chunks' sums shrink to ~0
    return x


FAMILIES = [fam_normal, fam_all_equal, fam_signed_zeros, fam_minus_infinity, fam_max_last, fam_max_last_chunk]


def make_rows(rows, V, turn):
    x = np.empty((rows, V), np.float32)
    for r in range(rows):
        x[r] = FAMILIES[(r + turn) % len(FAMILIES)](np.random.default_rng([rows, V, r, turn]), V)
    return x


def pick_targets(x, turn):
    """the last column, the maximum, the minimum, a -inf element where the row has one, the median: in turn"""
    t = np.zeros(x.shape[0], np.uint64)
    for r, row in enumerate(x):
        kind = (r + turn) % 5
        ninf = np.flatnonzero(np.isneginf(row))
        if kind == 0:
            t[r] = row.size - 1
        elif kind == 1:
            t[r] = np.argmax(row)
        elif kind == 2 or (kind == 3 and ninf.size == 0):
            t[r] = np.argmin(row)
        elif kind == 3:
            t[r] = ninf[ninf.size // 2]
        else:
            t[r] = np.argsort(row, kind="stable")[row.size // 2]
    return t


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("V", VOCABS)
def test_rows_against_float64(zg, V, rows):
    strides = [V, (V + 63) // 64 * 64 + 64]
    top_ns = sorted({0, min(1, V), min(TOP_MAX, V)})  # 0, 1, 20 and min(20, vocab)
    cache, worst, turn = {}, 0.0, 0
    for stride in strides:
        for top_n in top_ns:
            x = make_rows(rows, V, turn if rows < len(FAMILIES) else 0)
            key = x.tobytes()
            if key not in cache:  # (the float64 reference of a set of rows, once)
                cache[key] = ([logprob_all(r) for r in x], [top_order(r, min(TOP_MAX, V)) for r in x])
            ref_lp, ref_ids = cache[key]
            targets = pick_targets(x, turn)
            xs = padded(x, stride)
            rc, lp, ids, top = call(zg, xs, V, targets, top_n)
            assert rc == 0, (stride, top_n, zg.zg_last_error())
            for r in range(rows):
                tag = (FAMILIES[(r + (turn if rows < len(FAMILIES) else 0)) % len(FAMILIES)].__name__, V, rows, stride, top_n, r)
                t = int(targets[r])
                assert np.array_equal(ids[r].astype(np.int64), ref_ids[r][:top_n]), (tag, ids[r], ref_ids[r][:top_n])
                worst = max(worst, check_values(lp[r: r + 1], ref_lp[r][t: t + 1]))
                worst = max(worst, check_values(top[r], ref_lp[r][ref_ids[r][:top_n]]))
                for j in np.flatnonzero(ids[r] == t):  # where an id is the target: bit for bit its log-probability
                    assert top[r, j].view(np.uint32) == lp[r].view(np.uint32), (tag, top[r, j], lp[r])
            if top_n == min(TOP_MAX, V):  # the same inputs, the same bits
                rc2, lp2, ids2, top2 = call(zg, xs, V, targets, top_n)
                assert rc2 == 0 and np.array_equal(ids2, ids)
                assert np.array_equal(lp2.view(np.uint32), lp.view(np.uint32)) and np.array_equal(top2.view(np.uint32), top.view(np.uint32))
            turn += 1
    print(f"score rows V={V} rows={rows}: largest |got - ref64| / bound = {worst:.3f}")


@pytest.mark.parametrize("V", [257, 50257])
def test_a_nan_in_every_row_faults_nothing(zg, V):
    x = np.stack([fam_normal(np.random.default_rng([V, b]), V) for b in range(3)])
    for b in range(3):
        x[b, [0, V // 2, V - 1][b]] = np.nan
    targets = np.array([0, V // 2, 1], np.uint64)  # (one of them the NaN itself)
    for stride in (V, (V + 63) // 64 * 64 + 64):
        for top_n in (0, 5, 20):
            rc, lp, ids, top = call(zg, padded(x, stride), V, targets, top_n)
            assert rc == 0, zg.zg_last_error()
            assert np.all(ids < V)


def test_argument_errors(zg):
    x = np.stack([fam_normal(np.random.default_rng(b), 100) for b in range(2)])
    ok = np.array([3, 99], np.uint64)
    assert call(zg, x, 100, ok, 20)[0] == 0
    assert call(zg, x, 100, ok, 21)[0] == ERR_ARG
    assert call(zg, x, 7, np.array([3, 6], np.uint64), 8)[0] == ERR_ARG        # top_n > vocab (rows 100 apart)
    assert call(zg, x, 7, np.array([3, 6], np.uint64), 7)[0] == 0
    assert call(zg, x, 100, np.array([3, 100], np.uint64), 5)[0] == ERR_SHAPE  # target >= vocab
    assert call(zg, x, 101, ok, 5)[0] == ERR_ARG                               # row_stride < vocab
    many = np.zeros((4097, 4), np.float32)
    assert call(zg, many, 4, np.zeros(4097, np.uint64), 1)[0] == ERR_ARG       # rows > 4096
    assert call(zg, many[:4096], 4, np.zeros(4096, np.uint64), 1)[0] == 0
    assert call(zg, x, 100, ok, 5)[0] == 0
