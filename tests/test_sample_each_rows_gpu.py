"""Per-row sampling parameters, the kernels alone (zg_debug_sample_rows_each / zg_debug_penalize_rows_each).

The oracle is the library's own uniform call: sequences never interact, so row b of a per-row call must equal — tokens,
probabilities and thresholds, BIT FOR BIT — row b of zg_debug_edit_rows given that row's parameters for every row.  The table holds
all five sampler forms plus top-k + min-p and top-p + min-p at temperatures 0.3 / 0.8 / 1.7, so that whatever a row needs, some
neighbour makes the chain longer than that: a plain row inside six selection launches, a top-k-only row in front of a neighbour's
nucleus descent, a min-p-alone row behind both.  Vocabularies: 257 (one workgroup per row in the level kernels, 5 segments) and 5003
(several workgroups per row, 20 row-maximum partials).  The penalty stage is held to penalty_ref.penalize_row, bitwise."""
import ctypes as C

import numpy as np
import pytest

from edit_ref import edit_rows
from penalty_ref import pack, penalize_row, same_bits
from zig_gpt2_amd import _lib

pytestmark = pytest.mark.gpu
ARG = -6
VOCABS = [257, 5003]
B = 8
# temp, top_k, top_p, min_p: plain, top-k, top-p, both, min-p alone, top-k + min-p, top-p + min-p, plain at another temperature
TABLE = [(0.8, 0, 1.0, 0.0), (0.3, 5, 1.0, 0.0), (1.7, 0, 0.6, 0.0), (0.8, 12, 0.7, 0.0), (0.3, 0, 1.0, 0.2), (1.7, 9, 1.0, 0.1),
         (0.8, 0, 0.8, 0.05), (1.7, 0, 1.0, 0.0)]
PERMS = [list(range(B)), [3, 6, 0, 5, 7, 1, 4, 2]]  # row b takes TABLE[perm[b]]: every row changes its form between the two
EDITS = dict(bias={0: 2.5, 3: -4.0, 100: 3.0, 256: 1.25}, banned=[7, 41, 200, 7])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def logits_for(V):
    """Eight rows, each kind twice: random N(0, 4^2); quantised to 8 distinct values (ties at every threshold); a block of -inf, as
    an allow-list leaves it; all equal."""
    rng = np.random.default_rng(1000 + V)
    x = np.empty((B, V), np.float32)
    for b in range(B):
        r = (rng.standard_normal(V) * 4).astype(np.float32)
        kind = b % 4
        if kind == 1:
            r = (np.round(r / 4).clip(-4, 3) * 1.5).astype(np.float32)
        elif kind == 2:
            r[V // 5: V // 5 + V // 2] = -np.inf
        elif kind == 3:
            r[:] = np.float32(-2.75 if b < 4 else 0.0)
        x[b] = r
    return x


def as_rows(params):
    return [dict(temp=t, top_k=k, top_p=p, min_p=m) for t, k, p, m in params]


def each_rows(lib, x, params, u, edits=None, n_rows=None):
    """zg_debug_sample_rows_each: (rc, edited rows, tokens, probs, thresholds)."""
    x = np.ascontiguousarray(x, np.float32)
    nb, V = x.shape
    table = _lib.row_sampling(as_rows(params))
    u = np.ascontiguousarray(u, np.float32)
    tok = np.zeros(nb, np.uint64)
    edited = np.full((nb, V), np.float32(123.0), np.float32)
    probs = np.empty((nb, V), np.float32)
    thr = np.empty(nb, np.float32)
    e, keep = _lib.logit_edits(edits.get("bias"), None, edits.get("banned"), edits.get("min_p", 0.0)) if edits is not None else (None, ())
    rc = lib.zg_debug_sample_rows_each(_lib.ptr(x), nb, V, C.addressof(table), len(params) if n_rows is None else n_rows,
                                       None if e is None else C.addressof(e), _lib.ptr(u), _lib.ptr(edited), _lib.ptr(tok), _lib.ptr(probs), _lib.ptr(thr))
    del keep
    return rc, edited, tok, probs, thr


class Case:
    """The logits and uniforms of one vocabulary, and the uniform call's answer for every entry of TABLE (computed once)."""

    def __init__(self, lib, V):
        self.V, self.x = V, logits_for(V)
        self.u = np.random.default_rng(77 + V).random(B).astype(np.float32)
        self.uniform, self.uniform_edits = {}, {}
        for p in TABLE:
            for store, kw in ((self.uniform, {}), (self.uniform_edits, EDITS)):
                rc, ed, tok, probs, thr = edit_rows(lib, self.x, p[0], p[1], p[2], self.u, min_p=p[3], **kw)
                assert rc == 0, lib.zg_last_error()
                for a in (ed, tok, probs, thr):
                    a.setflags(write=False)
                store[p] = (ed, tok, probs, thr)


_cases = {}


@pytest.fixture(params=VOCABS)
def case(zg, request):
    V = request.param
    if V not in _cases:
        _cases[V] = Case(zg, V)
    return _cases[V]


def assert_rows_equal_uniform(got, want_by_param, params, what):
    _, ed, tok, probs, thr = got
    for b, p in enumerate(params):
        w_ed, w_tok, w_probs, w_thr = want_by_param[p]
        assert int(tok[b]) == int(w_tok[b]), (what, b, p, int(tok[b]), int(w_tok[b]))
        assert bits(thr[b:b + 1])[0] == bits(w_thr[b:b + 1])[0], (what, b, p, thr[b], w_thr[b])
        diff = np.flatnonzero(bits(probs[b]) != bits(w_probs[b]))
        assert diff.size == 0, (what, b, p, diff[:5], probs[b][diff[:5]], w_probs[b][diff[:5]])
        assert np.array_equal(bits(ed[b]), bits(w_ed[b])), (what, b, p)


@pytest.mark.parametrize("perm", [0, 1])
def test_every_row_equals_the_uniform_call_with_its_parameters(zg, case, perm):
    params = [TABLE[i] for i in PERMS[perm]]
    got = each_rows(zg, case.x, params, case.u)
    assert got[0] == 0, zg.zg_last_error()
    assert_rows_equal_uniform(got, case.uniform, params, f"V {case.V} perm {perm}")
    again = each_rows(zg, case.x, params, case.u)  # the same call twice: the same bits
    assert again[0] == 0 and np.array_equal(got[2], again[2]) and np.array_equal(bits(got[3]), bits(again[3])) and np.array_equal(bits(got[4]), bits(again[4]))
    # teeth: at least half the rows differ, in token or threshold, from what rows[0]'s parameters give them
    _, tok0, _, thr0 = case.uniform[params[0]]
    differ = sum(int(got[2][b]) != int(tok0[b]) or bits(got[4][b:b + 1])[0] != bits(thr0[b:b + 1])[0] for b in range(B))
    assert differ >= B // 2, differ


def test_with_edits_every_row_equals_the_uniform_call(zg, case):
    for perm in PERMS:
        params = [TABLE[i] for i in perm]
        got = each_rows(zg, case.x, params, case.u, edits=EDITS)
        assert got[0] == 0, zg.zg_last_error()
        assert_rows_equal_uniform(got, case.uniform_edits, params, f"V {case.V} edits")
    assert not np.array_equal(bits(case.uniform_edits[TABLE[3]][2]), bits(case.uniform[TABLE[3]][2])), "the edits changed nothing"


def test_a_row_keeps_its_result_wherever_it_sits(zg, case):
    """Logits, uniforms and parameters moved together to other rows: the results move with them."""
    base = each_rows(zg, case.x, TABLE, case.u)
    move = PERMS[1]
    got = each_rows(zg, case.x[move], [TABLE[i] for i in move], case.u[move])
    assert base[0] == 0 and got[0] == 0
    assert np.array_equal(got[2], base[2][move]) and np.array_equal(bits(got[3]), bits(base[3][move])) and np.array_equal(bits(got[4]), bits(base[4][move]))


@pytest.mark.parametrize("entry", range(len(TABLE)))
def test_a_table_of_equal_entries_is_the_uniform_call(zg, case, entry):
    p = TABLE[entry]
    got = each_rows(zg, case.x, [p] * B, case.u)
    assert got[0] == 0, zg.zg_last_error()
    ed, tok, probs, thr = case.uniform[p]
    assert np.array_equal(got[2], tok) and np.array_equal(bits(got[3]), bits(probs)) and np.array_equal(bits(got[4]), bits(thr)) and np.array_equal(
        bits(got[1]), bits(ed))


def test_harness_refusals(zg):
    x = logits_for(257)
    u = np.full(B, 0.5, np.float32)
    assert each_rows(zg, x, TABLE, u, n_rows=7)[0] == ARG and "rows" in zg.zg_last_error().decode()
    assert each_rows(zg, x, TABLE, u, edits=dict(min_p=0.1))[0] == ARG and "min_p" in zg.zg_last_error().decode()
    bad = list(TABLE)
    bad[5] = (0.8, 0, 1.5, 0.0)
    assert each_rows(zg, x, bad, u)[0] == ARG and "row 5" in zg.zg_last_error().decode()
    tok = np.zeros(B, np.uint64)
    assert zg.zg_debug_sample_rows_each(_lib.ptr(x), B, 257, None, B, None, _lib.ptr(u), None, _lib.ptr(tok), None, None) == ARG


# ---- the penalty stage: the row's own values, rows with penalties off untouched

PENS = [(1.3, 0.4, 0.15), (1.0, 0.0, 0.0), (0.7, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, -0.5, 0.25), (1.3, 0.4, 0.15), (1.0, 0.0, 0.0), (2.0, 1.0, 0.0)]
HIST_LENS = [0, 1, 40, 300, 300, 40, 1, 0]


def penalize_each(lib, x, pens, hists, n_rows=None):
    x = np.ascontiguousarray(x, np.float32)
    nb, V = x.shape
    table = _lib.row_sampling([dict(temp=1.0, repetition_penalty=r, presence_penalty=p, frequency_penalty=f) for r, p, f in pens])
    mat, lens, stride = pack(hists)
    out = np.full((nb, V), np.float32(123.0), np.float32)
    counts = np.full((nb, V), 0xFFFFFFFF, np.uint32)
    rc = lib.zg_debug_penalize_rows_each(_lib.ptr(x), nb, V, C.addressof(table), len(pens) if n_rows is None else n_rows, _lib.ptr(mat), stride, _lib.ptr(lens),
                                         _lib.ptr(out), _lib.ptr(counts))
    return rc, out, counts


@pytest.mark.parametrize("V", VOCABS)
def test_penalties_per_row_equal_the_reference_bitwise(zg, V):
    rng = np.random.default_rng(2000 + V)
    x = logits_for(V)
    x[2, V // 5: V // 5 + V // 2] = (rng.standard_normal(V // 2) * 4).astype(np.float32)  # (finite rows: every history token has a value to rewrite)
    # histories with repeats: tokens drawn from a pool a third of the length wide
    hists = [rng.integers(0, V, max(1, n // 3))[rng.integers(0, max(1, n // 3), n)] if n else np.zeros(0, np.int64) for n in HIST_LENS]
    nan = np.uint32(0x7FC12345).view(np.float32)  # a NaN with a payload
    for b in range(B):
        if len(hists[b]) >= 2:  # a NaN and a -0.0 planted at history tokens
            t_nan, t_zero = int(hists[b][0]), int(hists[b][-1])
            x[b, t_nan] = nan
            if t_zero != t_nan:
                x[b, t_zero] = np.float32(-0.0)
    for pens in (PENS, PENS[3:] + PENS[:3]):
        rc, out, counts = penalize_each(zg, x, pens, hists)
        assert rc == 0, zg.zg_last_error()
        touched = 0
        for b, (r, p, f) in enumerate(pens):
            want, c = penalize_row(x[b], hists[b], r, p, f)
            assert np.array_equal(counts[b], c), (b, np.flatnonzero(counts[b] != c)[:5])
            if (r, p, f) == (1.0, 0.0, 0.0):  # off: the input's own bits, a NaN's payload included
                assert np.array_equal(bits(out[b]), bits(x[b])), (b, np.flatnonzero(bits(out[b]) != bits(x[b]))[:5])
            else:
                assert same_bits(out[b], want), (b, (r, p, f), np.flatnonzero(bits(out[b]) != bits(want))[:5])
                touched += int((bits(out[b]) != bits(x[b])).any())
        assert touched >= 3, "the penalties changed nothing"
        again = penalize_each(zg, x, pens, hists)
        assert np.array_equal(bits(out), bits(again[1])) and np.array_equal(counts, again[2])
    assert penalize_each(zg, x, PENS, hists, n_rows=5)[0] == ARG
    assert penalize_each(zg, x, [(0.0, 0.0, 0.0)] + PENS[1:], hists)[0] == ARG and "row 0" in zg.zg_last_error().decode()
