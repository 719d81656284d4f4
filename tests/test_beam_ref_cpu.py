"""tests/beam_ref.py — the numpy-float32 reference of the beam stage — pinned against an independently written
restatement in plain Python (doubles rounded to float32 through struct, selection by repeated scans instead of a sort), over random
small tables, and against hand-worked cases for every rule: eos at rank < W and at rank >= W, pool replacement and the tie rule,
slot keeping, equal sums across slots, dead slots at c0, both done tests, finalisation and backtracking."""
import math
import struct

import numpy as np
import pytest

import beam_ref
from beam_ref import lists, random_lists

NEG = float("-inf")


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]  # a double rounded once to float32 (exact for +, / of two float32)


def before(a, b):
    """candidate a = (value, slot, j) ranks before b: value descending with NaN last, then slot, then j."""
    (va, sa, ja), (vb, sb, jb) = a, b
    na, nb = math.isnan(va), math.isnan(vb)
    if na != nb:
        return nb
    if not na and va != vb:
        return va > vb
    return (sa, ja) < (sb, jb)


class Plain:
    """The beam step and the finalisation restated without numpy, for ONE group."""

    def __init__(self, W, eos, length_penalty, early, c0):
        self.W, self.eos, self.lp, self.early, self.c0 = W, eos, f32(length_penalty), early, c0
        self.score = [0.0] + [NEG] * (W - 1)
        self.pool, self.done = [], -1

    def lenpow(self, L):
        return f32(math.pow(float(L), self.lp))

    def greater(self, a, b):
        return not math.isnan(a) and (math.isnan(b) or a > b)

    def offer(self, e):
        if len(self.pool) < self.W:
            self.pool.append(e)
            return
        w = 0
        for k in range(1, len(self.pool)):
            if not self.greater(self.pool[k][1], self.pool[w][1]):
                w = k
        if self.greater(e[1], self.pool[w][1]):
            self.pool[w] = e

    def step(self, ids, lps, col):
        W = self.W
        if self.done >= 0:
            return [(ids[s][0], s, self.score[s], lps[s][0]) for s in range(W)]
        live = range(W) if col > self.c0 else [0]
        left = [(f32(self.score[s] + lps[s][j]), s, j) for s in live for j in range(2 * W)]
        ranked = []
        while left and len(ranked) < 2 * W:
            best = left[0]
            for c in left[1:]:
                if before(c, best):
                    best = c
            left.remove(best)
            ranked.append(best)
        lp = self.lenpow(col - self.c0 + 1)
        beams = []
        for r, (v, s, j) in enumerate(ranked):
            if self.eos is not None and ids[s][j] == self.eos:
                if r < W:
                    self.offer((v, f32(v / lp), s, col))
            elif len(beams) < W:
                beams.append((v, s, j))
        if len(self.pool) == W:
            w = 0
            for k in range(1, W):
                if not self.greater(self.pool[k][1], self.pool[w][1]):
                    w = k
            best = beams[0][0] if beams else NEG
            if self.early or self.pool[w][1] >= f32(best / lp):
                self.done = col
        out = [None] * W
        for v, s, j in beams:
            if out[s] is None:
                out[s] = (ids[s][j], s, v, lps[s][j])
            else:
                out.append((ids[s][j], s, v, lps[s][j]))
        extra = out[W:]
        out = out[:W]
        for t in range(W):
            if out[t] is None:
                out[t] = extra.pop(0) if extra else (ids[t][0], t, NEG, lps[t][0])
        self.score = [o[2] for o in out]
        return out


@pytest.mark.parametrize("W", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("early", [True, False])
@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.0])
def test_reference_equals_the_plain_restatement(W, early, length_penalty):
    rng = np.random.default_rng(1000 * W + 10 * int(early) + int(length_penalty))
    V, c0 = 40, 5
    for trial in range(12):
        eos = None if trial % 4 == 0 else 7
        ref = beam_ref.Beams(W, W, eos, length_penalty, early, c0, n_lenpow=64)
        alt = Plain(W, eos, length_penalty, early, c0)
        for col in range(c0, c0 + 12):
            ids, lps = random_lists(rng, W, V, eos, 0.35, ties=trial % 2 == 1)
            tok, par, sc, lp = ref.step(ids, lps, col)
            got = alt.step(ids.tolist(), [[float(x) for x in row] for row in lps], col)
            assert [int(t) for t in tok] == [g[0] for g in got], (trial, col)
            assert [int(p) for p in par] == [g[1] for g in got], (trial, col)
            assert np.array_equal(beam_ref.bits(sc), beam_ref.bits([g[2] for g in got])), (trial, col)
            assert np.array_equal(beam_ref.bits(lp), beam_ref.bits([g[3] for g in got])), (trial, col)
            assert ref.done_col[0] == alt.done
            assert [(float(e["sum"]), float(e["norm"]), e["parent"], e["col"]) for e in ref.pools[0]] == [tuple(e) for e in alt.pool]


def test_dead_slots_at_c0_and_slot_keeping():
    b = beam_ref.Beams(2, 2, None, 1.0, True, c0=3, n_lenpow=16)
    # at c0 slot 1's list is ignored although it is better: only slot 0 is live
    ids, lps = lists(2, [[(10, -1.0), (11, -2.0), (12, -3.0), (13, -4.0)], [(20, -0.1), (21, -0.2), (22, -0.3), (23, -0.4)]])
    tok, par, sc, lp = b.step(ids, lps, 3)
    assert tok.tolist() == [10, 11] and par.tolist() == [0, 0] and sc.tolist() == [-1.0, -2.0] and lp.tolist() == [-1.0, -2.0]
    # the best candidate comes from slot 1 and keeps slot 1; the second comes from slot 1 too and takes the free slot 0
    ids, lps = lists(2, [[(30, -5.0), (31, -6.0)], [(40, -0.5), (41, -1.0)]])
    tok, par, sc, lp = b.step(ids, lps, 4)
    assert tok.tolist() == [41, 40] and par.tolist() == [1, 1] and sc.tolist() == [-3.0, -2.5] and lp.tolist() == [-1.0, -0.5]


def test_equal_sums_across_slots_go_to_the_lower_slot_then_the_lower_entry():
    b = beam_ref.Beams(2, 2, None, 1.0, True, c0=0, n_lenpow=16)
    b.score[:] = [-1.0, -2.0]
    ids, lps = lists(2, [[(10, -2.0), (11, -2.0)], [(20, -1.0), (21, -1.0)]])  # four candidates of value -3
    tok, par, sc, _ = b.step(ids, lps, 1)
    assert tok.tolist() == [10, 11] and par.tolist() == [0, 0] and sc.tolist() == [-3.0, -3.0]


def test_eos_below_rank_w_is_pooled_and_at_rank_w_or_above_is_dropped():
    eos = 7
    b = beam_ref.Beams(2, 2, eos, 1.0, False, c0=0, n_lenpow=16)
    b.score[:] = [0.0, -1.0]
    # ranks: (s0, 10, -0.5), (s1, eos, -1.1), (s0, 11, -3.0), (s0 eos, -4.0) ...: eos at rank 1 < W pooled, eos at rank 3 >= W dropped
    ids, lps = lists(2, [[(10, -0.5), (11, -3.0), (eos, -4.0)], [(eos, -0.1), (21, -9.0)]])
    tok, par, sc, _ = b.step(ids, lps, 1)
    assert tok.tolist() == [10, 11] and par.tolist() == [0, 0] and sc.tolist() == [-0.5, -3.0]
    assert len(b.pools[0]) == 1
    e = b.pools[0][0]
    assert (float(e["sum"]), float(e["norm"]), e["parent"], e["col"]) == (float(np.float32(-1.1)), float(np.float32(-1.1) / np.float32(2.0)), 1, 1)
    assert b.done_col == [-1] and b.host_done_col() == 0


def test_pool_replacement_and_the_tie_rule():
    pool = []
    for k, norm in enumerate([-2.0, -3.0, -3.0]):
        beam_ref.offer(pool, 3, {"sum": np.float32(norm), "norm": np.float32(norm), "parent": k, "col": 1})
    beam_ref.offer(pool, 3, {"sum": np.float32(-3.0), "norm": np.float32(-3.0), "parent": 9, "col": 2})  # not strictly greater: refused
    assert [e["parent"] for e in pool] == [0, 1, 2]
    beam_ref.offer(pool, 3, {"sum": np.float32(-2.5), "norm": np.float32(-2.5), "parent": 9, "col": 2})  # replaces the LATER of the two worst
    assert [e["parent"] for e in pool] == [0, 1, 9]
    beam_ref.offer(pool, 3, {"sum": np.float32(np.nan), "norm": np.float32(np.nan), "parent": 8, "col": 3})  # NaN never wins
    assert [e["parent"] for e in pool] == [0, 1, 9]
    beam_ref.offer(pool, 3, {"sum": np.float32(-1.0), "norm": np.float32(-1.0), "parent": 7, "col": 3})
    assert [e["parent"] for e in pool] == [0, 7, 9]


@pytest.mark.parametrize("early", [True, False])
def test_both_done_tests(early):
    eos = 7
    b = beam_ref.Beams(2, 2, eos, 1.0, early, c0=0, n_lenpow=16)
    # column 0: eos at rank 0 is pooled (sum -1, norm -1 / 1); the beams are 10 (-1.5) and 11 (-2.0).  One entry of two: not done
    ids, lps = lists(2, [[(eos, -1.0), (10, -1.5), (11, -2.0), (12, -2.5)], []])
    b.step(ids, lps, 0)
    assert b.done_col == [-1] and len(b.pools[0]) == 1
    # column 1: 13 at -1.6 (rank 0), eos at -2.0 (rank 1 < W: pooled, norm -2 / 2 = -1), 14 at -2.1.  The pool is full with worst
    # norm -1; the best new beam has -1.6 / 2 = -0.8 > -1: done only under early stopping
    ids, lps = lists(2, [[(13, -0.1), (eos, -0.5)], [(14, -0.1), (15, -9.0)]])
    tok, par, sc, _ = b.step(ids, lps, 1)
    assert tok.tolist() == [13, 14] and par.tolist() == [0, 1] and len(b.pools[0]) == 2
    assert [float(e["norm"]) for e in b.pools[0]] == [-1.0, -1.0]
    assert b.done_col == [1 if early else -1]
    assert b.host_done_col() == (2 if early else 0)
    # column 2: the best new beam falls to -4.6 / 3 < -1: the second test fires
    ids, lps = lists(2, [[(16, -3.0), (17, -3.5)], [(18, -3.0), (19, -4.0)]])
    tok, par, sc, _ = b.step(ids, lps, 2)
    if early:  # a done group: identity parents, the slots' own first tokens, scores as they stood
        assert tok.tolist() == [16, 18] and par.tolist() == [0, 1] and np.array_equal(sc, np.array([-1.6, -2.1], np.float32))
        assert b.done_col == [1]
    else:
        assert tok.tolist() == [16, 17] and par.tolist() == [0, 0] and b.done_col == [2] and b.host_done_col() == 3


def test_finalize_backtracks_through_the_parents():
    eos, W, c0 = 7, 2, 2
    b = beam_ref.Beams(2, W, eos, 1.0, False, c0=c0, n_lenpow=16)
    out_tokens = np.zeros((2, 8), np.int64)
    parents = np.zeros((2, 8), np.int64)
    steps = [
        [[(10, -1.0), (11, -2.0), (12, -3.0), (13, -4.0)], []],
        [[(20, -5.0), (21, -6.0)], [(30, -0.5), (31, -1.0)]],       # both beams come from slot 1
        [[(eos, -0.25), (40, -0.5)], [(50, -0.5), (51, -9.0)]],
    ]
    for i, rows in enumerate(steps):
        ids, lps = lists(W, rows)
        tok, par, _, _ = b.step(ids, lps, c0 + i)
        out_tokens[:, c0 + i], parents[:, c0 + i] = tok, par
    # column 3: 30 (from slot 1, keeps it) and 31 (from slot 1, moves to slot 0)
    assert out_tokens[:, 3].tolist() == [31, 30] and parents[:, 3].tolist() == [1, 1]
    # column 4: 50 (slot 1, -3.0) at rank 0, eos behind slot 0 at -3.25 (rank 1: pooled), 40 (slot 0, -3.5)
    assert out_tokens[:, 4].tolist() == [40, 50] and parents[:, 4].tolist() == [0, 1]
    assert [(float(e["sum"]), e["parent"], e["col"]) for e in b.pools[0]] == [(-3.25, 0, 4)]
    # the group is not done: slot 0 (-3.5 / 3) fills the pool, slot 1 (-3.0 / 3) replaces it as the worst; best first
    res = b.finalize(5, out_tokens, parents, 2)[0]
    assert [r[0] for r in res] == [[11, 30, 50], [11, 31, eos]]
    assert [float(r[2]) for r in res] == [-3.0, -3.25]
    assert [float(r[1]) for r in res] == [-1.0, float(np.float32(-3.25) / np.float32(3.0))]
    assert [r[0] for r in b.finalize(5, out_tokens, parents, 1)[0]] == [[11, 30, 50]]
