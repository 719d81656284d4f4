"""zg_debug_beam_rows — the beam kernel alone (sample_beam.h), launched once per column over given top-2W lists with
its state carried from column to column — is bit for bit tests/beam_ref.py: tokens, parents, scores, the chosen entries' bits, the
pools, the groups' done columns and the word the host is told.  Random lists (with eos sprinkled in, and on a coarse grid so that
sums tie across slots and entries) at every (num_beams, batch) shape the stage is specified for, and the hand-worked cases of
tests/test_beam_ref_cpu.py plus a NaN entry."""
import ctypes as C

import numpy as np
import pytest

import beam_ref
from beam_ref import bits, lists, random_lists
from zig_gpt2_amd import _lib

pytestmark = pytest.mark.gpu
V = 40
ERR_SHAPE, ERR_ARG = -2, -6


def device_rows(zg, ids, lps, W, first_col=0, vocab=1000, expect=0, **opt):
    """zg_debug_beam_rows over ids / lps [n_cols][batch][2W]: dict of what it returns."""
    ids = np.ascontiguousarray(ids, np.int32)
    lps = np.ascontiguousarray(lps, np.float32)
    n_cols, B = ids.shape[:2]
    o = _lib.beam_options(W, **opt)
    G = B // W if 0 < W <= B else B  # (a refused shape: any size will do)
    out = dict(tokens=np.zeros((n_cols, B), np.int32), parents=np.zeros((n_cols, B), np.int32), scores=np.zeros((n_cols, B), np.float32),
               logprobs=np.zeros((n_cols, B), np.float32), pool=np.zeros((B, 4), np.float32), pool_n=np.zeros(G, np.int32),
               done_cols=np.zeros(G, np.int32))
    done = C.c_size_t()
    rc = zg.zg_debug_beam_rows(_lib.ptr(ids), _lib.ptr(lps), n_cols, B, vocab, first_col, C.addressof(o), *(_lib.ptr(out[k]) for k in (
        "tokens", "parents", "scores", "logprobs", "pool", "pool_n", "done_cols")), C.byref(done))
    assert rc == expect, (rc, zg.zg_last_error())
    out["done_col"] = done.value
    return out


def check_against_ref(got, ids, lps, W, first_col, eos=None, length_penalty=1.0, early_stopping=True, tag=None):
    n_cols, B = ids.shape[:2]
    ref = beam_ref.Beams(B, W, eos, length_penalty, early_stopping, c0=first_col, n_lenpow=n_cols + 2)
    for c in range(n_cols):
        tok, par, sc, lp = ref.step(ids[c], lps[c], first_col + c)
        assert np.array_equal(got["tokens"][c], tok), (tag, c, got["tokens"][c], tok)
        assert np.array_equal(got["parents"][c], par), (tag, c, got["parents"][c], par)
        assert np.array_equal(bits(got["scores"][c]), bits(sc)), (tag, c, got["scores"][c], sc)
        assert np.array_equal(bits(got["logprobs"][c]), bits(lp)), (tag, c)
    assert got["done_cols"].tolist() == ref.done_col, (tag, got["done_cols"], ref.done_col)
    assert got["done_col"] == ref.host_done_col(), tag
    for g in range(B // W):
        assert got["pool_n"][g] == len(ref.pools[g]), (tag, g)
        for k, e in enumerate(ref.pools[g]):
            row = got["pool"][g * W + k]
            assert np.array_equal(bits(row[:2]), bits([e["sum"], e["norm"]])), (tag, g, k, row, e)
            assert (int(row[2]), int(row[3])) == (e["parent"], e["col"]), (tag, g, k, row, e)
    return ref


@pytest.mark.parametrize("W,B", [(1, 1), (2, 2), (3, 3), (4, 8), (8, 8)])
def test_random_lists_bit_for_bit(zg, W, B):
    rng = np.random.default_rng(100 * W + B)
    n_cols, forks, moves, pooled, done = 20, 0, 0, 0, 0  # (a pool of 8 needs 8 offers at rank < W: many columns, eos in most lists)
    for trial in range(12):
        eos = None if trial % 4 == 0 else 7
        early, lp, first_col = trial % 2 == 0, [0.0, 1.0, 2.0][trial % 3], [0, 5, 70][trial % 3]
        both = [random_lists(rng, W, V, eos, 0.9, ties=trial % 3 == 1, rows=B) for _ in range(n_cols)]
        ids, lps = np.stack([x[0] for x in both]), np.stack([x[1] for x in both])
        got = device_rows(zg, ids, lps, W, first_col, V, eos_token_id=eos, length_penalty=lp, early_stopping=early)
        ref = check_against_ref(got, ids, lps, W, first_col, eos, lp, early, tag=(W, B, trial))
        par = got["parents"]
        forks += sum(len(set(par[c])) < B for c in range(1, n_cols))
        moves += int((par[1:] != np.arange(B)).sum())
        pooled += sum(len(p) for p in ref.pools)
        done += sum(d >= 0 for d in ref.done_col)
    if W > 1:  # (the lists made the stage do something: beams shared parents and changed slots, pools filled, groups ended)
        assert forks > 0 and moves > 0
    assert pooled > 0 and done > 0


def test_hand_worked_cases(zg):
    eos = 7
    # eos at rank 1 < W pooled, at rank 3 >= W dropped (column 1 of a generation whose scores column 0 set to 0 and -1)
    c0 = lists(2, [[(10, 0.0), (11, -1.0), (12, -60.0), (13, -61.0)], []])
    c1 = lists(2, [[(10, -0.5), (11, -3.0), (eos, -4.0)], [(eos, -0.1), (21, -9.0)]])
    ids, lps = np.stack([c0[0], c1[0]]), np.stack([c0[1], c1[1]])
    got = device_rows(zg, ids, lps, 2, eos_token_id=eos, early_stopping=False)
    check_against_ref(got, ids, lps, 2, 0, eos, 1.0, False, "eos ranks")
    assert got["tokens"][1].tolist() == [10, 11] and got["pool_n"].tolist() == [1] and got["pool"][0].tolist()[2:] == [1.0, 1.0]
    # dead slots at c0, slot keeping, and a beam that moves into the free slot
    cols = [lists(2, [[(10, -1.0), (11, -2.0), (12, -3.0), (13, -4.0)], [(20, -0.1), (21, -0.2), (22, -0.3), (23, -0.4)]]),
            lists(2, [[(30, -5.0), (31, -6.0)], [(40, -0.5), (41, -1.0)]])]
    ids, lps = np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols])
    got = device_rows(zg, ids, lps, 2, first_col=3)
    check_against_ref(got, ids, lps, 2, 3, tag="slots")
    assert got["tokens"].tolist() == [[10, 11], [41, 40]] and got["parents"].tolist() == [[0, 0], [1, 1]]
    # equal sums across slots: the lower slot, then the lower entry
    cols = [lists(2, [[(10, -1.0), (11, -2.0)], []]), lists(2, [[(12, -2.0), (13, -2.0)], [(20, -1.0), (21, -1.0)]])]
    ids, lps = np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols])
    got = device_rows(zg, ids, lps, 2)
    check_against_ref(got, ids, lps, 2, 0, tag="ties")
    assert got["tokens"][1].tolist() == [12, 13] and got["parents"][1].tolist() == [0, 0]
    # both done tests, on the columns of test_beam_ref_cpu.test_both_done_tests
    cols = [lists(2, [[(eos, -1.0), (10, -1.5), (11, -2.0), (12, -2.5)], []]), lists(2, [[(13, -0.1), (eos, -0.5)], [(14, -0.1), (15, -9.0)]]),
            lists(2, [[(16, -3.0), (17, -3.5)], [(18, -3.0), (19, -4.0)]])]
    ids, lps = np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols])
    for early, done_at in ((True, 1), (False, 2)):
        got = device_rows(zg, ids, lps, 2, eos_token_id=eos, early_stopping=early)
        check_against_ref(got, ids, lps, 2, 0, eos, 1.0, early, ("done", early))
        assert got["done_cols"].tolist() == [done_at] and got["done_col"] == done_at + 1
    # pool replacement and the tie rule.  One good beam stays in front (rank 0), eos follows it at rank 1 < W, column by column:
    #   column 0: sum -2 / 1 = -2 pooled; column 1: -6 / 2 = -3 pooled (the pool of two is full); column 2: -9 / 3 = -3, not strictly
    #   greater than the worst: refused; column 3: -8 / 4 = -2 takes the worst entry's place: norms [-2, -2]; column 4: -7.5 / 5 = -1.5
    #   replaces the entry at the HIGHER index of the two equal worst
    cols = [lists(2, [[(eos, -2.0), (10, -2.5), (11, -9.0), (12, -9.5)], []]),
            lists(2, [[(13, -0.25), (eos, -3.5)], [(14, -7.0), (15, -9.0)]]),
            lists(2, [[(16, -0.25), (eos, -6.25)], [(17, -0.25), (18, -9.0)]]),
            lists(2, [[(19, -0.25), (eos, -5.0)], [(20, -0.25), (21, -9.0)]]),
            lists(2, [[(22, -0.25), (eos, -4.25)], [(23, -0.25), (24, -9.0)]])]
    ids, lps = np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols])
    got = device_rows(zg, ids, lps, 2, eos_token_id=eos, early_stopping=False)
    ref = check_against_ref(got, ids, lps, 2, 0, eos, 1.0, False, "pool")
    assert [e["col"] for e in ref.pools[0]] == [0, 4] and [float(e["norm"]) for e in ref.pools[0]] == [-2.0, -1.5]
    assert got["pool"][:, 3].tolist() == [0.0, 4.0] and got["done_cols"].tolist() == [-1]


def test_a_nan_entry_never_wins(zg):
    cols = [lists(2, [[(10, -1.0), (11, -2.0), (12, -3.0), (13, -4.0)], []]), lists(2, [[(14, np.nan), (15, -0.5)], [(16, -0.25), (17, -9.0)]])]
    ids, lps = np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols])
    got = device_rows(zg, ids, lps, 2)
    check_against_ref(got, ids, lps, 2, 0, tag="nan")
    assert got["tokens"][1].tolist() == [15, 16] and not np.isnan(got["scores"]).any()


def test_refusals(zg):
    ids, lps = lists(2, [[(10, -1.0)], []])
    ids, lps = ids[None], lps[None]
    device_rows(zg, ids, lps, 0, expect=ERR_ARG)
    device_rows(zg, ids[:, :1], lps[:, :1], 2, expect=ERR_ARG)            # one row, two beams
    device_rows(zg, ids, lps, 2, vocab=3, expect=ERR_ARG)                 # 2 W > vocab
    device_rows(zg, ids, lps, 2, length_penalty=float("nan"), expect=ERR_ARG)
    device_rows(zg, ids, lps, 2, vocab=V, eos_token_id=V, expect=ERR_SHAPE)
