"""zg_debug_guide_rows on a real MI355X: guided decoding's mask kernel (with the edit stage's part in the same launch) and its
advance kernel against tests/guide_ref.py, bitwise.

Vocabularies of 257 (two slices, the last bitmap word holds one bit, rows of the uint16 table at odd offsets) and 50257 (64
slices of three or four 256-blocks); 1, 3 and 8 rows; tables of 1, 2 and 256 states with rows in the first and the last state.
In every case: a row without a guide beside guided ones, holding NaN payloads and -0.0 that must survive; the raw argmax of a
guided row dropped by its state; a slice left all -inf; a pick of vocab - 1; a forced pick whose transition is dead.  With the
call's edits on top: a +1e4 bias on a token the first state drops (it stays -inf there, and becomes the maximum of the rows that
keep it) and a ban list."""
import numpy as np
import pytest

import guide_ref
from guide_ref import DEAD, NONE, guide_rows

pytestmark = pytest.mark.gpu
_TABLES = {}


def table(V, S):
    """S states, each allowing about half the vocabulary with transitions anywhere; state 0 drops the whole of slice 1, token 7 and
    token V - 2, and keeps token 3; the last state keeps V - 1.  Built once per shape."""
    if (V, S) not in _TABLES:
        rng = np.random.default_rng(1000 * S + V)
        t = rng.integers(0, S, (S, V)).astype(np.uint16)
        t[rng.random((S, V)) < 0.5] = DEAD
        n_part = min(64, (V + 255) // 256)
        t[0, (np.arange(V) // 256) % n_part == 1] = DEAD
        t[0, [7, V - 2]] = DEAD
        t[0, 3] = S - 1
        if S > 1 or ((V - 1) // 256) % n_part != 1:  # (257 tokens, one state: the last token is slice 1 itself)
            t[S - 1, V - 1] = 0
        assert (t != DEAD).any(axis=1).all()
        _TABLES[(V, S)] = t
    return _TABLES[(V, S)]


def rows_of(V, B, S, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    x[:, 7] = 50.0  # the raw argmax: dropped by state 0
    states = [0] + [S - 1 if b % 2 else (b // 2) % S for b in range(1, B)]
    if B > 1:
        states[1] = NONE
        bits = x[1].view(np.uint32)
        bits[[5, 300 % V, V - 1]] = [0x7FC12345, 0xFFC00001, 0x80000000]  # NaN payloads and -0.0: the row must keep them
        x[1, 256 % V] = np.float32(-0.0)
    if B > 2:
        states[-1] = S - 1
    picks = [int(rng.integers(0, V)) for _ in range(B)]
    picks[0] = V - 2       # dead in state 0: the state stays
    if B > 1:
        picks[-1] = V - 1
    return x, states, picks


def check(zg, V, B, S, edits):
    t = table(V, S)
    x, states, picks = rows_of(V, B, S, 17 * B + S)
    rc, got, pv, pi, nxt = guide_rows(zg, x, t, states, picks, **edits)
    assert rc == 0, zg.zg_last_error()
    n_part = pv.shape[1]
    for b in range(B):
        want = guide_ref.mask_row(x[b], t, states[b], **edits)
        assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), (b, states[b], np.flatnonzero(got[b].view(np.uint32) != want.view(np.uint32))[:5])
        wv, wi = guide_ref.slice_partials(want, n_part)
        assert np.array_equal(pv[b].view(np.uint32), wv.view(np.uint32)), (b, "part_val", np.flatnonzero(pv[b] != wv)[:5])
        assert np.array_equal(pi[b], wi), (b, "part_idx", np.flatnonzero(pi[b] != wi)[:5])
        assert int(nxt[b]) == guide_ref.advance(t, states[b], picks[b]), (b, states[b], picks[b])
    # the cases the shapes were built for
    assert np.isneginf(got[0, 7]) and pi[0].min() != 7 and int(nxt[0]) == 0, "the raw argmax is dropped; a dead pick leaves the state"
    assert pv[0, 1] == guide_ref.START_VAL and pi[0, 1] == guide_ref.START_IDX, "a slice left all -inf"
    if B > 1 and not edits:
        assert np.array_equal(got[1].view(np.uint32), x[1].view(np.uint32)), "a row without a guide keeps its bits"
        assert int(nxt[1]) == NONE
    if B > 1 and S > 1:
        assert int(nxt[-1]) == 0, "a pick of vocab - 1 in the last state"
    return got, states


@pytest.mark.parametrize("S", [1, 2, 256])
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("V", [257, 50257])
def test_mask_and_advance_equal_the_reference(zg, V, B, S):
    check(zg, V, B, S, {})


@pytest.mark.parametrize("V,B,S", [(257, 3, 2), (257, 8, 256), (50257, 3, 256), (50257, 1, 1)])
def test_with_the_edit_stage_in_the_same_launch(zg, V, B, S):
    edits = dict(bias={7: 1.0e4, 3: 2.5, V - 1: -1.5, 40: 0.25}, banned=[11, 40, V - 3])
    got, states = check(zg, V, B, S, edits)
    assert np.isneginf(got[0, [7, 11, 40]]).all(), "a bias on a token the state drops leaves it -inf"
    t = table(V, S)
    for b in range(1, B):  # where the row keeps token 7 the bias makes it the maximum: the partials are those of the edited row
        if states[b] == NONE or t[states[b], 7] != DEAD:
            assert got[b, 7] == np.float32(50.0) + np.float32(1.0e4)


def test_refusals(zg):
    V = 257
    t = table(V, 2)
    x = np.zeros((2, V), np.float32)
    assert guide_rows(zg, x, t, [0, 2], [0, 0])[0] == -6, "a state the table does not have"
    bad = t.copy()
    bad[1] = DEAD
    assert guide_rows(zg, x, bad, [0, 0], [0, 0])[0] == -6
    assert guide_rows(zg, x, t, [0, 0], [0, 0], allowed=[7])[0] == -6, "state 0 drops token 7: nothing is left"
    assert guide_rows(zg, x, t, [NONE, NONE], [0, 0], allowed=[7])[0] == 0
    assert guide_rows(zg, x, t, [0, 1], [1 << 40, V])[0] == 0, "picks outside the vocabulary are not followed"
