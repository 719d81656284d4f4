"""The NumPy statement of guided decoding (tests/guide_ref.py) on examples worked by hand, and the builders of
zig_gpt2_amd/guide.py: choices that share prefixes, a byte DFA for [0-9]+\\n over a synthetic vocabulary with
multi-byte tokens, union offsets, and the ValueErrors.  No GPU: the tables are checked by the library's own rules through
zg_debug_guide_check."""
import numpy as np
import pytest

import guide_ref
from guide_ref import DEAD, NONE
from zig_gpt2_amd import guide
from zig_gpt2_amd.guide import Guide

D = DEAD


def test_mask_partials_advance_and_record_on_a_hand_worked_table():
    nxt = np.array([[1, D, 0, D, D, D], [D, 1, D, D, D, 0]], np.uint16)
    x = np.array([3.0, -0.0, np.nan, 9.0, -np.inf, 1.0], np.float32)
    y = guide_ref.mask_row(x, nxt, 0)
    assert np.isneginf(y[[1, 3, 4, 5]]).all() and y[0] == 3.0 and np.isnan(y[2])
    assert np.array_equal(guide_ref.mask_row(x, nxt, NONE).view(np.uint32), x.view(np.uint32)), "a row without a guide keeps its bits"
    y = guide_ref.mask_row(x, nxt, 1, bias={1: 2.0, 3: 1e4}, banned=[5])
    assert y[1] == 2.0 and np.isneginf(y[[0, 2, 3, 4, 5]]).all(), "a bias on a dropped token leaves it -inf; the ban and the state intersect"
    val, idx = guide_ref.slice_partials(guide_ref.mask_row(x, nxt, 0), 1)
    assert val[0] == 3.0 and idx[0] == 0, "the raw argmax (index 3) is banned by the state"
    val, idx = guide_ref.slice_partials(np.full(6, -np.inf, np.float32), 1)
    assert val[0] == guide_ref.START_VAL and idx[0] == guide_ref.START_IDX
    # slices: 600 elements over two slices of 256-blocks: block 0 and 2 are slice 0, block 1 is slice 1
    z = np.zeros(600, np.float32)
    z[300], z[520], z[10] = 5.0, 7.0, 7.0
    val, idx = guide_ref.slice_partials(z, 2)
    assert list(val) == [7.0, 5.0] and list(idx) == [10, 300]
    assert guide_ref.advance(nxt, 0, 0) == 1 and guide_ref.advance(nxt, 0, 1) == 0 and guide_ref.advance(nxt, 0, 99) == 0
    assert guide_ref.advance(nxt, NONE, 0) == NONE
    rec, end = guide_ref.record(nxt, [0, NONE], np.array([[4, 4, 0, 1, 5, 2], [0, 0, 0, 0, 0, 0]]), [2, 1])
    assert list(rec[0]) == [NONE, NONE, 0, 1, 1, 0] and (rec[1] == NONE).all() and end == [0, NONE]


def test_choices_that_share_prefixes():
    V, end = 50, 49
    choices = [[7, 8], [7, 8, 9], [7, 3], [12]]
    g = Guide.from_choices(choices, V, end)
    done = g.n_states - 1
    assert g.n_states == 4  # root, [7], [7, 8], done
    assert list(g.allowed(0)) == [7, 12] and list(g.allowed(done)) == [end] and g.step(done, end) == done
    s7 = g.step(0, 7)
    assert list(g.allowed(s7)) == [3, 8] and g.step(s7, 3) == done and g.step(0, 12) == done
    s78 = g.step(s7, 8)
    assert list(g.allowed(s78)) == [9, end], "a choice that a longer one continues may end or go on"
    assert g.walk(0, [7, 8, 9]) == done and g.walk(0, [7, 8, end, end]) == done
    with pytest.raises(ValueError):
        g.step(0, 8)
    # every accepted path is a choice, and every choice is a path
    def paths(st, prefix):
        for t in g.allowed(st):
            if t == end:
                yield tuple(prefix)
            else:
                yield from paths(g.step(st, int(t)), prefix + [int(t)]) if g.step(st, int(t)) != done else [tuple(prefix + [int(t)])]
    assert sorted(paths(0, [])) == sorted(tuple(c) for c in choices)


def digits_dfa():
    """[0-9]+\\n: state 0 start, 1 some digits, 2 behind the newline (accepting)."""
    trans = np.full((3, 256), -1, np.int64)
    trans[0, ord("0"): ord("9") + 1] = 1
    trans[1, ord("0"): ord("9") + 1] = 1
    trans[1, ord("\n")] = 2
    return trans


def test_byte_dfa_for_digits_then_newline_over_multi_byte_tokens():
    toks = [b"0", b"7", b"42", b"\n", b"9\n", b"a", b"4a", b"\n\n", b"", b"<end>", b"12\n3"]
    end = 9
    g = Guide.from_byte_dfa(digits_dfa(), 0, [2], toks, end)
    assert g.vocab == len(toks) and g.n_states == 4  # start, digits, behind the newline, done
    assert list(g.allowed(0)) == [0, 1, 2, 4], "digits, and 9\\n which crosses two byte states; never a bare newline or a letter"
    digits = g.step(0, 0)
    assert g.step(0, 2) == digits and list(g.allowed(digits)) == [0, 1, 2, 3, 4]
    after = g.step(digits, 3)
    assert g.step(0, 4) == after and list(g.allowed(after)) == [end]
    done = g.step(after, end)
    assert list(g.allowed(done)) == [end] and g.step(done, end) == done
    assert g.walk(0, [2, 1, 4, end, end]) == done
    # unreachable byte states are dropped: start at `digits`' byte state and the start state is gone
    assert Guide.from_byte_dfa(digits_dfa(), 1, [2], toks, end).n_states == 3


def test_byte_dfa_value_errors():
    toks = [b"0", b"1", b"\n", b"<end>"]
    with pytest.raises(ValueError, match="allows no token"):  # the newline's state is reachable, not accepting, and nothing follows
        Guide.from_byte_dfa(digits_dfa(), 0, [], toks, 3)
    # a counter of 300 byte states, one per digit read: more than 256 remain
    trans = np.full((300, 256), -1, np.int64)
    for s in range(299):
        trans[s, ord("0")] = s + 1
    trans[299, ord("0")] = 299
    with pytest.raises(ValueError, match="256"):
        Guide.from_byte_dfa(trans, 0, [], toks, 3)
    with pytest.raises(ValueError):
        Guide.from_byte_dfa(np.zeros((3, 255)), 0, [], toks, 3)


def test_union_offsets_and_the_library_rules():
    V = 20
    a = Guide.from_choices([[1, 2], [3]], V, 19)
    b = Guide.from_choices([[4]], V, 19)
    c = Guide(np.zeros((1, V), np.uint16))  # one state that allows everything and loops
    u, off = Guide.union([a, b, c])
    assert off == [0, a.n_states, a.n_states + b.n_states] and u.n_states == a.n_states + b.n_states + 1
    for g, o in zip((a, b, c), off):
        for s in range(g.n_states):
            assert list(u.allowed(o + s)) == list(g.allowed(s))
            for t in g.allowed(s):
                assert u.step(o + s, int(t)) == g.step(s, int(t)) + o
    with pytest.raises(ValueError):
        Guide.union([a, Guide(np.zeros((1, V + 1), np.uint16))])
    with pytest.raises(ValueError):
        Guide.union([Guide(np.zeros((200, V), np.uint16)), Guide(np.zeros((57, V), np.uint16))])
    assert Guide.union([Guide(np.zeros((200, V), np.uint16)), Guide(np.zeros((56, V), np.uint16))])[0].n_states == 256
    # the library's own rules, as ValueError: a state allowing nothing (named), a transition out of range, too many states
    with pytest.raises(ValueError, match="state 1 allows no token"):
        Guide(np.array([[0, 1], [D, D]]))
    with pytest.raises(ValueError, match="state 0 goes to state 2"):
        Guide(np.array([[2, 1], [0, D]]))
    with pytest.raises(ValueError):
        Guide(np.zeros((257, 4), np.uint16))
    with pytest.raises(ValueError):
        Guide.from_choices([[1], []], V, 19)
    with pytest.raises(ValueError):
        Guide.from_choices([[1, 19]], V, 19)
    assert guide.NONE == NONE and guide.DEAD == DEAD and guide.MAX_STATES == 256
