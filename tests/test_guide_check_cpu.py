"""zg_debug_guide_check (include/zgpt2.h): every refusal a load of a table and a guided call behind it give — without
a GPU and without zg_init —, a state emptied only by the call's ban list among them, and the edge cases that are accepted."""
import ctypes as C

import numpy as np
import pytest

from guide_ref import DEAD, NONE, guide_check
from zig_gpt2_amd import _lib

ARG, SHAPE = -6, -2
V = 70  # (three bitmap words, the last holding six bits)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def cycle(n):
    """n states, state s allowing the tokens congruent to s mod 2 plus token 64 + (s % 6), each leading to s + 1."""
    t = np.full((n, V), DEAD, np.uint16)
    for s in range(n):
        t[s, s % 2: 64: 2] = (s + 1) % n
        t[s, 64 + s % 6] = (s + 1) % n
    return t


def test_the_refusals_of_a_load(lib):
    good = cycle(4)
    assert guide_check(lib, good, V) == 0
    assert guide_check(lib, good, V, n_states=0) == ARG
    assert guide_check(lib, np.zeros((257, V), np.uint16), V) == ARG and b"257" in lib.zg_last_error()
    assert guide_check(lib, good, V, null_table=True) == ARG
    assert lib.zg_debug_guide_check(None, V, None, None, 0, 0) == ARG
    bad = good.copy()
    bad[2, 5] = 4  # a transition to a state the table does not have
    assert guide_check(lib, bad, V) == ARG and b"state 2" in lib.zg_last_error()
    bad = good.copy()
    bad[3] = DEAD
    assert guide_check(lib, bad, V) == ARG and b"state 3 allows no token" in lib.zg_last_error()
    assert guide_check(lib, good, 0) == ARG


def test_the_refusals_of_a_call(lib):
    good = cycle(4)
    assert guide_check(lib, good, V, [0, 3, NONE]) == 0
    assert guide_check(lib, good, V, [0, 4]) == ARG and b"row 1" in lib.zg_last_error()
    assert guide_check(lib, good, V, [0], greedy=True) == ARG
    assert guide_check(lib, good, V, [NONE, NONE], greedy=True) == 0, "no guided row: the unguided call, greedy included"
    # the call's own lists: every state of the table must keep a token, also one no row starts in
    even = list(range(0, 64, 2))
    assert guide_check(lib, good, V, [0], allowed=even + [65, 67]) == 0
    assert guide_check(lib, good, V, [0], allowed=even) == ARG and b"state 1" in lib.zg_last_error(), "the odd states keep nothing"
    only = np.full((2, V), DEAD, np.uint16)
    only[0, [3, 69]] = 1
    only[1, 69] = 0
    assert guide_check(lib, only, V, [0], banned=[3]) == 0
    assert guide_check(lib, only, V, [0], banned=[69]) == ARG and b"state 1" in lib.zg_last_error(), "a state emptied only by the ban list"
    assert guide_check(lib, only, V, [NONE], banned=[69]) == 0, "nobody is guided: the lists are judged alone"
    assert guide_check(lib, only, V, [0], bias={69: 1.0}) == 0
    # the edits' own refusals come through unchanged
    assert guide_check(lib, only, V, [0], banned=[V]) == SHAPE
    assert guide_check(lib, only, V, [0], bias={1: float("inf")}) == ARG
    st = np.zeros(1, np.uint64)
    g_keep = np.ascontiguousarray(good)
    g = _lib.Guide(4, _lib.ptr(g_keep))
    assert lib.zg_debug_guide_check(C.addressof(g), V, None, None, 1, 0) == ARG, "null start states"
    assert lib.zg_debug_guide_check(C.addressof(g), V, None, _lib.ptr(st), 1, 0) == 0


def test_accepted_edge_cases(lib):
    one = np.full((1, V), DEAD, np.uint16)
    one[0, V - 1] = 0  # a single state allowing the last token alone
    assert guide_check(lib, one, V, [0]) == 0
    big = cycle(256)
    assert guide_check(lib, big, V, [255, 0, NONE]) == 0
    assert guide_check(lib, big, V, [256]) == ARG
    assert guide_check(lib, np.zeros((256, 1), np.uint16), 1, [17]) == 0, "a vocabulary of one token"
