"""The NumPy statement of the history-dependent bans (tests/ban_ref.py; include/zgpt2.h zg_ban_rules) on cases worked
by hand and against an independent brute force that enumerates every n-gram into a dict, as HF does; then the host twin
zig_gpt2_amd.bans.banned_now against it on seeded random inputs, and the binding of the new names.  No GPU."""
import numpy as np
import pytest

import ban_ref
from ban_ref import ban_set, ngram_bans_by_dict
from zig_gpt2_amd import _lib, bans


def test_ngram_edges_by_hand():
    # L = n - 2: nothing; L = n - 1: the suffix is the whole history and there is no window
    assert ban_set([5], 0, n=3) == [] and ban_set([5, 6], 0, n=3) == []
    # a match at window 0 and at the last window (L = 6, n = 3: windows 0 .. 3, suffix h[4 .. 6) = [1, 2])
    assert ban_set([1, 2, 9, 7, 1, 2], 0, n=3) == [9]
    assert ban_set([7, 8, 3, 1, 2, 4, 1, 2], 0, n=3) == [4]
    assert ban_set([9, 5, 5, 5], 0, n=3) == [5], "the last window (i = L - n = 1) overlaps the suffix and bans the last token itself"
    assert ban_set([0, 0, 3, 1, 2, 1, 2], 0, n=3) == [1]
    assert ban_set([1, 2, 3, 9, 1, 2, 4, 1, 2], 0, n=3) == [3, 4], "two windows, two tokens"
    # the window that overlaps the suffix: all-equal history, n = 3 — every window matches and they all ban the same token
    assert ban_set([4, 4, 4, 4, 4], 0, n=3) == [4]
    assert ban_set([4, 4], 0, n=3) == [] and ban_set([4, 4, 4], 0, n=3) == [4]
    # n = 1 bans every token of the history; n = 2 the followers of the last token
    assert ban_set([3, 1, 3, 7], 0, n=1) == [1, 3, 7] and ban_set([], 0, n=1) == []
    assert ban_set([3, 1, 3, 7, 3], 0, n=2) == [1, 7]
    assert ban_set([3, 1, 3], 5, n=0) == []


def test_words_by_hand():
    # longer than the history (L < m - 1): nothing; matching at L = m - 1: the whole history is the prefix
    assert ban_set([1, 2], 0, words=[[1, 2, 3, 4]]) == []
    assert ban_set([1, 2, 3], 0, words=[[1, 2, 3, 4]]) == [4]
    assert ban_set([9, 1, 2, 3], 0, words=[[1, 2, 3, 4]]) == [4] and ban_set([1, 2, 3, 9], 0, words=[[1, 2, 3, 4]]) == []
    # a one-token word is always banned, on an empty history too
    assert ban_set([], -3, words=[[6]]) == [6] and ban_set([1, 2], 0, words=[[6]]) == [6]
    # two words banning one token; a word and an n-gram banning the same one
    assert ban_set([5, 1, 2], 0, words=[[1, 2, 8], [2, 8], [5, 9]]) == [8]
    assert ban_set([1, 2, 8, 1, 2], 0, n=3, words=[[2, 8]]) == [8]


def test_min_tokens_by_hand():
    kw = dict(min_tokens=4, suppress=[7, 2])
    assert ban_set([1], 3, **kw) == [2, 7], "picked = min - 1: banned"
    assert ban_set([1], 4, **kw) == [], "picked = min: not banned"
    assert ban_set([1], 0, **kw) == [2, 7] and ban_set([1], -1, **kw) == [], "a prompt column is not suppressed"
    assert ban_set([1], 0, min_tokens=0, suppress=[7]) == [] and ban_set([1], 0, min_tokens=3, suppress=[]) == []


def test_a_token_outside_the_vocabulary_matches_nothing_and_bans_nothing():
    V = 10
    assert ban_set([3, 12, 3], 0, n=1, vocab=V) == [3]
    assert ban_set([12, 4, 5, 12, 4], 0, n=3, vocab=V) == [], "the suffix holds it: no window equals it"
    assert ban_set([4, 12, 4, 1, 4], 0, n=2, vocab=V) == [1], "it would be banned as a follower of 4: it is skipped"
    assert ban_set([12, 4, 5, 12, 4], 0, n=3) == [5], "(without a vocabulary it is a token like any other)"


@pytest.mark.parametrize("seed", range(6))
def test_ngram_rule_equals_the_dict_brute_force(seed):
    rng = np.random.default_rng(seed)
    for _ in range(300):
        alphabet = int(rng.integers(1, 5))  # small alphabets: repeats are the rule
        L = int(rng.integers(0, 40))
        n = int(rng.integers(0, ban_ref.MAX_NGRAM + 1))
        h = rng.integers(0, alphabet, L)
        assert ban_set(h, 0, n=n) == ngram_bans_by_dict(h, n), (list(h), n)


@pytest.mark.parametrize("seed", range(6))
def test_the_host_twin_equals_the_reference(seed):
    rng = np.random.default_rng(100 + seed)
    V = 12
    for _ in range(300):
        L = int(rng.integers(0, 30))
        h = rng.integers(0, int(rng.integers(1, V + 3)), L)  # (sometimes with tokens >= vocab)
        n = int(rng.integers(0, 6))
        words = [list(rng.integers(0, 4, int(rng.integers(1, 5)))) for _ in range(int(rng.integers(0, 5)))]
        picked, mt = int(rng.integers(-2, 6)), int(rng.integers(0, 5))
        supp = list(rng.integers(0, V, int(rng.integers(0, 4))))
        want = ban_set(h, picked, n=n, words=words, min_tokens=mt, suppress=supp, vocab=V)
        assert bans.banned_now(h, picked, n, words, mt, supp, vocab=V) == want, (list(h), picked, n, words, mt, supp)
    with pytest.raises(ValueError):
        bans.banned_now([1], 0, n=17)
    with pytest.raises(ValueError):
        bans.banned_now([1], 0, words=[[]])


def test_the_new_names_are_bound():
    lib = _lib.load()
    for name in ("zg_gpt_generate_banned_enqueue", "zg_debug_ban_check", "zg_debug_ban_rows"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert (_lib.BAN_MAX_NGRAM, _lib.BAN_MAX_WORDS, _lib.BAN_MAX_WORD_LEN, _lib.BAN_MAX_SUPPRESS) == (16, 64, 16, 16)
    assert _lib.GPT_BANNED_GENERATE == 1 << 16
    assert (bans.MAX_NGRAM, bans.MAX_WORDS, bans.MAX_WORD_LEN, bans.MAX_SUPPRESS) == (ban_ref.MAX_NGRAM, ban_ref.MAX_WORDS, ban_ref.MAX_WORD_LEN, ban_ref.MAX_SUPPRESS)
