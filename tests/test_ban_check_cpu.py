"""zg_debug_ban_check (include/zgpt2.h zg_ban_rules): every refusal a banned call gives, with its status — without a GPU
and without zg_init —, the bound that keeps a row from being left without a token at its edge, and what is accepted."""
import ctypes as C

import numpy as np
import pytest

from ban_ref import ban_check
from zig_gpt2_amd import _lib

ARG, SHAPE, UNSUPPORTED = -6, -2, -5
V, CTX, B = 70, 128, 3


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def check(lib, **kw):
    kw.setdefault("batch", B)
    kw.setdefault("vocab", V)
    kw.setdefault("context", CTX)
    return ban_check(lib, kw.pop("batch"), kw.pop("vocab"), kw.pop("context"), **kw)


def test_all_off_is_accepted(lib):
    assert lib.zg_debug_ban_check(None, B, V, CTX, None, 10, None, 0, 0) == 0, "no rules"
    assert check(lib) == 0
    assert check(lib, greedy=True) == 0 and check(lib, guided=True) == 0 and check(lib, context=16384) == 0, "all off: the call without rules"
    assert check(lib, min_tokens=5, greedy=True) == 0, "min_tokens without a suppress id suppresses nothing"
    assert check(lib, suppress=[3], greedy=True) == 0, "suppress ids without min_tokens are never applied"
    null = lambda r: (setattr(r, "no_repeat_ngram", None), setattr(r, "min_tokens", None))
    assert check(lib, patch=null, greedy=True) == 0, "null per-row arrays: all off"


def test_argument_refusals(lib):
    assert check(lib, n=3, patch=lambda r: setattr(r, "size", r.size - 8)) == ARG and b"size" in lib.zg_last_error()
    assert check(lib, words=[[1, 2]], patch=lambda r: setattr(r, "words", None)) == ARG and b"null array" in lib.zg_last_error()
    assert check(lib, words=[[1, 2]], patch=lambda r: setattr(r, "word_lens", None)) == ARG
    assert check(lib, min_tokens=2, suppress=[1], patch=lambda r: setattr(r, "suppress_ids", None)) == ARG
    assert check(lib, n=[0, 17, 0]) == ARG and b"row 1" in lib.zg_last_error()
    assert check(lib, n=[0, 16, 0], n_steps=4) == 0
    assert check(lib, words=[[1]] * 64) == 0 and check(lib, words=[[1]] * 65) == ARG
    assert check(lib, min_tokens=1, suppress=list(range(16))) == 0 and check(lib, min_tokens=1, suppress=list(range(17))) == ARG
    # word lengths: 0, above 16, above the stride
    assert check(lib, words=[[1], [2, 3]], patch=lambda r: C.cast(r.word_lens, C.POINTER(C.c_size_t)).__setitem__(1, 0)) == ARG and b"word 1" in lib.zg_last_error()
    assert check(lib, words=[list(range(16))]) == 0 and check(lib, words=[list(range(17))]) == ARG
    assert check(lib, words=[[1, 2, 3]], patch=lambda r: setattr(r, "word_stride", 2)) == ARG
    # greedy and guided with any rule on
    for kw in (dict(n=2, n_steps=4), dict(words=[[1, 2]]), dict(min_tokens=[0, 0, 1], suppress=[4])):
        assert check(lib, **kw) == 0
        assert check(lib, greedy=True, **kw) == ARG and b"greedy" in lib.zg_last_error()
        assert check(lib, guided=True, **kw) == ARG and b"guided" in lib.zg_last_error()


def test_shape_and_unsupported(lib):
    assert check(lib, words=[[1, V]]) == SHAPE and b"word 0" in lib.zg_last_error()
    assert check(lib, words=[[1, V - 1]]) == 0
    assert check(lib, min_tokens=1, suppress=[V]) == SHAPE
    assert check(lib, suppress=[V]) == SHAPE, "checked also while nothing applies it"
    assert check(lib, n=2, n_steps=4, context=8192) == 0
    assert check(lib, n=2, n_steps=4, context=8193) == UNSUPPORTED
    # the edits' own refusals come through unchanged
    assert check(lib, n=2, n_steps=4, banned=[V]) == SHAPE and check(lib, n=2, n_steps=4, bias={1: float("inf")}) == ARG


def test_the_bound_that_keeps_a_token_at_its_edge(lib):
    """kept < 1 + max D is refused: kept == max D refused, kept == max D + 1 accepted."""
    # n-gram alone, no lists: kept = V = 70, D = min(prior + n_steps, V)
    assert check(lib, n=[0, 2, 0], n_steps=69) == 0 and check(lib, n=[0, 2, 0], n_steps=70) == ARG
    assert b"row 1" in lib.zg_last_error()
    assert check(lib, n=[0, 2, 0], n_steps=40, prior_lens=[60, 29, 60]) == 0, "only the rows with the rule on count their history"
    assert check(lib, n=[0, 2, 0], n_steps=40, prior_lens=[0, 30, 0]) == ARG
    assert check(lib, n=1, n_steps=100, context=4096, vocab=50257) == 0
    # words and suppress ids add up; min(.., V) caps the n-gram part
    kw = dict(n=[3, 0, 0], min_tokens=[2, 0, 0], words=[[1, 2], [3]], suppress=[5, 6, 7])
    assert check(lib, n_steps=64, **kw) == 0, "D = 64 + 2 + 3 = 69 = kept - 1"
    assert check(lib, n_steps=65, **kw) == ARG, "D = 70 = kept"
    assert check(lib, n_steps=65, **dict(kw, min_tokens=[0, 2, 0])) == 0, "no row has both: max D = 65 + 2"
    # an allow-list and a ban list shrink kept: 10 allowed, one of them banned -> kept 9
    lists = dict(allowed=list(range(10)), banned=[4])
    assert check(lib, words=[[1]] * 8, **lists) == 0, "D = 8 = kept - 1"
    assert check(lib, words=[[1]] * 9, **lists) == ARG, "D = 9 = kept"
    assert check(lib, n=1, n_steps=8, **lists) == 0 and check(lib, n=1, n_steps=9, **lists) == ARG
    assert check(lib, n=1, n_steps=200, vocab=20, context=256) == ARG, "min(prior + n_steps, vocab) = vocab = kept"
