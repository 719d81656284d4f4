"""The teeth of tests/edit_ref.py, and the one piece of the library's edit path that runs without a GPU: zg_debug_min_p_offset."""
import ctypes as C

import numpy as np

from edit_ref import MIN_P_CASES, edit_row, filter_row_edit, min_p_offset, same_bits
from trunc_ref import filter_row


def rows(V, n, seed):
    return (3.0 * np.random.default_rng(seed).standard_normal((n, V))).astype(np.float32)


def test_min_p_zero_is_filter_row():
    for V in (1, 2, 65, 4097):
        for x in rows(V, 3, 10 + V):
            for k, p in ((0, 1.0), (7, 1.0), (0, 0.9), (12, 0.8)):
                a, b = filter_row(x, 0.8, k, p), filter_row_edit(x, 0.8, k, p, 0.0)
                assert np.array_equal(a.kept, b.kept) and a.tau == b.tau and np.array_equal(a.probs, b.probs)


def test_the_cut_is_a_ratio_and_keeps_the_top_token():
    for V in (2, 65, 4097):
        for x in rows(V, 3, 20 + V):
            for temp, mp in MIN_P_CASES:
                r = filter_row_edit(x, temp, 0, 1.0, mp)
                assert r.kept[int(x.argmax())] and abs(r.probs.sum() - 1.0) < 1e-12 and (r.probs[~r.kept] == 0).all()
                if mp == 0.0:
                    assert r.kept.all()
                    continue
                # HF's statement of the same cut on the temperature-scaled distribution, away from the boundary
                pr = filter_row(x, temp).probs
                ratio = pr / pr.max()
                clear = np.abs(ratio - mp) > 1e-6 * mp
                assert np.array_equal(r.kept[clear], (ratio >= mp)[clear])


def test_the_cut_is_order_independent_with_respect_to_top_k():
    """min-p after top-k (HF's order) keeps exactly the intersection: the ratio test does not see the renormalisation."""
    for V in (65, 4097):
        for x in rows(V, 3, 30 + V):
            for k in (1, 3, 40):
                for temp, mp in MIN_P_CASES:
                    both = filter_row_edit(x, temp, k, 1.0, mp)
                    assert np.array_equal(both.kept, filter_row(x, temp, k).kept & filter_row_edit(x, temp, 0, 1.0, mp).kept)


def test_edit_row_contract():
    x = np.array([0.5, -0.0, np.nan, -np.inf, 1e-45, 1e30, -1e30, 2.0], np.float32)
    assert same_bits(edit_row(x), x)  # nothing on: untouched, bit for bit
    y = edit_row(x, bias={0: 1.25, 5: 1e30, 7: -3.0}, banned=[1])
    assert y[0] == np.float32(1.75) and y[5] == np.float32(2e30) and y[7] == np.float32(-1.0) and y[1] == -np.inf
    assert same_bits(y[[2, 3, 4, 6]], x[[2, 3, 4, 6]])
    # a bias on a masked token leaves it -inf, whichever list masks it
    assert edit_row(x, bias={7: 100.0}, banned=[7])[7] == -np.inf
    assert edit_row(x, bias={7: 100.0}, allowed=[0, 1])[7] == -np.inf
    z = edit_row(x, allowed=[0, 7, 4], banned=[7, 7])
    assert np.array_equal(np.isneginf(z), np.array([0, 1, 1, 1, 0, 1, 1, 1], bool))
    # the sum is float32's: 1e30 + 1 is 1e30
    assert edit_row(x, bias={5: 1.0})[5] == np.float32(1e30)


def test_the_library_computes_the_same_offset_bit_for_bit():
    from zig_gpt2_amd import _lib

    lib = _lib.load()
    extra = [(t, p) for t in (0.05, 0.7, 1.0, 2.5, 100.0) for p in (1e-30, 1e-6, 0.01, 0.25, float(np.nextafter(np.float32(1), np.float32(0))))]
    for temp, mp in MIN_P_CASES + extra:
        d = C.c_float()
        assert lib.zg_debug_min_p_offset(temp, mp, C.byref(d)) == 0, (temp, mp)
        want = min_p_offset(temp, mp)
        assert np.array([d.value], np.float32).view(np.uint32)[0] == np.array([want], np.float32).view(np.uint32)[0], (temp, mp, d.value, want)
        assert d.value < 0 or mp == 0.0
    d = C.c_float()
    assert lib.zg_debug_min_p_offset(0.8, 0.0, C.byref(d)) == 0 and d.value == -np.inf


def test_the_offset_refusals():
    from zig_gpt2_amd import _lib

    lib = _lib.load()
    d = C.c_float(7.0)
    for temp, mp in ((0.0, 0.1), (-1.0, 0.1), (float("nan"), 0.1), (0.8, -0.1), (0.8, 1.0), (0.8, 1.5), (0.8, float("nan"))):
        assert lib.zg_debug_min_p_offset(temp, mp, C.byref(d)) == -6 and d.value == 7.0, (temp, mp)  # ZG_ERR_ARG, the output untouched
    assert lib.zg_debug_min_p_offset(0.8, 0.1, None) == -6
