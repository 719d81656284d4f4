"""zg_debug_ban_rows on a real MI355X: the ban launch (sample_ban.h) and the rebuild of the row-maximum partials — or the edit launch
— behind it, against tests/ban_ref.py and tests/edit_ref.py, bitwise.

Vocabularies of 257 (two slices) and 50257 (64 slices); 1, 3 and 8 rows; n in {1, 2, 3, 16}; histories of 0, n - 2, n - 1, n, 255,
256, 257 and 8192 tokens over a small alphabet (so that n-grams do repeat: a period of 20 tokens gives every 16-gram its twin),
with a token outside the vocabulary among them; words of 1 and 16 tokens; picked at min - 1, min and on a prompt column.  Then a
banned token that is the row maximum in the first and in the last slice (ties behind it: the lowest index), a row with every rule
off between two active rows, and the edit stage behind the bans."""
import numpy as np
import pytest

from ban_ref import ban_row, ban_rows, ban_set
from guide_ref import slice_partials

pytestmark = pytest.mark.gpu
NS = [1, 2, 3, 16]
W16 = [3, 9, 4, 11, 2, 8, 6, 1, 12, 5, 10, 7, 13, 0, 14, 33]  # a word of 16 tokens; its last one is banned behind the first 15
WORDS = [[5], W16, [2, 8, 21]]
SUPPRESS = [0, 40, 41]
MIN = 4


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lengths(n):
    return sorted({L for L in (0, n - 2, n - 1, n, 255, 256, 257, 8192) if L >= 0})


def history(rng, L, V, with_word):
    """L tokens of period 20 over an alphabet of 15 (every n-gram up to 16 recurs), one token outside the vocabulary in the
    middle of the longer ones, and — with_word — the first 15 tokens of W16 at the end."""
    period = rng.integers(0, 15, 20)
    h = np.resize(period, L).astype(np.int64)
    if L >= 64:
        h[L // 2] = V + 5
    if with_word and L >= 15:
        h[L - 15:] = W16[:15]
    return h


def check_rows(zg, x, hists, picked, n, words, min_tokens, suppress, **edits):
    B, V = x.shape
    rc, got, pv, pi = ban_rows(zg, x, hists, picked, n, words, min_tokens, suppress, **edits)
    assert rc == 0, zg.zg_last_error()
    n_part = pv.shape[1]
    ns = np.broadcast_to(np.asarray(n), (B,))
    mts = np.broadcast_to(np.asarray(min_tokens), (B,))
    sets = []
    for b in range(B):
        now = ban_set(hists[b], int(picked[b]), int(ns[b]), words or (), int(mts[b]), suppress or (), vocab=V)
        want = ban_row(x[b], now, **edits)
        bad = np.flatnonzero(u32(got[b]) != u32(want))
        assert bad.size == 0, (b, len(hists[b]), int(ns[b]), bad[:5], got[b][bad[:5]], want[bad[:5]])
        wv, wi = slice_partials(want, n_part)
        assert np.array_equal(u32(pv[b]), u32(wv)), (b, "part_val", np.flatnonzero(pv[b] != wv)[:5])
        assert np.array_equal(pi[b], wi), (b, "part_idx", np.flatnonzero(pi[b] != wi)[:5])
        sets.append(now)
    return got, sets


@pytest.mark.parametrize("V", [257, 50257])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_every_rule_at_every_history_length(zg, V, B):
    rng = np.random.default_rng(31 * B + V)
    x = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    hit = 0
    for n in NS:
        Ls = lengths(n)
        for shift in range(0, len(Ls), B):  # every length of the set in some row
            row_L = [Ls[(shift + b) % len(Ls)] for b in range(B)]
            hists = [history(rng, L, V, with_word=(b + shift) % 2 == 0) for b, L in enumerate(row_L)]
            picked = [(MIN - 1, MIN, -1, 0)[(b + shift) % 4] for b in range(B)]
            _, sets = check_rows(zg, x, hists, picked, n, WORDS, MIN, SUPPRESS)
            hit += sum(len(s) > 1 for s in sets)  # (more than the one-token word alone)
    assert hit >= 8, "the cases ban something"


@pytest.mark.parametrize("V,first,last", [(257, 7, 256), (50257, 7, 16200)])
def test_a_banned_row_maximum_in_the_first_and_in_the_last_slice(zg, V, first, last):
    """n = 1 bans the two largest elements of the row; the partials of both slices fall back to a tie, whose lowest index wins."""
    B = 3
    rng = np.random.default_rng(V)
    x = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    n_part = min(64, (V + 255) // 256)
    assert (first // 256) % n_part == 0 and (last // 256) % n_part == n_part - 1
    x[:, first], x[:, last] = 50.0, 49.0
    x[:, [10, 20]] = 40.0                 # slice 0: the tie behind the banned maximum
    tie = [last - 1, last - 2] if V > 257 else []
    x[:, tie] = 39.0                      # the last slice of the large vocabulary likewise (of 257 it holds one token: left empty)
    hists = [[first, 3, last, 3], [3, first], [last]]
    rc, got, pv, pi = ban_rows(zg, x, hists, [0, 0, 0], 1)
    assert rc == 0, zg.zg_last_error()
    for b in range(B):
        want = ban_row(x[b], ban_set(hists[b], 0, 1, vocab=V))
        assert np.array_equal(u32(got[b]), u32(want))
        wv, wi = slice_partials(want, n_part)
        assert np.array_equal(u32(pv[b]), u32(wv)) and np.array_equal(pi[b], wi), b
    assert np.isneginf(got[0][[first, last]]).all() and pi[0][0] == 10 and pv[0][0] == 40.0
    assert pi[1][0] == 10 and pv[1][n_part - 1] == 49.0 and pi[1][n_part - 1] == last, "row 1 keeps its last-slice maximum"
    assert pv[2][0] == 50.0 and pi[2][0] == first
    if V > 257:
        assert pi[0][n_part - 1] == last - 2 and pv[2][n_part - 1] == 39.0


@pytest.mark.parametrize("V", [257, 50257])
def test_a_row_with_every_rule_off_keeps_its_bits_between_active_rows(zg, V):
    B = 3
    rng = np.random.default_rng(5 + V)
    x = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    bits = x[1].view(np.uint32)
    bits[[5, 300 % V, V - 1]] = [0x7FC12345, 0xFFC00001, 0x80000000]  # NaN payloads and -0.0
    x[1, 256 % V] = np.float32(-0.0)
    before = x[1].view(np.uint32).copy()
    hists = [[5, 6, 5, 6, 5], [5, 6, 5, 6, 5], [V - 1, 5, V - 1]]
    # row 1: n 0, min_tokens 0 and no words in the call: nothing applies to it — its neighbours are banned 5 / 6 / the suppress ids
    got, sets = check_rows(zg, x, hists, [0, 0, 1], [3, 0, 2], None, [2, 0, 2], [V - 1, 300 % V])
    assert np.array_equal(got[1].view(np.uint32), before), "bit-identical on exit"
    assert sets[1] == [] and len(sets[0]) >= 2 and len(sets[2]) >= 2
    # and at a column where its only rule does not apply (picked past min_tokens; picked on a prompt column)
    for picked in (2, -1):
        got, sets = check_rows(zg, x, hists, [0, picked, 1], [3, 0, 2], None, [2, 2, 2], [V - 1, 5])
        assert np.array_equal(got[1].view(np.uint32), before) and sets[1] == []


@pytest.mark.parametrize("V", [257, 50257])
def test_the_edit_stage_behind_the_bans(zg, V):
    B = 3
    rng = np.random.default_rng(9 + V)
    x = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    hists = [[7, 3, 7, 3, 7], [7, 3, 5, 7], [11, 12, 11]]
    # a +1e4 bias on token 3, which rows 0 and 1 ban (n = 2: the follower of 7): it stays -inf there and is row 2's maximum
    got, sets = check_rows(zg, x, hists, [0, 0, 0], 2, [[9]], 0, None, bias={3: 1e4, 20: -2.5}, banned=[21])
    assert 3 in sets[0] and 3 in sets[1] and 3 not in sets[2]
    assert np.isneginf(got[0][3]) and np.isneginf(got[1][3]) and got[2][3] > 9000.0 and np.isneginf(got[:, [9, 21]]).all()
    # an allow-list beside the bans: the kept set is the allow-list minus what the history bans
    allowed = sorted(set(range(0, V, 3)) | {7, 12})
    got, sets = check_rows(zg, x, hists, [0, 0, 0], 2, [[9]], 0, None, allowed=allowed)
    keep0 = sorted(set(allowed) - set(sets[0]))
    assert np.array_equal(np.flatnonzero(~np.isneginf(got[0])), keep0)
    assert 12 in sets[2] and np.isneginf(got[2][12]) and not np.isneginf(got[0][12])
