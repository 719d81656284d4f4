"""NumPy restatement of the history-dependent bans (include/zgpt2.h zg_ban_rules), shared by the test_ban_*.py and
test_generate_banned_gpu.py files: the set of tokens forbidden at one column, written from the header's text index by index, the
row the ban stage (and the edit stage behind it, through edit_ref.edit_row) leaves, and the wrappers of the two debug entries.
Applied to the caller's history and logits, never to the device's output.  Does not import zig_gpt2_amd.bans: that is the host
twin this file is the yardstick for."""
import ctypes as C

import numpy as np

from edit_ref import edit_row

MAX_NGRAM, MAX_WORDS, MAX_WORD_LEN, MAX_SUPPRESS = 16, 64, 16, 16


def ban_set(history, picked, n=0, words=(), min_tokens=0, suppress=(), vocab=None):
    """The sorted ids banned for a row with history h[0 .. L) and `picked` picks behind it.  vocab: a history token >= vocab matches
    nothing and bans nothing (None: every token counts)."""
    h = np.asarray(history, np.int64).reshape(-1)
    L = h.size
    ok = np.ones(L, bool) if vocab is None else (h >= 0) & (h < vocab)
    out = set()
    if n >= 1 and L >= n - 1:
        for i in range(0, L - n + 1):  # i = 0 .. L - n
            same = all(h[i + j] == h[L - n + 1 + j] and ok[i + j] for j in range(n - 1))
            if same and ok[i + n - 1]:
                out.add(int(h[i + n - 1]))
    for w in words:
        w = np.asarray(w, np.int64).reshape(-1)
        m = w.size
        assert m >= 1
        if L >= m - 1 and all(h[L - m + 1 + j] == w[j] for j in range(m - 1)):
            out.add(int(w[m - 1]))
    if 0 <= picked < min_tokens:
        out.update(int(t) for t in suppress)
    return sorted(out)


def ngram_bans_by_dict(history, n):
    """HF's way (NoRepeatNGramLogitsProcessor): every n-gram of the history into a dict prefix -> continuations, then the
    continuations of the last n - 1 tokens.  The independent brute force ban_set's n-gram rule is held against."""
    h = [int(t) for t in history]
    if n == 0 or len(h) + 1 < n:
        return []
    grams = {}
    for i in range(len(h) - n + 1):
        grams.setdefault(tuple(h[i: i + n - 1]), []).append(h[i + n - 1])
    return sorted(set(grams.get(tuple(h[len(h) - n + 1:]) if n > 1 else (), [])))


def ban_row(x, banned_now, bias=None, allowed=None, banned=None):
    """The row behind the ban stage and (any of the three lists given) the edit stage: -inf at every id of banned_now, then
    edit_ref.edit_row.  A row with nothing banned and no edits is returned as it came, bit for bit."""
    y = np.ascontiguousarray(x, np.float32).copy()
    if len(banned_now):
        y[np.asarray(banned_now, np.int64)] = np.float32(-np.inf)
    if bias is None and allowed is None and banned is None:
        return y
    return edit_row(y, bias, allowed, banned)


def rules_struct(batch, n=0, words=None, min_tokens=0, suppress=None):
    """(zg_ban_rules, the arrays it points into) through the package's own builder."""
    from zig_gpt2_amd import _lib

    return _lib.ban_rules(batch, n, words, min_tokens, suppress)


def ban_check(lib, batch, vocab, context, n=0, words=None, min_tokens=0, suppress=None, n_steps=1, prior_lens=None, greedy=False, guided=False,
              bias=None, allowed=None, banned=None, patch=None):
    """zg_debug_ban_check: the refusal of a call, or 0.  patch(rules): a last change to the structure (a wrong size, a null array)."""
    from zig_gpt2_amd import _lib

    r, keep_r = rules_struct(batch, n, words, min_tokens, suppress)
    if patch:
        patch(r)
    e, keep_e = (None, ()) if bias is None and allowed is None and banned is None else _lib.logit_edits(bias, allowed, banned, 0.0)
    pl = None if prior_lens is None else np.ascontiguousarray(prior_lens, np.uint64)
    rc = lib.zg_debug_ban_check(C.addressof(r), batch, vocab, context, None if e is None else C.addressof(e), n_steps, _lib.ptr(pl), int(greedy), int(guided))
    del keep_r, keep_e
    return rc


def ban_rows(lib, logits, histories, picked, n=0, words=None, min_tokens=0, suppress=None, bias=None, allowed=None, banned=None):
    """zg_debug_ban_rows; returns (rc, the rows as the stages leave them, part_val, part_idx)."""
    from zig_gpt2_amd import _lib

    logits = np.ascontiguousarray(logits, np.float32)
    B, V = logits.shape
    n_part = min(64, (V + 255) // 256)
    lens = np.array([len(h) for h in histories], np.uint64)
    stride = max(int(lens.max()), 1)
    hist = np.zeros((B, stride), np.uint64)
    for b, h in enumerate(histories):
        hist[b, : len(h)] = h
    pk = np.ascontiguousarray(picked, np.int64)
    r, keep_r = rules_struct(B, n, words, min_tokens, suppress)
    e, keep_e = (None, ()) if bias is None and allowed is None and banned is None else _lib.logit_edits(bias, allowed, banned, 0.0)
    edited = np.full((B, V), np.float32(123.0), np.float32)
    pv = np.zeros((B, n_part), np.float32)
    pi = np.zeros((B, n_part), np.int32)
    rc = lib.zg_debug_ban_rows(_lib.ptr(logits), B, V, C.addressof(r), _lib.ptr(hist), stride, _lib.ptr(lens), _lib.ptr(pk),
                               None if e is None else C.addressof(e), _lib.ptr(edited), _lib.ptr(pv), _lib.ptr(pi))
    del keep_r, keep_e
    return rc, edited, pv, pi
