"""NumPy restatement of guided decoding's stage (include/zgpt2.h zg_guide), shared by the test_guide_*.py and
test_generate_guided_gpu.py files: the mask on a row (with the edit stage's part, through edit_ref.edit_row), the rule the
row-maximum partials are rebuilt by, the advance behind a pick and the state record of a generation.  Applied to the caller's
logits, never to the device's output."""
import ctypes as C

import numpy as np

from edit_ref import edit_row

DEAD = 0xFFFF
NONE = (1 << 64) - 1
START_VAL = np.float32(-3.0e38)   # where a slice maximum starts: below every finite logit
START_IDX = 0x7FFFFFFF            # ... and the index of a slice that holds nothing comparable


def mask_row(x, next, state, bias=None, allowed=None, banned=None):
    """y[i] = keep[i] ? (i biased ? x[i] + v : x[i]) : -inf with keep = the call's keep set AND (state is NONE or next[state][i] is a
    state).  A kept, unbiased index keeps its bits; a row with neither a guide nor edits is returned as it came."""
    y = edit_row(x, bias, allowed, banned)
    if state != NONE:
        y[np.asarray(next)[state] == DEAD] = np.float32(-np.inf)
    return y


def slice_partials(y, n_part):
    """The partials of one row as the stage leaves them: slice j = the indices i with (i // 256) % n_part == j; its value the
    largest element that compares (NaN never does), never below START_VAL; its index the lowest one holding that value, START_IDX
    where none does."""
    y = np.ascontiguousarray(y, np.float32)
    owner = (np.arange(y.size) // 256) % n_part
    val = np.full(n_part, START_VAL, np.float32)
    idx = np.full(n_part, START_IDX, np.int32)
    for j in range(n_part):
        ids = np.flatnonzero(owner == j)
        v = y[ids]
        ok = ~np.isnan(v)
        if ok.any():
            val[j] = max(START_VAL, v[ok].max())
        hit = ids[v == val[j]]
        if hit.size:
            idx[j] = hit[0]
    return val, idx


def advance(next, state, tok):
    """The state behind the pick: unchanged for a row without a guide, for a pick outside the vocabulary and for a transition that
    is dead or out of range."""
    next = np.asarray(next)
    if state == NONE or not 0 <= tok < next.shape[1]:
        return state
    nx = int(next[state, tok])
    return nx if nx < next.shape[0] else state


def record(next, start_states, tokens, first_cols):
    """The state record of a generation: tokens [batch][n] (absolute columns 0 .. n - 1), first_cols[b] the first picked column of
    row b.  Returns (record [batch][n] of uint64 — the state each picked column was drawn in, NONE elsewhere —, the state behind
    the last column)."""
    tokens = np.asarray(tokens)
    B, n = tokens.shape
    rec = np.full((B, n), NONE, np.uint64)
    end = []
    for b in range(B):
        st = start_states[b]
        for p in range(int(first_cols[b]), n):
            if st != NONE:
                rec[b, p] = st
                st = advance(next, st, int(tokens[b, p]))
        end.append(st)
    return rec, end


def guide_struct(next):
    """(zg_guide over a uint16 table, the table: keep it alive while the structure is in use)"""
    from zig_gpt2_amd import _lib

    t = np.ascontiguousarray(next, np.uint16)
    return _lib.Guide(t.shape[0], _lib.ptr(t)), t


def guide_rows(lib, logits, next, states, picks, bias=None, allowed=None, banned=None):
    """zg_debug_guide_rows; returns (rc, edited rows, part_val, part_idx, next states)."""
    from zig_gpt2_amd import _lib

    logits = np.ascontiguousarray(logits, np.float32)
    B, V = logits.shape
    n_part = min(64, (V + 255) // 256)
    g, keep_g = guide_struct(next)
    st = np.ascontiguousarray(states, np.uint64)
    pk = np.ascontiguousarray(picks, np.uint64)
    edited = np.full((B, V), np.float32(123.0), np.float32)
    pv = np.zeros((B, n_part), np.float32)
    pi = np.zeros((B, n_part), np.int32)
    out = np.zeros(B, np.uint64)
    e, keep_e = (None, ()) if bias is None and allowed is None and banned is None else _lib.logit_edits(bias, allowed, banned, 0.0)
    rc = lib.zg_debug_guide_rows(_lib.ptr(logits), B, V, C.addressof(g), _lib.ptr(st), None if e is None else C.addressof(e), _lib.ptr(pk), _lib.ptr(edited),
                                 _lib.ptr(pv), _lib.ptr(pi), _lib.ptr(out))
    del keep_g, keep_e
    return rc, edited, pv, pi, out


def guide_check(lib, next, vocab, start_states=None, greedy=False, bias=None, allowed=None, banned=None, n_states=None, null_table=False):
    """zg_debug_guide_check: the refusal of a load (and, with start_states, of a call), or 0."""
    from zig_gpt2_amd import _lib

    g, keep_g = guide_struct(next)
    if n_states is not None:
        g.n_states = n_states
    if null_table:
        g.next = None
    st = None if start_states is None else np.ascontiguousarray(start_states, np.uint64)
    e, keep_e = (None, ()) if bias is None and allowed is None and banned is None else _lib.logit_edits(bias, allowed, banned, 0.0)
    rc = lib.zg_debug_guide_check(C.addressof(g), vocab, None if e is None else C.addressof(e), _lib.ptr(st), 0 if st is None else st.size, int(greedy))
    del keep_g, keep_e
    return rc
