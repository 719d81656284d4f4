"""NumPy float32 restatement of the logit penalties (include/zgpt2.h zg_logit_penalties), shared by the test_*pen*_gpu.py files:
the operations in the order the header gives, each rounded to float32 on its own, integer counts by np.bincount.  Applied to the
caller's logits or to logits read back from the device before the penalty stage, never to its output."""
import ctypes as C

import numpy as np


def penalize_row(x, history, repetition=1.0, presence=0.0, frequency=0.0):
    """One row x [V] and its history (token ids, any order) -> (penalised row float32 [V], counts uint32 [V])."""
    x = np.ascontiguousarray(x, np.float32)
    c = np.bincount(np.asarray(history, np.int64).reshape(-1), minlength=x.size).astype(np.uint32)
    r, p, f = np.float32(repetition), np.float32(presence), np.float32(frequency)
    with np.errstate(all="ignore"):
        y = np.where(x > 0, x / r, x * r)           # float32 / float32 and float32 * float32: -0.0, +0.0, negatives and NaN multiply
        off = p + f * c.astype(np.float32)          # one product, one sum
        out = np.where(c > 0, y - off, x)
    assert y.dtype == np.float32 and off.dtype == np.float32
    return out.astype(np.float32), c


def pack(histories):
    """Lists of token ids, one per row -> (uint64 [rows, stride >= 1], uint64 lengths [rows], stride)."""
    hs = [np.asarray(h, np.uint64).reshape(-1) for h in histories]
    stride = max(1, max(len(h) for h in hs))
    mat = np.zeros((len(hs), stride), np.uint64)
    for b, h in enumerate(hs):
        mat[b, : len(h)] = h
    return mat, np.array([len(h) for h in hs], np.uint64), stride


def penalize_rows(lib, logits, histories, repetition, presence, frequency, want_counts=True):
    """zg_debug_penalize_rows; returns (rc, penalised rows, counts)."""
    from zig_gpt2_amd import _lib

    logits = np.ascontiguousarray(logits, np.float32)
    B, V = logits.shape
    mat, lens, stride = pack(histories)
    pen = _lib.LogitPenalties(repetition, presence, frequency)
    out = np.full((B, V), np.float32(123.0), np.float32)
    counts = np.full((B, V), 0xFFFFFFFF, np.uint32) if want_counts else None
    rc = lib.zg_debug_penalize_rows(_lib.ptr(logits), B, V, C.addressof(pen), _lib.ptr(mat), stride, _lib.ptr(lens), _lib.ptr(out), _lib.ptr(counts))
    return rc, out, counts


def same_bits(got, want):
    """Bitwise equality of two float32 arrays, a NaN on one side matching any NaN on the other."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
