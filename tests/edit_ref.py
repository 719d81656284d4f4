"""NumPy restatement of the logit edits and of min-p (include/zgpt2.h zg_logit_edits), shared by the test_*edit*.py files: the row
edit in float32, bitwise the contract; the min-p offset as the header computes it; the truncated sampler of trunc_ref.filter_row
followed by the min-p cut.  Applied to the caller's logits or to the device's own raw logits, never to the device's output."""
import ctypes as C
import math

import numpy as np

from trunc_ref import filter_row


# every (temp, min_p) pair the GPU tests run: test_edit_ref_cpu.py pins the library's offset for each of them
MIN_P_CASES = [(0.8, 0.05), (0.3, 0.1), (1.7, 0.02), (1.0, 0.5), (0.8, 0.3), (0.8, 0.0)]


def edit_row(x, bias=None, allowed=None, banned=None):
    """y[i] = keep[i] ? (i biased ? x[i] + v : x[i]) : -inf, keep = (no allow-list or i allowed) and i not banned.  bias: {id: value}.
    One float32 add; kept, unbiased indices keep their bits."""
    x = np.ascontiguousarray(x, np.float32)
    V = x.size
    keep = np.ones(V, bool)
    if allowed is not None and len(allowed):
        keep[:] = False
        keep[np.asarray(allowed, np.int64)] = True
    if banned is not None and len(banned):
        keep[np.asarray(banned, np.int64)] = False
    y = x.copy()
    for i, v in (bias or {}).items():
        with np.errstate(all="ignore"):
            y[int(i)] = np.float32(x[int(i)]) + np.float32(v)
    y[~keep] = np.float32(-np.inf)
    assert y.dtype == np.float32
    return y


def min_p_offset(temp, min_p):
    """d = (float)((double)temp * log((double)min_p)), -inf when min_p == 0 — temp and min_p as the float32 values the call carries."""
    t, p = float(np.float32(temp)), float(np.float32(min_p))
    if p == 0.0:
        return np.float32(-np.inf)
    return np.float32(t * math.log(p))


def filter_row_edit(x, temp, top_k=0, top_p=1.0, min_p=0.0):
    """trunc_ref.filter_row, then the cut at tau_m = max + d (one float32 add) and the renormalisation.  Returns filter_row's
    object with kept, tau and probs updated."""
    r = filter_row(x, temp, top_k, top_p)
    if min_p == 0.0:
        return r
    x32 = np.asarray(x, np.float32) + np.float32(0.0)
    with np.errstate(all="ignore"):
        tau_m = np.float32(x32.max()) + min_p_offset(temp, min_p)
    tau = np.float32(max(r.tau, tau_m))
    r.tau = tau
    r.kept = x32 >= tau
    t = float(np.float32(temp))
    xd = x32.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(r.kept, np.exp(xd / t - xd.max() / t), 0.0)
    r.probs = w / w.sum()
    return r


def same_bits(got, want):
    """Bitwise equality of two float32 arrays, a NaN on one side matching any NaN on the other."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def edit_rows(lib, logits, temp, top_k, top_p, uniforms, bias=None, allowed=None, banned=None, min_p=0.0, want_probs=True, want_edited=True):
    """zg_debug_edit_rows; returns (rc, edited rows, tokens, probs, thresholds)."""
    from zig_gpt2_amd import _lib

    logits = np.ascontiguousarray(logits, np.float32)
    B, V = logits.shape
    u = np.ascontiguousarray(uniforms, np.float32)
    tok = np.zeros(B, np.uint64)
    edited = np.full((B, V), np.float32(123.0), np.float32) if want_edited else None
    probs = np.empty((B, V), np.float32) if want_probs else None
    thr = np.empty(B, np.float32)
    opt = _lib.SampleOptions(temp, top_k, top_p)
    e, keep = _lib.logit_edits(bias, allowed, banned, min_p)
    rc = lib.zg_debug_edit_rows(_lib.ptr(logits), B, V, C.addressof(opt), C.addressof(e), _lib.ptr(u), _lib.ptr(edited), _lib.ptr(tok), _lib.ptr(probs),
                                _lib.ptr(thr))
    del keep
    return rc, edited, tok, probs, thr
