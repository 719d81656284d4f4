"""NumPy float64 restatement of the truncated sampler's semantics (include/zgpt2.h zg_sample_options), shared by
test_sample_filter_gpu.py, test_truncated_generate_gpu.py and sweeps/sample_trunc.py.  Applied to the caller's logits or to the
oracle's, never to the device's output."""
import ctypes as C

import numpy as np

M64 = (1 << 64) - 1


def uniform(seed, seq_len, b):
    """The library's counter PRNG of (seed, seq_len, b): what zg_gpt_sample(_ex) uses for uniforms == NULL."""
    z = (seed * 0x9E3779B97F4A7C15 + seq_len * 0xD1B54A32D192ED03 + b + 1) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return np.float32((z >> 40) & 0xFFFFFF) * np.float32(5.9604644775390625e-08)


class Filtered:
    """One row: kept (bool [V]), tau (float32; -inf when nothing is dropped by a filter that is on ... the threshold itself),
    probs (float64 [V], exact 0 where dropped), cum (descending cumulative masses of K by tie group, normalised), vals (their values)."""


def filter_row(x, temp, top_k=0, top_p=1.0):
    x = np.asarray(x, np.float32) + np.float32(0.0)  # -0.0 and +0.0 are one value; a zero threshold reads +0.0
    V = x.size
    xd = x.astype(np.float64)
    t = float(np.float32(temp))
    r = Filtered()
    tk = np.float32(-np.inf)
    if 0 < top_k < V:
        tk = np.sort(x)[V - top_k]  # the k-th largest, duplicates counted
    K = x >= tk
    mx = xd.max()
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.where(K, np.exp(xd / t - mx / t), 0.0)
    order = np.argsort(-xd[K], kind="stable")
    xs, es = x[K][order], e[K][order]
    cum = np.cumsum(es)
    last = np.r_[xs[1:] != xs[:-1], True]  # ends of the tie groups
    r.vals, r.cum = xs[last], cum[last] / cum[-1]
    tau = tk
    if top_p < 1.0:
        tp = r.vals[int(np.argmax(r.cum >= float(np.float32(top_p))))]  # the largest v whose mass reaches top_p of K's
        tau = max(tk, tp)
    r.tau = np.float32(tau)
    r.kept = x >= r.tau
    w = np.where(r.kept, e, 0.0)
    r.probs = w / w.sum()
    return r


def weighted_index(probs, u):
    """std.rand weightedIndex: the first index whose running sum exceeds u x total; also the distance of the point to the
    nearest boundary of the running sum."""
    cdf = np.cumsum(np.asarray(probs, np.float64))
    point = float(u) * cdf[-1]
    idx = int(np.searchsorted(cdf, point, side="right"))
    return min(idx, len(cdf) - 1), float(np.abs(cdf - point).min())


def sample_rows(lib, logits, temp, top_k, top_p, uniforms, want_probs=True):
    """zg_debug_sample_rows; returns (rc, tokens, probs, thresholds)."""
    from zig_gpt2_amd import _lib

    logits = np.ascontiguousarray(logits, np.float32)
    B, V = logits.shape
    u = np.ascontiguousarray(uniforms, np.float32)
    tok = np.zeros(B, np.uint64)
    probs = np.empty((B, V), np.float32) if want_probs else None
    thr = np.empty(B, np.float32)
    opt = _lib.SampleOptions(temp, top_k, top_p)
    rc = lib.zg_debug_sample_rows(_lib.ptr(logits), B, V, C.addressof(opt), _lib.ptr(u), _lib.ptr(tok), _lib.ptr(probs), _lib.ptr(thr))
    return rc, tok, probs, thr
