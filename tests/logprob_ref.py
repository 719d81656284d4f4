"""float64 restatement of the log-probability stage (include/zgpt2.h zg_gpt_generate_logprobs_enqueue), shared by the
test_*logprob*.py files.  For a row x of float32 logits, m = max x and S = sum exp(x_i - m):  logprob(i) = (x_i - m) - log S;  the
top-N are the N largest x, value descending, index ascending on ties (-0.0 and +0.0 tie, -inf is an ordinary value)."""
import numpy as np

TOP_MAX = 20    # ZG_LOGPROBS_TOP_MAX
CHUNK = 1024    # elements of a row per workgroup of logprob_part_kernel (the header's zg_debug_logprob_rows says so)


def logprob_all(x):
    """The log-probability of every index of one row, float64 [V]."""
    x = np.asarray(x, np.float32).astype(np.float64)
    m = x.max()
    with np.errstate(all="ignore"):
        return (x - m) - np.log(np.exp(x - m).sum())


def top_order(x, top_n):
    """Indices of the top_n largest values: value descending, index ascending on ties.  A stable sort of -x: numpy compares
    -0.0 == +0.0, and -(-inf) = +inf sorts last like any other value."""
    x = np.asarray(x, np.float32).astype(np.float64)
    return np.argsort(-x, kind="stable")[:top_n].astype(np.int64)


def logprob_ref(x, tok, top_n):
    """One row -> (logprob of tok float64, top_ids int64 [top_n], top_logprobs float64 [top_n])."""
    lp = logprob_all(x)
    ids = top_order(x, top_n)
    return lp[int(tok)], ids, lp[ids]


def bound(ref):
    """The tests' bound on |got - ref| for finite ref: fp32 errors of the expression, 1e-5 + 2.5e-7 |ref|."""
    return 1e-5 + 2.5e-7 * np.abs(ref)


def check_values(got, ref):
    """got float32 against ref float64: -inf exactly where ref is -inf, within the bound elsewhere.  Returns the largest
    |got - ref| / bound over the finite entries (0.0 when there are none)."""
    got = np.asarray(got, np.float32).astype(np.float64).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    ninf = np.isneginf(ref)
    assert np.array_equal(np.isneginf(got), ninf), "-inf entries differ"
    fin = ~ninf
    assert np.all(np.isfinite(got[fin])), got[fin][~np.isfinite(got[fin])][:4]
    if not fin.any():
        return 0.0
    ratio = np.abs(got[fin] - ref[fin]) / bound(ref[fin])
    worst = float(ratio.max())
    assert worst <= 1.0, (worst, got[fin][ratio.argmax()], ref[fin][ratio.argmax()])
    return worst
