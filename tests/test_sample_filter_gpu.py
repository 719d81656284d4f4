"""Top-k / nucleus truncation in the device sampler, the kernels alone (zg_debug_sample_rows: the caller's logits) against the
float64 restatement of the semantics in trunc_ref.py.  Selection is comparison only: the kept set (probs != 0) and the
threshold must equal the reference EXACTLY; probabilities under golden_io.assert_model_close, summing to 1 within 1e-5, exact 0
outside the set; 32 draws per row equal the reference weightedIndex except where u x total lies within 1e-6 of a boundary of
the reference running sum (at most max(2, n / 20) of them), and every drawn token is in the kept set.

Top-p cuts: top_p is the midpoint between two consecutive reference cumulative masses at tie-group positions 1, 2, ~sqrt(V) and
V - 1, and both neighbours must lie >= 1e-4 from it (asserted): fp32 sums over <= 50257 terms err around 1e-6.  That margin needs
the token at the cut to weigh >= 2e-4, so the rows of these cases are N(0, sigma) with the widest sigma of a fixed list (and the
first of a few seeds) at which it holds, chosen here on the CPU.  A cut at position V - 1 needs ALL V tokens >= 2e-4, which no
distribution over more than 5000 tokens has: at V = 50257 the deepest cut is ~sqrt(V)."""
import numpy as np
import pytest

from golden_io import assert_model_close
from trunc_ref import filter_row, sample_rows, weighted_index

pytestmark = pytest.mark.gpu
VOCABS = [1, 2, 63, 64, 65, 257, 4097, 50257]
U_EDGE = np.array([0.0, np.nextafter(np.float32(1.0), np.float32(0.0))], np.float32)


def uniforms(rng, n=32):
    return np.concatenate([U_EDGE, rng.random(n - 2).astype(np.float32)]).astype(np.float32)


def rows_for(V, B, rng, kind, k=0):
    if kind == "normal":
        return (3.0 * rng.standard_normal((B, V))).astype(np.float32)
    if kind == "equal":
        return np.full((B, V), np.float32(rng.standard_normal()), np.float32)
    if kind == "straddle":  # the k-th value duplicated across the cut: up to 5 copies around rank k
        x = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
        for b in range(B):
            order = np.argsort(-x[b], kind="stable")
            kk = min(max(k, 1), V)
            lo, hi = max(0, kk - 3), min(V, kk + 2)
            x[b, order[lo:hi]] = x[b, order[kk - 1]]
        return x
    if kind == "mixed":
        pool = np.array([0.0, -0.0, -np.inf, 1e-45, -1e-45, 1e-40, 1e30, -1e30, 1.5, -1.5, 3.0, 2.0], np.float32)
        x = pool[rng.integers(0, pool.size, (B, V))]
        x[:, rng.integers(0, V)] = np.float32(4.0)  # (a finite top token: a row of -inf alone has no distribution)
        return x
    if kind == "asc":
        return np.sort((3.0 * rng.standard_normal((B, V))).astype(np.float32), axis=1)
    if kind == "desc":
        return -np.sort(-(3.0 * rng.standard_normal((B, V))).astype(np.float32), axis=1)
    raise ValueError(kind)


def check(zg, x, temp, top_k, top_p, rng, what, n_u=32):
    B, V = x.shape
    refs = [filter_row(x[b], temp, top_k, top_p) for b in range(B)]
    us = np.stack([uniforms(rng, n_u) for _ in range(B)], axis=1)  # [n_u, B]
    rc, tok, probs, thr = sample_rows(zg, x, temp, top_k, top_p, us[0])
    assert rc == 0, what
    rc2, tok2, probs2, thr2 = sample_rows(zg, x, temp, top_k, top_p, us[0])  # a second identical call: identical results
    assert rc2 == 0 and np.array_equal(tok, tok2) and np.array_equal(thr.view(np.uint32), thr2.view(np.uint32)) and np.array_equal(
        probs.view(np.uint32), probs2.view(np.uint32)), what
    near = 0
    for b, r in enumerate(refs):
        got_kept = probs[b] != 0
        # (a kept token may weigh less than fp32's smallest value: it is then 0 on both sides)
        tiny = r.kept & (r.probs < 1e-37)
        assert np.array_equal(got_kept | tiny, r.kept), (what, b, np.flatnonzero((got_kept | tiny) != r.kept)[:5], thr[b], r.tau)
        if top_k or top_p < 1.0:
            assert thr[b:b + 1].view(np.uint32)[0] == np.array([r.tau], np.float32).view(np.uint32)[0], (what, b, thr[b], r.tau)
        assert (probs[b][~r.kept] == 0.0).all(), what
        assert_model_close(r.probs, probs[b], what + f" probs row {b}")
        assert abs(float(probs[b].sum(dtype=np.float64)) - 1.0) < 1e-5, what
    toks = [tok] + [sample_rows(zg, x, temp, top_k, top_p, us[i], want_probs=False)[1] for i in range(1, n_u)]
    for i in range(n_u):
        for b, r in enumerate(refs):
            t = int(toks[i][b])
            assert t < V and r.kept[t], (what, "drawn token outside the kept set", i, b, t)
            exp, dist = weighted_index(r.probs, us[i][b])
            if t != exp:
                assert dist < 1e-6, (what, i, b, t, exp, float(us[i][b]))
                near += 1
    assert near <= max(2, n_u * B // 20), (what, near)


def ks_for(V):
    return sorted({k for k in (1, 2, 7, 64, V - 1, V, V + 5, 0) if k >= 0})


@pytest.mark.parametrize("V", VOCABS)
def test_top_k_kept_set_threshold_probabilities_and_draws(zg, V):
    rng = np.random.default_rng(7000 + V)
    if V == 50257:  # the real vocabulary: every k on normal rows at one batch each, every row kind at k = 7 (3 rows) and V - 1 (1 row)
        for j, k in enumerate(ks_for(V)):
            B = (1, 3, 8)[j % 3]
            check(zg, rows_for(V, B, rng, "normal"), 0.8, k, 1.0, rng, f"V {V} B {B} k {k} normal")
        for k, B in ((7, 3), (V - 1, 1)):
            for kind in ("equal", "straddle", "mixed", "asc", "desc"):
                check(zg, rows_for(V, B, rng, kind, k), 0.8, k, 1.0, rng, f"V {V} B {B} k {k} {kind}")
        return
    for B in (1, 3, 8):
        for k in ks_for(V):
            for kind in ("normal", "equal", "straddle", "mixed", "asc", "desc"):
                x = rows_for(V, B, rng, kind, k)
                if not 0 < k < V:  # filters off is the plain sampler, whose x / temp - max / temp does not carry 1e30 (its own, older, limit)
                    x = np.where(np.abs(x) == np.float32(1e30), np.sign(x) * np.float32(30.0), x).astype(np.float32)
                check(zg, x, 0.8, k, 1.0, rng, f"V {V} B {B} k {k} {kind}")


def nucleus_case(V, temp, cut, seed0):
    """A row and the top_p that cuts it behind tie group `cut` (1-based) with the 1e-4 margin, or top_p below the top token (cut 0)."""
    for sigma in (3.0, 1.0, 0.3, 0.1, 0.03, 0.01):
        for seed in range(seed0, seed0 + 4):
            x = (sigma * temp * np.random.default_rng(seed).standard_normal(V)).astype(np.float32)
            r = filter_row(x, temp)
            if cut == 0:
                p = r.cum[0] / 2
                lo, hi = 0.0, r.cum[0]
            elif cut >= len(r.cum):
                continue
            else:
                lo, hi = r.cum[cut - 1], r.cum[cut]
                p = (lo + hi) / 2
            p32 = float(np.float32(p))
            if 0 < p32 < 1 and p32 - lo >= 1e-4 and hi - p32 >= 1e-4:
                return x, p32, (lo, hi)
    raise AssertionError(f"no row with the 1e-4 margin for V {V} temp {temp} cut {cut}")


@pytest.mark.parametrize("V", VOCABS)
def test_top_p_cuts_between_reference_cumulative_masses(zg, V):
    rng = np.random.default_rng(8000 + V)
    root = max(3, int(round(np.sqrt(V))))
    cuts = [c for c in dict.fromkeys([0, 1, 2, root, V - 1]) if c < V and (c == 0 or V >= 2)]
    if V > 4097:
        cuts.remove(V - 1)  # (needs every token >= 2e-4: the module docstring)
    for temp in (0.3, 0.8, 1.7):
        for B in (1, 3, 8):
            for cut in cuts:
                rows, ps = [], []
                for b in range(B):
                    if b and V > 4097:  # (the wide rows: a rotation of row 0 — another row, the same masses — keeps the CPU side short)
                        rows.append(np.roll(rows[0], 1000 * b))
                        ps.append(ps[0])
                        continue
                    x, p, (lo, hi) = nucleus_case(V, temp, cut, 100 * V % 9973 + 10 * cut + 40 * b)
                    assert p - lo >= 1e-4 and hi - p >= 1e-4  # the precondition
                    rows.append(x)
                    ps.append(p)
                # options are per call: rows of one call share top_p, so each row's own cut runs as its own call beside B - 1 others
                for b in range(B if V <= 4097 else 1):
                    x = np.stack(rows)
                    r = filter_row(x[b], temp, 0, ps[b])
                    assert int(r.kept.sum()) == (cut + 1 if cut else 1)  # (no ties in these rows: tie groups are tokens)
                    rc, tok, probs, thr = sample_rows(zg, x, temp, 0, ps[b], rng.random(B).astype(np.float32))
                    assert rc == 0
                    assert np.array_equal(probs[b] != 0, r.kept), (V, temp, B, cut, b, thr[b], r.tau)
                    assert thr[b:b + 1].view(np.uint32)[0] == np.array([r.tau], np.float32).view(np.uint32)[0]
            if V >= 2:  # draws, probabilities and the repeat call on one cut per temperature
                x, p, _ = nucleus_case(V, temp, cuts[min(2, len(cuts) - 1)], 77)
                check(zg, x[None, :], temp, 0, p, rng, f"V {V} temp {temp} top_p {p}")
        check(zg, rows_for(V, 3, rng, "normal"), temp, 0, 1.0, rng, f"V {V} temp {temp} top_p 1")


def test_top_p_applies_to_what_top_k_kept(zg):
    """Sequential order: the nucleus of the top-k-restricted distribution differs from the nucleus of the full one."""
    V, temp, k = 257, 0.8, 5
    x = np.full(V, -1.0, np.float32)
    x[[10, 20, 30, 40, 50]] = [2.0, 1.6, 1.2, 0.8, 0.4]
    full, restricted = filter_row(x, temp), filter_row(x, temp, k)
    p = float(np.float32((restricted.cum[1] + restricted.cum[2]) / 2))  # behind the 3rd token of the restricted distribution
    assert min(p - restricted.cum[1], restricted.cum[2] - p) >= 1e-4
    assert int(filter_row(x, temp, 0, p).kept.sum()) != int(filter_row(x, temp, k, p).kept.sum())  # the orders differ here
    assert min(abs(p - c) for c in full.cum) >= 1e-4
    rng = np.random.default_rng(5)
    check(zg, np.stack([x, x[::-1].copy(), np.roll(x, 7)]), temp, k, p, rng, "top-k then top-p")
    for V2 in (4097, 50257):  # and on wide rows: top-k 40, the nucleus cut behind 10 of them
        xs = []
        for b in range(3):
            xr = (3.0 * np.random.default_rng(900 + b + V2).standard_normal(V2)).astype(np.float32)
            xs.append(xr)
        r0 = filter_row(xs[0], 1.7, 40)
        p = float(np.float32((r0.cum[9] + r0.cum[10]) / 2))
        for xr in xs:
            rr = filter_row(xr, 1.7, 40)
            assert min(abs(p - c) for c in rr.cum) >= 1e-4
        check(zg, np.stack(xs), 1.7, 40, p, rng, f"V {V2} top-k 40 then top-p {p}")


def test_a_nan_row_returns_a_token_inside_the_vocabulary(zg):
    rng = np.random.default_rng(11)
    for V in (65, 4097, 50257):
        x = rows_for(V, 3, rng, "normal")
        x[1, V // 2] = np.nan
        for k, p in ((7, 1.0), (0, 0.9), (40, 0.95)):
            rc, tok, _, _ = sample_rows(zg, x, 0.8, k, p, rng.random(3).astype(np.float32))
            assert rc == 0 and (tok < V).all(), (V, k, p, tok)
    x = rows_for(257, 2, rng, "normal")  # the library is still sound afterwards
    check(zg, x, 0.8, 7, 1.0, rng, "after the NaN rows")


def test_filters_off_is_the_plain_sampler(zg):
    rng = np.random.default_rng(12)
    for V in (65, 4097, 50257):
        x = rows_for(V, 3, rng, "normal")
        check(zg, x, 0.8, 0, 1.0, rng, f"filters off V {V}")
        check(zg, x, 0.8, V + 5, 1.0, rng, f"top_k beyond the vocabulary V {V}")


def test_bad_options_are_refused(zg):
    import ctypes as C

    from zig_gpt2_amd import _lib

    x = np.zeros((1, 8), np.float32)
    for temp, p in ((0.0, 1.0), (-1.0, 1.0), (1.0, 0.0), (1.0, -0.5), (1.0, 1.5), (1.0, float("nan"))):
        assert sample_rows(zg, x, temp, 0, p, np.zeros(1, np.float32))[0] == -6, (temp, p)  # ZG_ERR_ARG
    tok, u = np.zeros(1, np.uint64), np.zeros(1, np.float32)
    assert zg.zg_debug_sample_rows(_lib.ptr(x), 1, 8, None, _lib.ptr(u), _lib.ptr(tok), None, None) == -6
