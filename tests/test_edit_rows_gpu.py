"""Logit bias, allow / ban lists and min-p, the kernels alone (zg_debug_edit_rows: the caller's rows) against edit_ref.py.

The edited row equals edit_ref.edit_row bit for bit.  Behind it the sampler is held the way test_sample_filter_gpu.check holds it,
against edit_ref.filter_row_edit of the reference's edited row: kept set and threshold exact; probabilities under
golden_io.assert_model_close, summing to 1 within 1e-5, exact 0 outside the set; draws equal the reference weightedIndex except
where u x total lies within 1e-6 of a boundary of the reference running sum.  At most max(2, n / 20) draws may lie that near: that
is a condition on the uniforms, met by choosing their seed on the CPU before the device is asked (the two edge uniforms of every
row, 0 and the largest float below 1, always may: hence 40 draws per row, whose allowance is exactly those).  min-p's cut is one float32
comparison on both sides and needs no margin; the top-p cuts run beside it carry test_sample_filter_gpu's 1e-4 margin."""
import ctypes as C

import numpy as np
import pytest

from edit_ref import MIN_P_CASES, edit_row, edit_rows, filter_row_edit, same_bits
from golden_io import assert_model_close
from test_sample_filter_gpu import nucleus_case, rows_for, uniforms
from trunc_ref import filter_row, sample_rows, weighted_index
from zig_gpt2_amd import _lib

pytestmark = pytest.mark.gpu
VOCABS = [1, 2, 63, 64, 65, 257, 4097, 50257]
ARG, SHAPE = -6, -2


def batches(V):
    return (1, 3, 8) if V <= 4097 else (1, 3)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pick_uniforms(refs, n_u, seed):
    """[n_u, B] uniforms (test_sample_filter_gpu.uniforms per row) for which at most max(2, n_u B / 20) reference draws lie within 1e-6
    of a boundary: the first of a few seeds that meets the condition."""
    B = len(refs)
    for s in range(seed, seed + 50):
        rng = np.random.default_rng(s)
        us = np.stack([uniforms(rng, n_u) for _ in range(B)], axis=1)
        near = sum(weighted_index(r.probs, us[i][b])[1] < 1e-6 for i in range(n_u) for b, r in enumerate(refs))
        if near <= max(2, n_u * B // 20):
            return us
    raise AssertionError("no seed meets the near-boundary condition")


def check(zg, x, temp, top_k, top_p, min_p, what, bias=None, allowed=None, banned=None, n_u=40, seed=1):
    """zg: the library (zg_debug_edit_rows runs on x), or a callable with edit_rows' arguments behind the library and its
    results — a model's per-token call, which returns neither the edited row nor the threshold (None: not compared here; the kept
    set, which the threshold decides, is)."""
    B, V = x.shape
    edit_rows = globals()["edit_rows"] if not callable(zg) else (lambda _zg, *a, **k: zg(*a, **k))
    y = np.stack([edit_row(x[b], bias, allowed, banned) for b in range(B)])
    refs = [filter_row_edit(y[b], temp, top_k, top_p, min_p) for b in range(B)]
    us = pick_uniforms(refs, n_u, seed)
    kw = dict(bias=bias, allowed=allowed, banned=banned, min_p=min_p)
    rc, ed, tok, probs, thr = edit_rows(zg, x, temp, top_k, top_p, us[0], **kw)
    assert rc == 0, what
    rc2, ed2, tok2, probs2, thr2 = edit_rows(zg, x, temp, top_k, top_p, us[0], **kw)  # a second identical call: identical bits
    assert rc2 == 0 and np.array_equal(tok, tok2) and np.array_equal(bits(probs), bits(probs2)), what
    assert thr is None or np.array_equal(bits(thr), bits(thr2)), what
    assert ed is None or (same_bits(ed, ed2) and same_bits(ed, y)), (what, np.flatnonzero(bits(ed) != bits(y))[:5])
    truncating = 0 < top_k < V or top_p < 1.0 or min_p > 0.0
    near = 0
    for b, r in enumerate(refs):
        got_kept = probs[b] != 0
        tiny = r.kept & (r.probs < 1e-37)  # (a kept token may weigh less than fp32's smallest value: it is then 0 on both sides)
        assert np.array_equal(got_kept | tiny, r.kept), (what, b, np.flatnonzero((got_kept | tiny) != r.kept)[:5], r.tau)
        if thr is None:
            pass
        elif truncating:
            assert bits(thr[b:b + 1])[0] == bits([r.tau])[0], (what, b, thr[b], r.tau)
        else:
            assert thr[b] == -np.inf, what
        assert (probs[b][~r.kept] == 0.0).all(), what
        assert_model_close(r.probs, probs[b], what + f" probs row {b}")
        assert abs(float(probs[b].sum(dtype=np.float64)) - 1.0) < 1e-5, what
    toks = [tok] + [edit_rows(zg, x, temp, top_k, top_p, us[i], want_probs=False, want_edited=False, **kw)[2] for i in range(1, n_u)]
    for i in range(n_u):
        for b, r in enumerate(refs):
            t = int(toks[i][b])
            assert t < V and r.kept[t], (what, "drawn token outside the kept set", i, b, t)
            exp, dist = weighted_index(r.probs, us[i][b])
            if t != exp:
                assert dist < 1e-6, (what, i, b, t, exp, float(us[i][b]))
                near += 1
    assert near <= max(2, n_u * B // 20), (what, near)


def special_rows(V, B, rng):
    """-0.0, -inf, denormals and +-1e30 among ordinary values; the three indices the edit sets below always keep hold finite values
    (a kept set whose every logit is -inf has no distribution), and there is a finite top token somewhere."""
    pool = np.array([0.0, -0.0, -np.inf, 1e-45, -1e-45, 1e-40, 1e30, -1e30, 1.5, -1.5, 3.0, 2.0], np.float32)
    x = pool[rng.integers(0, pool.size, (B, V))]
    x[:, V // 2], x[:, V // 3], x[:, V - 1] = np.float32(2.0), np.float32(1.5), np.float32(1.0)
    x[:, rng.integers(0, V)] = np.float32(4.0)
    return x


def edit_sets(V, rng):
    """The edit sets of the bit-for-bit test, by name."""
    n = min(V, 512)
    many = rng.choice(V, n, replace=False)
    sets = {
        "bias at 0 and V - 1": dict(bias={0: 1.5, V - 1: -2.25} if V > 1 else {0: 1.5}),
        f"{n} biases": dict(bias={int(i): float(v) for i, v in zip(many, rng.standard_normal(n).astype(np.float32) * 5)}),
        "allow-list of one": dict(allowed=[V // 2]),
        "everything banned but one": dict(banned=[i for i in range(V) if i != V // 3] + [0] * (V > 3)),  # (a duplicate is harmless)
        "bias, allow and ban together": dict(bias={int(i): 0.75 for i in many[: max(1, n // 3)]}, allowed=sorted({int(i) for i in many[: max(1, n // 2)]} | {V - 1}),
                                             banned=[int(i) for i in many[:3] if i != V - 1]),  # (V - 1 stays: the kept set is never empty)
    }
    return sets


@pytest.mark.parametrize("V", VOCABS)
def test_the_edited_row_is_the_reference_bit_for_bit(zg, V):
    rng = np.random.default_rng(9000 + V)
    for B in batches(V):
        for kind, x in (("normal", rows_for(V, B, rng, "normal")), ("special", special_rows(V, B, rng))):
            for name, kw in edit_sets(V, rng).items():
                y = np.stack([edit_row(x[b], kw.get("bias"), kw.get("allowed"), kw.get("banned")) for b in range(B)])
                # (top_k = 7: the truncated sampler carries 1e30; the plain one, by its own older limit, does not)
                rc, ed, tok, _, _ = edit_rows(zg, x, 0.8, 7, 1.0, rng.random(B).astype(np.float32), want_probs=False, **kw)
                assert rc == 0, (V, B, kind, name)
                assert same_bits(ed, y), (V, B, kind, name, np.argwhere(bits(ed) != bits(y))[:5])
                assert (tok < V).all() and all(y[b, int(tok[b])] > -np.inf for b in range(B)), (V, B, kind, name, tok)


@pytest.mark.parametrize("V", VOCABS)
def test_min_p_alone_and_beside_the_filters(zg, V):
    rng = np.random.default_rng(9100 + V)
    for j, (temp, mp) in enumerate(MIN_P_CASES):
        for B in batches(V) if j == 0 else (3 if V <= 4097 else 1,):
            x = rows_for(V, B, rng, "normal")
            check(zg, x, temp, 0, 1.0, mp, f"V {V} B {B} temp {temp} min_p {mp} alone", seed=j)
            check(zg, x, temp, 7, 1.0, mp, f"V {V} B {B} temp {temp} min_p {mp} top-k 7", seed=j)
    if V < 2:
        return
    for temp, mp in ((0.8, 0.05), (0.8, 0.3)):
        # top-p with its margin (one row: the cut is the row's own), then min-p cuts further or not at all
        x, p, _ = nucleus_case(V, temp, min(2, V - 1), 55)
        check(zg, x[None, :], temp, 0, p, mp, f"V {V} temp {temp} top_p {p} min_p {mp}")
    if V >= 4097:  # top-k 40, the nucleus behind 10 of them, then min-p
        x = (3.0 * np.random.default_rng(900 + V).standard_normal(V)).astype(np.float32)
        r0 = filter_row(x, 1.7, 40)
        p = float(np.float32((r0.cum[9] + r0.cum[10]) / 2))
        assert min(abs(p - c) for c in r0.cum) >= 1e-4
        for mp in (0.02, 0.5):
            check(zg, x[None, :], 1.7, 40, p, mp, f"V {V} top-k 40, top-p {p}, min_p {mp}")


@pytest.mark.parametrize("V", [257, 4097, 50257])
def test_min_p_on_edited_rows(zg, V):
    rng = np.random.default_rng(9200 + V)
    x = rows_for(V, 3, rng, "normal")
    sets = edit_sets(V, rng)
    for name in ("bias at 0 and V - 1", "512 biases" if V >= 512 else f"{V} biases", "bias, allow and ban together"):
        kw = sets[name]
        check(zg, x, 0.8, 0, 1.0, 0.05, f"V {V} {name} min_p 0.05", **kw)
        check(zg, x, 0.8, 0, 1.0, 0.0, f"V {V} {name} plain sampler", **kw)
        check(zg, x, 0.8, 7, 1.0, 0.0, f"V {V} {name} top-k 7", **kw)


@pytest.mark.parametrize("V", [65, 4097, 50257])
def test_stale_row_maximum(zg, V):
    """The partials the samplers start from are those of the UNEDITED row until the stage rebuilds them: the new top token lies in
    another slice than the old one (slices are 256-index chunks dealt round-robin; V / 6 away is another chunk from V = 4097 up)."""
    rng = np.random.default_rng(9300 + V)
    for B in (1, 3):
        x = rows_for(V, B, rng, "normal")
        top = x.argmax(axis=1)
        u = rng.random(B).astype(np.float32)
        # 1. the argmax and every runner-up nearer than a sixth of the vocabulary are banned (the same ban list for every row: the union)
        #    of its own old argmax
        banned, new_top, rest = set(), None, x.copy()
        while True:
            nt = rest.argmax(axis=1)
            close = [b for b in range(B) if abs(int(nt[b]) - int(top[b])) < max(1, V // 6)]
            if not close:
                new_top = [int(t) for t in nt]
                break
            banned.update(int(nt[b]) for b in close)
            rest[:, sorted(banned)] = -np.inf
        assert 1 <= len(banned) < V
        # 2. +1e4 on the least likely token at least V / 6 away from every row's top
        far = np.abs(np.arange(V)[None, :] - top[:, None]).min(axis=0) >= V // 6
        assert far.any()
        low = int(np.where(far, x.sum(axis=0), np.inf).argmin())
        for kw, want in ((dict(banned=sorted(banned)), new_top), (dict(bias={low: 1.0e4}), [low] * B)):
            for k in (1, 0):  # top_k = 1, and the plain sampler
                if k == 0 and "banned" in kw:
                    continue  # (banning leaves a distribution, not a point mass: the plain sampler's draw is not determined)
                rc, ed, tok, probs, thr = edit_rows(zg, x, 0.8, k, 1.0, u, **kw)
                assert rc == 0 and [int(t) for t in tok] == want, (V, B, k, kw.keys(), tok, want)
                for b in range(B):  # all of the mass on one token (the plain sampler's own rounding: one nonzero entry, 1 within 1e-6)
                    assert np.count_nonzero(probs[b]) == 1 and (probs[b, want[b]] == 1.0 if k else abs(probs[b, want[b]] - 1.0) < 1e-6), (V, B, k, b)
        # banning through the plain sampler: still never a banned token, and the probabilities are the reference's
        check(zg, x, 0.8, 0, 1.0, 0.0, f"V {V} B {B} argmax banned, plain sampler", banned=sorted(banned))


def test_an_allow_list_smaller_than_top_k(zg):
    rng = np.random.default_rng(9400)
    for V in (65, 4097, 50257):
        x = rows_for(V, 3, rng, "normal")
        allowed = sorted(int(i) for i in rng.choice(V, 5, replace=False))
        for i in range(8):
            rc, ed, tok, probs, _ = edit_rows(zg, x, 1.7, 40, 1.0, rng.random(3).astype(np.float32), allowed=allowed)
            assert rc == 0 and all(int(t) in allowed for t in tok), (V, tok, allowed)
            assert (np.count_nonzero(probs, axis=1) <= 5).all() and np.allclose(probs.sum(axis=1), 1.0, atol=1e-5)
        check(zg, x, 1.7, 40, 1.0, 0.0, f"V {V} allow 5 under top-k 40", allowed=allowed)


def test_a_nan_row_returns_a_token_inside_the_vocabulary(zg):
    rng = np.random.default_rng(9500)
    for V in (65, 4097, 50257):
        x = rows_for(V, 3, rng, "normal")
        x[1, V // 2] = np.nan
        for k, p, mp, kw in ((0, 1.0, 0.05, {}), (7, 1.0, 0.0, dict(bias={V // 2: 1.0})), (0, 0.9, 0.1, dict(banned=[0, 1])), (0, 1.0, 0.0, dict(allowed=[V // 2, 3]))):
            rc, ed, tok, _, _ = edit_rows(zg, x, 0.8, k, p, rng.random(3).astype(np.float32), min_p=mp, **kw)
            assert rc == 0 and (tok < V).all(), (V, k, p, mp, tok)
            assert same_bits(ed, np.stack([edit_row(x[b], kw.get("bias"), kw.get("allowed"), kw.get("banned")) for b in range(3)]))
    check(zg, rows_for(257, 2, rng, "normal"), 0.8, 7, 1.0, 0.05, "after the NaN rows")  # the library is still sound afterwards


def test_everything_off_is_zg_debug_sample_rows_bit_for_bit(zg):
    rng = np.random.default_rng(9600)
    for V in (65, 4097, 50257):
        x = rows_for(V, 3, rng, "normal")
        u = rng.random(3).astype(np.float32)
        for k, p in ((0, 1.0), (7, 1.0), (0, 0.9), (40, 0.85)):
            rc0, tok0, probs0, thr0 = sample_rows(zg, x, 0.8, k, p, u)
            rc1, ed, tok1, probs1, thr1 = edit_rows(zg, x, 0.8, k, p, u)
            assert rc0 == 0 and rc1 == 0 and same_bits(ed, x)
            assert np.array_equal(tok0, tok1) and np.array_equal(bits(probs0), bits(probs1)) and np.array_equal(bits(thr0), bits(thr1)), (V, k, p)


def test_refusals(zg):
    V = 64
    x = rows_for(V, 2, np.random.default_rng(9700), "normal")
    u = np.array([0.25, 0.5], np.float32)

    def rc(**kw):
        return edit_rows(zg, x, 0.8, 0, 1.0, u, **kw)[0]

    assert rc(bias={i: 0.5 for i in range(64)}) == 0
    wide = rows_for(1024, 1, np.random.default_rng(1), "normal")
    assert edit_rows(zg, wide, 0.8, 0, 1.0, u[:1], bias={i: 0.5 for i in range(513)})[0] == ARG  # n_bias > 512
    assert edit_rows(zg, wide, 0.8, 0, 1.0, u[:1], bias={i: 0.5 for i in range(512)})[0] == 0
    for v in (float("inf"), float("-inf"), float("nan")):
        assert rc(bias={3: v}) == ARG
    for mp in (-0.1, 1.0, 1.5, float("nan")):
        assert rc(min_p=mp) == ARG
    assert rc(banned=list(range(V))) == ARG                      # an empty kept set
    assert rc(allowed=[5, 6], banned=[6, 5, 5]) == ARG
    assert rc(allowed=[5, 6], banned=[6]) == 0
    assert rc(bias={V: 1.0}) == SHAPE and rc(allowed=[V]) == SHAPE and rc(banned=[2 ** 40]) == SHAPE
    # what the Python builder cannot express: a duplicate bias id, NULL arrays with counts, NULL edits
    tok, opt = np.zeros(2, np.uint64), _lib.SampleOptions(0.8, 0, 1.0)
    ids, vals = np.array([3, 9, 3], np.uint64), np.array([1, 2, 3], np.float32)

    def raw(e):
        return zg.zg_debug_edit_rows(_lib.ptr(x), 2, V, C.addressof(opt), None if e is None else C.addressof(e), _lib.ptr(u), None, _lib.ptr(tok), None, None)

    assert raw(_lib.LogitEdits(_lib.ptr(ids), _lib.ptr(vals), 3, None, 0, None, 0, 0.0)) == ARG
    assert raw(_lib.LogitEdits(_lib.ptr(ids), _lib.ptr(vals), 2, None, 0, None, 0, 0.0)) == 0
    assert raw(_lib.LogitEdits(None, _lib.ptr(vals), 2, None, 0, None, 0, 0.0)) == ARG
    assert raw(_lib.LogitEdits(_lib.ptr(ids), None, 2, None, 0, None, 0, 0.0)) == ARG
    assert raw(_lib.LogitEdits(None, None, 0, None, 2, None, 0, 0.0)) == ARG
    assert raw(_lib.LogitEdits(None, None, 0, None, 0, None, 2, 0.0)) == ARG
    assert raw(None) == ARG
    assert zg.zg_debug_edit_rows(_lib.ptr(x), 2, V, None, C.addressof(_lib.LogitEdits()), _lib.ptr(u), None, _lib.ptr(tok), None, None) == ARG
    check(zg, x, 0.8, 7, 1.0, 0.05, "after the refusals", bias={1: 2.0}, banned=[0])  # the library still works
