"""The case list of test_op_stages_gpu.py, judged on the CPU: (1) coverage — every route an op-tier Linear can plan, all three
matrix-core kernels with six pairs, both chunk epilogues and every kind of first chunk appear in a case, and what the module
docstring of op_stage_cases.py calls unreachable is unreachable by the plan; (2) teeth — the bound the GPU test applies,
stage_ref.bound_y(route) x Y with Y the float32 numpy evaluation's own error, is exceeded 1.5 x by every emulated defect, at every
shape the GPU test runs on that route.  The defects are emulated in float64 from exact planes (stage_ref.split3), so what is
measured is the defect alone, without any accumulation error on top."""
import numpy as np
import pytest

import op_stage_cases as oc
import stage_ref as sr
from test_gemv_plan_cpu import EPI_RESID, EPI_STORE
from zig_gpt2_amd import synth


# ---------------------------------------------------------------------------------------------- coverage
GEMV = [c for c in oc.LINEAR_CASES if not oc.mfma_ok(c.M, c.K, c.N)]
MC = [c for c in oc.LINEAR_CASES if oc.mfma_ok(c.M, c.K, c.N)]


def names(launches):
    return {(l.route, l.epi) for l in launches}


def test_every_route_a_plain_linear_can_plan_is_in_a_case():
    planned = set()
    for M in range(1, 16):
        for K in (1, 7, 8, 64, 100, 256, 768, 1600, 2040, 2048, 2056, 3072, 4104, 4108, 6400, 8184, 8192, 8200, 8771, 8776, 12328, 16384, 16389, 20000, 24581):
            for N in (1, 37, 300, 2100):
                planned |= names(oc.gemv_launches(M, K, N))
    covered = set()
    for c in GEMV:
        covered |= names(oc.gemv_launches(c.M, c.K, c.N, c.bias))
    assert planned <= covered, planned - covered
    assert {r for r, _ in covered} == set(oc.ROUTES)
    assert {e for _, e in covered} == {EPI_STORE, EPI_RESID}            # both chunk epilogues
    assert ("GR_KSPLIT", EPI_RESID) in covered and ("GR_VALU", EPI_RESID) in covered and ("GR_VALU_GROUPS", EPI_RESID) in covered
    print(sorted(covered))


def test_the_list_has_the_shapes_the_gemv_paths_branch_on():
    assert {c.M for c in GEMV if c.K <= 8192} >= {1, 3, 8, 9, 5}
    assert {c.M for c in GEMV if c.K > 8192} >= {1, 3, 9}
    assert {c.bias for c in GEMV} == {True, False} and {c.place for c in GEMV} == {"host", "device", "registered"}
    # row blocks: 8 + 1 at M = 9; 4 + 1 at K = 8192
    assert [l.M for l in oc.gemv_launches(9, 384, 131)] == [8, 1]
    ls = oc.gemv_launches(5, 8192, 40)
    assert [(l.M, l.route) for l in ls] == [(4, "GR_VALU"), (1, "GR_KSPLIT")]
    # the first chunk: whole (K % 8192 == 0), ragged on the generic kernel (K % 8 != 0), ragged on gemv_kernel (a multiple of 8)
    first = {(l.K == oc.K_CHUNK, l.route) for c in GEMV if c.K > 8192 for l in oc.gemv_launches(c.M, c.K, c.N)[:1]}
    assert first >= {(True, "GR_KSPLIT"), (True, "GR_VALU"), (False, "GR_GENERIC"), (False, "GR_VALU")}, first
    # ... and in every chunked case the ragged chunk, if any, is the first and stores; every later chunk is whole and accumulates
    for c in GEMV:
        if c.K > 8192:
            for l in oc.gemv_launches(c.M, c.K, c.N):
                assert (l.epi == EPI_STORE) == (l.k0 == 0) and (l.k0 == 0 or l.K == oc.K_CHUNK), (c.id, l)
    assert any(len({l.n0 for l in oc.gemv_launches(c.M, c.K, c.N)}) == 2 for c in GEMV if c.K > 8192)  # the 2048-row block of W
    assert {16384, 8192 + 579, 16389} <= {c.K for c in GEMV}
    # GR_GENERIC: K = 100, 4104 + 4 and 7; N = 37 and N = 1
    gen = [c for c in GEMV if c.K <= 8192 and c.K % 8]
    assert {c.K for c in gen} == {100, 4108, 7} and {c.N for c in gen} == {37, 1}
    # GR_KSPLIT at both ends of its range
    assert {c.K for c in GEMV if c.M == 1 and oc.gemv_launches(1, c.K, c.N)[0].route == "GR_KSPLIT" and c.K <= 8192} == {2048, 8192}


def test_what_the_module_calls_unreachable_is_unreachable():
    # GR_VALU_GROUPS: never through linear_device's row blocks, always for 5 .. 8 rows of a whole chunk
    for M in range(1, 16):
        for K in range(8, 8193, 8):
            assert all(l.route != "GR_VALU_GROUPS" for l in oc.gemv_launches(M, K, 4)), (M, K)
    for M in range(1, 9):
        routes = [l.route for l in oc.gemv_launches(M, 16384, 4)]
        assert routes == ["GR_KSPLIT" if M == 1 else "GR_VALU" if M <= 4 else "GR_VALU_GROUPS"] * 2, (M, routes)
    assert oc.gemv_launches(8, 16384, 4)[0].plan["row_group"] == 4
    # waves per workgroup at M = 1 on GR_VALU: 1, or 2 for K in 2048 .. 8192 — never 4, however wide the matrix
    seen = set()
    for K in (8, 64, 768, 1600, 2040, 2056, 4104, 8184):
        for N in (1, 72, 2304, 50257, 200000, 1 << 20):
            (l,) = oc.gemv_launches(1, K, N)
            assert l.route == "GR_VALU"
            seen.add(l.plan["waves_per_wg"])
    assert seen == {1, 2}
    mine = {l.plan["waves_per_wg"] for c in GEMV if c.M == 1 and c.K <= 8192 for l in oc.gemv_launches(1, c.K, c.N) if l.route == "GR_VALU"}
    assert mine == {1, 2}
    assert oc.gemv_launches(1, 64, 50257)[0].plan["waves_per_wg"] == 1


def test_all_three_matrix_core_kernels_run_six_pairs_in_the_list():
    ran = {}
    for c in MC:
        ran.setdefault(oc.gemm_kernel(c.M, c.N, c.K, c.force), []).append(c)
    assert set(ran) == {"s4", "p8:192", "p8:256"}
    for k, cs in ran.items():
        if k != "s4":  # (ragged widths are the four-wave kernel's)
            assert all(c.N % 4 == 0 for c in cs)
        assert {c.M for c in cs} >= {16, 127, 128, 129, 257}, k
        assert {c.K for c in cs} >= {128, 192, 768, 1600}, k
        assert {c.N for c in cs} >= {8, 192, 260}, k
        assert any(c.wgs == 1 or c.wgs == 3 for c in cs), k
    assert {c.N for c in ran["s4"]} >= {131, 193}
    assert {c.wgs for c in MC} >= {1, 3}
    assert {c.force for c in MC} == {None, "s4", "p8:192", "p8:256"}
    assert all(oc.gemm_kernel(c.M, c.N, c.K, None) == "s4" for c in MC if c.K < 16384)    # the unforced choice at these sizes
    assert any(c.force is None and c.K < 16384 for c in MC)
    # several tiles per workgroup where the workgroups are capped
    assert all(oc.gemm_tiles(c.M, c.N, oc.gemm_kernel(c.M, c.N, c.K, c.force)) > c.wgs for c in MC if c.wgs)
    # a ragged width stays on the four-wave kernel under a force, and K = 16384 leaves it
    assert oc.gemm_kernel(128, 131, 192, "p8:256") == "s4" and oc.gemm_kernel(257, 193, 768, "p8:192") == "s4"
    assert oc.gemm_kernel(*[oc.FALL_THROUGH[i] for i in (0, 2, 1)]) == "p8:192"
    assert oc.mfma_ok(16, 16384, 128) and not oc.mfma_ok(16, 16384, 130) and not oc.mfma_ok(15, 768, 64) and not oc.mfma_ok(16, 100, 64)
    assert {c.place for c in MC} == {"host", "device", "registered"}
    assert len({c.id for c in oc.LINEAR_CASES}) == len(oc.LINEAR_CASES)


# ---------------------------------------------------------------------------------------------- teeth
def margin(what, defect, Y, bound, exempt=False):
    ratio = defect / (bound * Y) if Y > 0 else np.inf
    print(f"TEETH {what}: Y {Y:.2e}  defect {defect:.2e} = {defect / Y:.1f} Y = {ratio:.1f} x the bound of {bound:.0f} Y" + ("  (exempt)" if exempt else ""))
    assert ratio >= (1.0 if exempt else 1.5), (what, defect, Y, bound)


def without(pair):
    return tuple(p for p in sr.SIX_PAIRS if p != pair)


MC_SHAPES = sorted({(c.M, c.K, c.N) for c in MC})


@pytest.mark.parametrize("M,K,N", MC_SHAPES)
def test_six_product_defects_exceed_the_bound_by_half(M, K, N):
    """Each of the three cross products dropped (lo.hi, mid.mid, hi.lo), lo.hi taken twice in place of hi.lo (one digit of pa_bits),
    the activation's lo plane lost, the weight rounded to B24 — under the widest bound any case of this shape is given.  The six
    products as designed are printed beside them.  Exempt from the 1.5 x, by name and alone: the fall-through shape K = 16384
    (op_stage_cases.FALL_THROUGH).  Its chain of 6144 accumulations measured 4.11 Y on the MI355X, so it shares its kernel's 6 Y, and
    the weakest defect there is 9.1 Y = 1.5 x that bound with nothing to spare (Y is a float32 BLAS sum and moves a few per cent
    between hosts).  It stays on the GPU as a check of the fall-through at that bound; here its defects must still exceed the bound."""
    x, w, b = oc.linear_operands(M, K, N)
    ref, s, y32 = sr.linear_stage(x, w, b)
    Y = sr.metric(y32, ref, s)
    bound = max(sr.bound_y(oc.route_of(c)[0]) for c in MC if (c.M, c.K, c.N) == (M, K, N))
    designed = sr.metric(sr.plane_products(x, w, b), ref, s)
    print(f"TEETH {M}x{K}x{N}: the six products as designed {designed:.2e} = {designed / Y:.2f} Y")
    assert designed < 0.5 * Y
    xp = sr.split3(x)
    two = xp.copy()
    two[2] = 0
    exempt = (M, K, N) == oc.FALL_THROUGH
    defects = {"lo.hi dropped": sr.plane_products(x, w, b, without((2, 0))), "mid.mid dropped": sr.plane_products(x, w, b, without((1, 1))),
               "hi.lo dropped": sr.plane_products(x, w, b, without((0, 2))), "lo.hi twice for hi.lo": sr.plane_products(x, w, b, without((0, 2)) + ((2, 0),)),
               "activation lo plane lost": sr.plane_products(x, w, b, x_planes=two), "weight rounded to B24": sr.plane_products(x, sr.round_b24(w), b)}
    for name, got in defects.items():
        margin(f"{M}x{K}x{N} {name}", sr.metric(got, ref, s), Y, bound, exempt)


@pytest.mark.parametrize("case", [c for c in GEMV if c.K > 8192 and c.K % 8], ids=lambda c: c.id)
def test_a_ragged_tail_cut_to_a_multiple_of_eight_exceeds_the_bound_by_half(case):
    """K chunks: the ragged chunk's last K % 8 columns dropped (what a chunk handed to a kernel that takes multiples of 8 would lose)."""
    x, w, b = oc.linear_operands(case.M, case.K, case.N)
    b = b if case.bias else None
    ref, s, y32 = sr.linear_stage(x, w, b)
    first = case.K % oc.K_CHUNK
    cut = x.copy()
    cut[:, first - first % 8:first] = 0
    margin(f"{case.id} last {first % 8} columns of the ragged chunk dropped", sr.metric(sr.linear(cut, w, b), ref, s), sr.metric(y32, ref, s), sr.bound_y(oc.route_of(case)[0]))


@pytest.mark.parametrize("rows,n", oc.LAYERNORM_CASES)
def test_layernorm_defects_exceed_the_bound_by_half(rows, n):
    x, g, b = oc.layernorm_operands(rows, n)
    ref, s, y32 = sr.layernorm_stage(x, g, b, single_pass=True)
    Y = sr.metric(y32, ref, s)
    x64 = x.astype(np.float64)
    mean = x64.mean(axis=-1, keepdims=True)
    for name, var in (("n - 1 divisor", x64.var(axis=-1, keepdims=True, ddof=1) + sr.EPS), ("eps omitted", x64.var(axis=-1, keepdims=True))):
        margin(f"LayerNorm {rows}x{n} {name}", sr.metric((x64 - mean) / np.sqrt(var) * g + b, ref, s), Y, 3.0)


@pytest.mark.parametrize("n", oc.GELU_SIZES)
def test_gelu_with_a_shortened_constant_exceeds_the_bound_by_half(n):
    x = synth.fill_normal(9 + n, oc.rows_for(n) * n, 0, 2.0)
    ref, s, y32 = sr.gelu_stage(x)
    x64 = x.astype(np.float64)
    bad = 0.5 * x64 * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * x64 * (1.0 + 0.0447 * x64 * x64)))
    margin(f"gelu {n} with 0.0447", sr.metric(bad, ref, s), sr.metric(y32, ref, s), 3.0)


def scores_b24(q, K, V, scale):
    sc = sr.round_b24((np.einsum("bhd,bhtd->bht", q.astype(np.float64), K.astype(np.float64)) * scale).astype(np.float32)).astype(np.float64)
    p = np.exp(sc - sc.max(axis=-1, keepdims=True))
    return np.einsum("bht,bhtd->bhd", p / p.sum(axis=-1, keepdims=True), V.astype(np.float64))


@pytest.mark.parametrize("b,h,T,d", [(b, h, T, 64) for b, h, T in oc.SDPA64_CASES if T > 1] + [(1, h, T, d) for h, d, T in oc.SDPA_ANY_CASES])
def test_attention_defects_exceed_the_bound_by_half(b, h, T, d):
    """V rounded to the 24-bit float, the scores rounded to it.  (T = 1 has no defect to show: the one probability is 1 and the
    output is V's row, which the GPU test then holds to equality — its Y is 0.)"""
    q, k, v = oc.attention_operands(b, h, T, d)
    scale = 1.0 / np.sqrt(d)
    ref, s, y32 = sr.attention_stage(q, k, v, scale)
    Y = sr.metric(y32, ref, s)
    route = "ATTN_64" if d == 64 else "ATTN_ANY"
    margin(f"attention b{b} h{h} T{T} d{d} V as B24", sr.metric(sr.attention(q, k, sr.round_b24(v), np.float64, scale)[0], ref, s), Y, sr.bound_y(route))
    margin(f"attention b{b} h{h} T{T} d{d} scores as B24", sr.metric(scores_b24(q, k, v, scale), ref, s), Y, sr.bound_y(route))
