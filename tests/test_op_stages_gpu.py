"""The public op tier (zig_gpt2_amd.ops -> zg_linear_forward, zg_layernorm_forward, zg_gelu, zg_softmax,
zg_scaled_dot_product_attention, zg_attn_forward) held to float64, route by route, with the stage metric of the model tier's
stage tests: |got - ref64| / s within stage_ref.bound_y(route) x Y, Y the same metric for a float32 numpy evaluation of the same
formula from the same input (stage_ref).  test_ops_gpu.py holds these ops to the reference's tolerance (6e-4 relative), which
is fifty times a dropped plane product of the batch >= 16 Linear; this module is where such a defect fails.

The cases and the kernel each one must run on come from op_stage_cases.py, whose coverage and whose bounds' teeth
test_op_stage_cases_cpu.py asserts without a GPU; here the kernel a call reports (zg_debug_last_kernel, zg_debug_gemm_launches)
is held to that prediction before anything is compared.

LayerNorm: the kernel deliberately evaluates the reference's single-pass form, std = sqrt(E[x^2] - E[x]^2 + eps) (src/ops.zig:88-95,
include/zgpt2.h), and the float64 reference here is the two-pass definition.  The two agree to fp32 rounding only while
|mean| / sigma is modest — the subtraction loses 1 + (mean / sigma)^2 ulps of the variance — so the rows keep mean 0.3 and standard
deviation 2.0, and a large offset is not tested: it would measure the formula the reference prescribes, not the kernel.  For the
same reason the yardstick is the float32 numpy evaluation of THAT formula (stage_ref.layernorm_stage(single_pass=True)); the
reference stays the float64 two-pass definition.  With the two-pass float32 yardstick five of the six shapes measure the same
(Y within 6 %), and the (1, 5) row, whose five draws happen to have mean / sigma = 1.17, does not: two-pass Y 3.2e-8 (half an ulp,
over five outputs), single-pass Y 1.29e-7, the kernel 1.65e-7 = 5.2 of the former and 1.28 of the latter — the single-pass float32
numpy evaluation reproduces the loss on the CPU, so it is the formula's, not the kernel's.

gelu: beside the metric (s = |x|), the negative tail x in -12 .. -3 is held RELATIVE to |ref64| (DESIGN section 4 claims relative
accuracy in both tails): within 3 x the relative error of the float32 numpy evaluation of the kernel's own form
x / (1 + exp(-2u)), bin by bin of width 1, wherever the result is a normal float32 and exp(-2u) is finite in float32; beyond
that the result must have flushed towards zero.

Measured on one MI355X (123 cases, 3.2 s for the module; metric values; "launches" are kernel launches, or calls for the elementwise ops):

| route | cases | launches | Y | worst | worst / Y (at) |
|---|---|---|---|---|---|
| GR_VALU, K <= 8192 | 8 | 9 | 3.8e-7 .. 5.8e-7 | 4.27e-7 | 1.12 (8x1600x64) |
| GR_KSPLIT | 3 | 3 | 4.2e-7 .. 8.1e-7 | 2.54e-7 | 0.50 (1x2048x72) |
| GR_VALU + GR_KSPLIT (row blocks 4 + 1 at K = 8192) | 1 | 2 | 7.5e-7 | 7.32e-7 | 0.98 |
| GR_GENERIC | 6 | 7 | 1.4e-7 .. 3.9e-7 | 4.05e-7 | 1.70 (8x4108x1: eight outputs) |
| K chunks: GR_KSPLIT, GR_KSPLIT + resid onto y | 1 | 2 | 6.0e-7 | 2.49e-7 | 0.42 |
| K chunks: GR_VALU, GR_VALU + resid (also the 2048-row block of W) | 4 | 10 | 4.6e-7 .. 7.3e-7 | 8.40e-7 | 1.36 (3x16384x24) |
| K chunks: GR_VALU_GROUPS (+ resid), GR_KSPLIT (+ resid) | 1 | 4 | 6.3e-7 | 7.05e-7 | 1.13 (9x16384x16) |
| K chunks: GR_GENERIC, then GR_KSPLIT / GR_VALU / GR_VALU_GROUPS + resid | 5 | 15 | 4.1e-7 .. 1.0e-6 | 6.21e-7 | 1.52 (3x8771x37) |
| OP_S4 six pairs, K = 128 / 192 | 12 | 12 | 2.5e-7 .. 6.0e-7 | 8.07e-7 | 1.46 (257x192x260) |
| OP_S4 six pairs, K = 768 | 8 | 8 | 4.1e-7 .. 7.3e-7 | 1.74e-6 | 3.19 (129x768x193) |
| OP_S4 six pairs, K = 1600 | 6 | 6 | 5.3e-7 .. 6.1e-7 | 2.22e-6 | 3.80 (127x1600x193) |
| OP_P8_192 six pairs, K <= 1600 | 9 | 9 | 2.5e-7 .. 7.1e-7 | 1.87e-6 | 3.20 (16x1600x260) |
| OP_P8_192 six pairs, K = 16384 (the fall-through) | 1 | 1 | 9.2e-7 | 3.80e-6 | 4.11 |
| OP_P8_256 six pairs | 9 | 9 | 2.5e-7 .. 7.3e-7 | 1.87e-6 | 3.20 (16x1600x260) |
| LayerNorm, row in registers (single-pass Y) | 10 | 10 | 1.3e-7 .. 2.6e-7 | 2.51e-7 | 1.28 (1x5) |
| LayerNorm, n = 4097 | 2 | 2 | 1.6e-7 | 1.62e-7 | 0.99 |
| gelu, s = abs(x) | 6 | 257 | 7.7e-8 .. 1.1e-7 | 1.16e-7 | 1.17 (n = 64) |
| gelu, x in -10 .. -3 relative to abs(ref64), per unit bin | 7 | 1 | 1.6e-6 .. 1.1e-5 | 1.26e-5 | 1.25 (-8 .. -7) |
| softmax, N(0, 3) | 8 | 327 | 0 .. 1.1e-6 | 1.83e-6 | 1.88 (n = 65) |
| softmax, one dominant element | 3 | 3 | 2.0e-6 .. 2.1e-6 | 5.13e-6 | 2.49 (n = 50257) |
| ATTN_64 (attn_decode + merge), 1 / 2 / 3 splits | 8 | 8 | 0 .. 2.7e-6 | 7.31e-7 | 0.54 (T = 64) |
| ATTN_64, one dominant key in each split | 4 | 4 | 3.9e-12 .. 8.0e-12 | 8.01e-12 | 1.00 (the float32 evaluation's bits) |
| ATTN_ANY (attn_any_dim_kernel), head_dim 7 .. 2048 | 8 | 8 | 3.7e-7 .. 2.3e-6 | 4.21e-6 | 2.08 (d 2048, T 19) |
| attn.forward: c_attn / c_proj (GR_VALU), 40 steps each, heads 2 and 4 | 4 | 160 | 3.5e-7 .. 5.1e-7 | 4.05e-7 | 1.00 |
| attn.forward: attention, T = 1 .. 40, ATTN_64 / ATTN_ANY | 2 | 80 | 7.9e-7 .. 9.2e-7 | 8.16e-7 | 0.89 |

The three matrix-core kernels return the same bits for the same shape.  Their six-pair chain is one accumulator through 6 K / 16
accumulations; it lies above 3 Y from K = 768 on and carries 6 Y (stage_ref.BOUND_Y, with the reason).  Everything else is within
3 Y.  No defect was found in a kernel.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import op_stage_cases as oc
import stage_ref as sr
from zig_gpt2_amd import _lib, ops, synth

pytestmark = pytest.mark.gpu


def z(*shape):
    return np.zeros(shape, np.float32)


def last_kernel(zg):
    sym = C.create_string_buffer(160)
    _lib.check(zg.zg_debug_last_kernel(sym, 160))
    return sym.value.decode()


def assert_stage(what, route, got, ref, s, y32, launches=1):
    """The stage metric: printed, then asserted."""
    Y, worst = sr.metric(y32, ref, s), sr.metric(got, ref, s)
    bound = sr.bound_y(route)
    print(f"STAGE {what} | {route} | launches {launches} | Y {Y:.3e} worst {worst:.3e} = {worst / Y if Y > 0 else (0.0 if worst == 0 else np.inf):.2f} Y, bound {bound:.0f} Y")
    assert worst <= bound * Y, (what, route, worst, Y)


@functools.lru_cache(maxsize=None)
def linear_reference(M, K, N, bias):
    """Operands and both sides of the reference, once per shape: the forces, placements and workgroup caps of a shape share them."""
    x, w, b = oc.linear_operands(M, K, N)
    b = b if bias else None
    for a in (x, w, b):
        if a is not None:
            a.setflags(write=False)
    return (x, w, b) + sr.linear_stage(x, w, b)


# ---------------------------------------------------------------------------------------------- Linear
@pytest.mark.parametrize("case", oc.LINEAR_CASES, ids=lambda c: c.id)
def test_linear_stage(zg, monkeypatch, case):
    import torch

    M, K, N = case.M, case.K, case.N
    x, w, b, ref, s, y32 = linear_reference(M, K, N, case.bias)
    route, kernel, gemms = oc.route_of(case)
    for name, v in (("ZGPT2_GEMM_KERNEL", case.force), ("ZGPT2_GEMM_WGS", case.wgs)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    if case.place == "device":
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        wd, bd, xd, yd = dev(w), dev(b), dev(x), torch.full((M, N), float("nan"), device="cuda")
        torch.cuda.synchronize()  # (the fills run on torch's stream, the library launches on its own)
    else:
        wd, bd, xd, yd = w, b, x, np.full((M, N), np.nan, np.float32)
        if case.place == "registered":
            _lib.check(zg.zg_register_tensor(w.ctypes.data, w.size))
            if b is not None:
                _lib.check(zg.zg_register_tensor(b.ctypes.data, b.size))
    before = zg.zg_debug_gemm_launches()
    try:
        ops.Linear(K, N, wd, bd).forward(xd, yd)
    finally:
        if case.place == "registered":
            _lib.check(zg.zg_unregister_all())
    assert zg.zg_debug_gemm_launches() - before == gemms, (case.id, route)
    assert last_kernel(zg).startswith(kernel), (case.id, route, last_kernel(zg), kernel)
    got = yd.cpu().numpy() if case.place == "device" else yd
    launches = 1 if gemms else len(oc.gemv_launches(M, K, N, case.bias))
    assert_stage(f"Linear {case.id}", route, got, ref, s, y32, launches)


# ---------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("place", ["host", "device"])
@pytest.mark.parametrize("rows,n", oc.LAYERNORM_CASES)
def test_layernorm_stage(zg, rows, n, place):
    import torch

    x, g, b = oc.layernorm_operands(rows, n)
    ref, s, y32 = sr.layernorm_stage(x, g, b, single_pass=True)
    if place == "device":
        xd = torch.from_numpy(x.copy()).cuda()
        torch.cuda.synchronize()
        ops.LayerNorm(n, g, b).forward(xd)
        got = xd.cpu().numpy()
    else:
        got = x.copy()
        ops.LayerNorm(n, g, b).forward(got)
    assert_stage(f"LayerNorm {rows}x{n} {place}", "LN " + ("registers" if n <= 2048 else "two reads"), got, ref, s, y32)


# ---------------------------------------------------------------------------------------------- gelu
@pytest.mark.parametrize("n", oc.GELU_SIZES)
def test_gelu_stage(zg, n):
    x = synth.fill_normal(9 + n, oc.rows_for(n) * n, 0, 2.0).reshape(-1, n)
    got = x.copy()
    for row in got:
        ops.gelu(row)
    ref, s, y32 = sr.gelu_stage(x)
    assert_stage(f"gelu {n} x {len(x)} calls", "GELU", got, ref, s, y32, len(x))


def test_gelu_negative_tail_is_relatively_accurate(zg):
    x = synth.fill_uniform(77, 9 * 1024, -12.0, -3.0)
    got = x.copy()
    ops.gelu(got)
    ref, y32 = sr.gelu_tail(x), sr.gelu_tail(x, np.float32)
    x64 = x.astype(np.float64)
    u2 = -2.0 * x64 * 0.7978845608028654 * (1.0 + 0.044715 * x64 * x64)
    held = (np.abs(ref) >= 2.0 ** -126) & (u2 < 88.0)   # a normal float32 result from a finite float32 exp(-2u)
    assert held.sum() > 6500 and (~held).sum() > 500
    assert np.all(np.abs(got[~held]) <= 2.0 ** -120), "beyond the float32 range of exp(-2u) the result flushes towards zero"
    rel = lambda v: np.abs(v.astype(np.float64) - ref) / np.abs(ref)
    for lo in range(-12, -3):
        m = held & (x >= lo) & (x < lo + 1)
        if not m.any():
            continue
        Y, worst = rel(y32)[m].max(), rel(got)[m].max()
        print(f"STAGE gelu tail x in [{lo}, {lo + 1}) | GELU relative | outputs {int(m.sum())} | Y {Y:.3e} worst {worst:.3e} = {worst / Y:.2f} Y, bound 3 Y")
        assert worst <= 3.0 * Y, (lo, worst, Y)


# ---------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("n", oc.SOFTMAX_SIZES)
def test_softmax_stage(zg, n):
    x = synth.fill_normal(40 + n, oc.rows_for(n) * n, 0.0, 3.0).reshape(-1, n)
    got = x.copy()
    for row in got:
        ops.softmax(row)
    ref, s, y32 = sr.softmax_stage(x)
    assert_stage(f"softmax {n} x {len(x)} calls", "SOFTMAX " + ("registers" if n <= 65536 else "two reads"), got, ref, s, y32, len(x))


@pytest.mark.parametrize("n,hot", [(1025, 0), (1025, 1024), (50257, 31000)])
def test_softmax_one_dominant_element(zg, n, hot):
    """One element 30 above N(0, 3): every other probability is e^-30 and below, and is still held relative to itself."""
    x = synth.fill_normal(45 + n, n, 0.0, 3.0)
    x[hot] = 40.0
    got = x.copy()
    ops.softmax(got)
    ref, s, y32 = sr.softmax_stage(x)
    assert_stage(f"softmax {n} dominant at {hot}", "SOFTMAX registers", got[None], ref, s, y32)


# ---------------------------------------------------------------------------------------------- attention
def run_sdpa(q, k, v):
    b, h, T, d = k.shape
    y = np.full(b * h * d, np.nan, np.float32)
    ops.scaled_dot_product_attention(np.ascontiguousarray(q).ravel(), np.ascontiguousarray(k).ravel(), np.ascontiguousarray(v).ravel(), h, T, d, y, z(T))
    return y.reshape(b, h, d)


@pytest.mark.parametrize("b,h,T", oc.SDPA64_CASES)
def test_sdpa_head_dim_64_stage(zg, b, h, T):
    """attn_decode + merge over the op tier's head-major strides.  (T = 1: the one probability is 1 — Y is 0 and the output must be V's row.)"""
    q, k, v = oc.attention_operands(b, h, T, 64)
    got = run_sdpa(q, k, v)
    assert last_kernel(zg) == "attn_decode_kernel<float>"
    assert_stage(f"sdpa b{b} h{h} T{T}", f"ATTN_64 {(T + 255) // 256} splits", got, *sr.attention_stage(q, k, v, 0.125))


def test_sdpa_one_dominant_key_stage(zg):
    """The cross-wave / cross-split rescale: one key far above the rest, placed in each split (test_ops_gpu.py test_sdpa_one_dominant_key)."""
    h, T = 2, 700
    for hot in (0, 100, 300, 699):
        q = synth.fill_normal(60, h * 64, 0, 1.0).reshape(1, h, 64)
        k = synth.fill_normal(61, h * T * 64, 0, 0.3).reshape(1, h, T, 64)
        k[0, :, hot] = q[0] * 4.0
        v = synth.fill_normal(62, h * T * 64, 0, 1.0).reshape(1, h, T, 64)
        got = run_sdpa(q, k, v)
        assert last_kernel(zg) == "attn_decode_kernel<float>"
        assert_stage(f"sdpa hot key {hot} of {T}", "ATTN_64 3 splits", got, *sr.attention_stage(q, k, v, 0.125))


@pytest.mark.parametrize("h,d,T", oc.SDPA_ANY_CASES)
def test_sdpa_any_head_dim_stage(zg, h, d, T):
    q, k, v = oc.attention_operands(1, h, T, d)
    got = run_sdpa(q, k, v)
    assert last_kernel(zg) == "attn_any_dim_kernel"
    assert_stage(f"sdpa h{h} d{d} T{T}", "ATTN_ANY", got, *sr.attention_stage(q, k, v, 1.0 / np.sqrt(d)))


@pytest.mark.parametrize("hds", [2, 4])
def test_attn_forward_stages(zg, hds):
    """CausalSelfAttention.forward over 40 incremental steps at e = 128 (head_dim 64: attn_decode + merge; 32: the general kernel,
    over the cache's [T][H][d] strides), every sub-stage from the buffers the call leaves behind: c_attn from the input to _qkv,
    the cache rows bitwise equal to _qkv's k / v columns, the attention from the device's own q / K / V to the merged heads the
    call leaves in _q (ops.zig:171), c_proj from those to the output.  The 40 steps of a sub-stage are one stage of 40 rows."""
    e, T = 128, 40
    d = e // hds
    caw = synth.fill_normal(70, 3 * e * e, 0, 0.08).reshape(3 * e, e)
    cab = synth.fill_normal(71, 3 * e, 0, 0.05)
    cpw = synth.fill_normal(72, e * e, 0, 0.08).reshape(e, e)
    cpb = synth.fill_normal(73, e, 0, 0.05)
    xs = synth.fill_normal(74, T * e, 0, 1.0).reshape(T, e)
    attn = ops.CausalSelfAttention(hds, e, ops.Linear(e, 3 * e, caw, cab), ops.Linear(e, e, cpw, cpb))
    k_cache, v_cache = z(T * e), z(T * e)
    _qkv, _q, _k, _v, _attn = z(3 * e), z(e), z(T * e), z(T * e), z(T)
    qkvs, heads, outs, att = z(T, 3 * e), z(T, e), z(T, e), []
    for t in range(1, T + 1):
        attn.forward(t, xs[t - 1], k_cache[: t * e], v_cache[: t * e], outs[t - 1], _qkv, _q, _k[: t * e], _v[: t * e], _attn[:t])
        qkvs[t - 1], heads[t - 1] = _qkv, _q
        assert np.array_equal(k_cache[(t - 1) * e: t * e].view(np.uint32), _qkv[e:2 * e].view(np.uint32)), f"k row {t - 1}"
        assert np.array_equal(v_cache[(t - 1) * e: t * e].view(np.uint32), _qkv[2 * e:].view(np.uint32)), f"v row {t - 1}"
        kv = lambda c: np.ascontiguousarray(c[: t * e].reshape(1, t, hds, d).transpose(0, 2, 1, 3))
        ref, s, y32 = sr.attention_stage(_qkv[:e].reshape(1, hds, d), kv(k_cache), kv(v_cache), 1.0 / np.sqrt(d))
        att.append((ref.ravel(), s.ravel(), y32.ravel()))
    assert np.array_equal(k_cache.reshape(T, e), qkvs[:, e:2 * e]) and np.array_equal(v_cache.reshape(T, e), qkvs[:, 2 * e:])  # no earlier row was touched
    (l,) = oc.gemv_launches(1, e, 3 * e)
    assert_stage(f"attn.forward heads {hds}: c_attn, 40 steps", l.route, qkvs, *sr.linear_stage(xs, caw, cab), T)
    assert_stage(f"attn.forward heads {hds}: attention, T = 1 .. 40", "ATTN_64 1 split" if d == 64 else "ATTN_ANY", heads, *(np.stack(c) for c in zip(*att)), T)
    (l,) = oc.gemv_launches(1, e, e)
    assert_stage(f"attn.forward heads {hds}: c_proj, 40 steps", l.route, outs, *sr.linear_stage(heads, cpw, cpb), T)
