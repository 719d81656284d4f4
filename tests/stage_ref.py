"""The float64 side of the stage tests (test_decode_stages_gpu.py, test_pass_stages_gpu.py, test_op_stages_gpu.py and their *_cases_cpu.py): decoders of the raw
buffers a tapped decode step or whole-prompt pass returns (zg_debug_gpt_step_taps, zg_debug_gpt_pass_taps) and plain numpy float64 versions of each stage,
written from the operations' definitions (LayerNorm, Linear, split_qkv, softmax attention, the merge of split partials,
tanh-GELU, the residual add) — nothing here calls the library.

The metric of every Linear check is per output  |got - ref64| / s,  s = sqrt(sum_k (a_k w_nk)^2) + |bias_n| + |resid_n|  in
float64: the l2 norm of the products a blocked fp32 sum adds up, so that an output that happens to cancel is not held to a
relative bound no fp32 sum can meet.  The attention's s is the l2 norm of the weighted V terms p_t v_td.  The yardstick Y of a
stage is the same metric for a float32 numpy evaluation (float32 LayerNorm, float32 `@`) of the same stage from the same input."""
import numpy as np

EPS = 1e-5  # LayerNorm.eps


# ---------------------------------------------------------------------------------------------- storage formats
def bf16_bits_to_f32(u):
    return (np.asarray(u, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def round_bf16(x):
    """fp32 -> nearest bf16 (ties to even), as fp32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    b = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return b.view(np.float32)


def round_b24(x):
    """fp32 -> the 24-bit float (sign, 8 exponent bits, 15 mantissa bits; ties to even), as fp32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + np.uint64(0x7F) + ((b >> np.uint64(8)) & np.uint64(1))) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)
    return (r << np.uint64(8)).astype(np.uint32).view(np.float32).reshape(np.shape(x))


def b24_planes_to_f32(hi_u16, lo_u8):
    """B24 element: a bf16-shaped upper half and the next 8 mantissa bits in a byte plane with the same element index."""
    return ((np.asarray(hi_u16, np.uint16).astype(np.uint32) << np.uint32(16)) | (np.asarray(lo_u8, np.uint8).astype(np.uint32) << np.uint32(8))).view(np.float32)


# half an ulp of a storage format relative to the stored value, from its bit layout: p significant bits -> 2^-p
HALF_ULP = {"f32": 0.0, "f16": 2.0 ** -11, "b24": 2.0 ** -16}  # fp16: 1 + 10 bits; B24: 1 + 15 bits


def stored_matrix(w, weight_type):
    """The values a handle holds for a matrix it was given as fp32: bf16 (nearest), fp32, or the 24-bit value."""
    w = np.asarray(w, np.float32)
    return {"bf16": round_bf16, "f32": lambda v: v, "b24": round_b24}[weight_type](w)


def plane_index(K):
    """Element offsets of (plane p, batch row m, column k) of a [3][8][K] plane triple: (((k >> 5) * 3 + p) * 8 + m) * 32 + (k & 31)."""
    p = np.arange(3)[:, None, None]
    m = np.arange(8)[None, :, None]
    k = np.arange(K)[None, None, :]
    return (((k >> 5) * 3 + p) * 8 + m) * 32 + (k & 31)


def decode_planes(raw_u16, K):
    """Raw plane buffer -> the three bf16 planes as fp32 [3][8][K]."""
    raw = np.asarray(raw_u16, np.uint16)
    assert raw.size == 3 * 8 * K, (raw.size, K)
    return bf16_bits_to_f32(raw[plane_index(K)])


def planes_value(planes):
    """hi + mid + lo in float64 (exact: 24 bits of mantissa at the most)."""
    return planes.astype(np.float64).sum(axis=0)


def split3(x):
    """The exact three-term bf16 split of fp32 values: each plane the bf16 rounding of what the planes before it left."""
    x = np.asarray(x, np.float32)
    hi = round_bf16(x)
    r = x - hi
    mid = round_bf16(r)
    lo = round_bf16(r - mid)
    return np.stack([hi, mid, lo])


def planes_are_a_valid_split(planes):
    """Every plane is the bf16 rounding of what the planes before it left of the value hi + mid + lo, and nothing is left behind
    the third: [8][K] bools.  The remainders are taken in float64, where they are exact, and a plane may be 2^-16 of half a bf16
    ulp further away than the nearest bf16: a producer that rounds an fp32 intermediate first rounds twice.  (The value need not be
    an fp32 number: the embed kernel forms the remainder of gain * x with a fused multiply-subtract, so its three planes split
    the exact product.  The value itself is held to 1 ulp of float32(gain * x) by the caller.)"""
    r = planes_value(planes)
    ok = np.ones(r.shape, bool)
    for p in planes.astype(np.float64):
        with np.errstate(divide="ignore"):
            half = np.exp2(np.floor(np.log2(np.abs(r))) - 8)  # half an ulp of bf16 (8 significant bits) in r's binade
        ok &= np.where(r == 0, p == 0, np.abs(r - p) <= half * (1 + 2.0 ** -16))
        r = r - p
    return ok & (r == 0)


def planes_beyond_fp32(planes):
    """How many values hi + mid + lo are not fp32 numbers (information for the report)."""
    v = planes_value(planes)
    return int((v.astype(np.float32).astype(np.float64) != v).sum())


def decode_stats(raw_f32, E):
    """Tile statistics [8][E / 16][2]: the sum and the sum of squares of 16 columns of a batch row."""
    return np.asarray(raw_f32, np.float32).reshape(8, (E + 15) // 16, 2)


def decode_cache(taps, which, kv, B, H, T):
    """The K ("k") or V ("v") rows of positions < T as the fp32 values they stand for, [B][H][T][64], from the raw tap(s)."""
    hi = taps[which]
    if kv == "f32":
        return np.asarray(hi, np.float32).reshape(B, H, T, 64)
    if kv == "f16":
        return np.asarray(hi, np.float16).astype(np.float32).reshape(B, H, T, 64)
    return b24_planes_to_f32(hi, taps[which + "_lo"]).reshape(B, H, T, 64)


def store_kv(v, kv):
    """An fp32 value as the cache format keeps it (fp16 saturates), as fp32."""
    v = np.asarray(v, np.float32)
    if kv == "f16":
        return np.clip(v, -65504.0, 65504.0).astype(np.float16).astype(np.float32)
    return round_b24(v) if kv == "b24" else v


# ---------------------------------------------------------------------------------------------- stages, dtype-generic
def layernorm(x, g, b, dtype=np.float64):
    x, g, b = (np.asarray(t, dtype) for t in (x, g, b))
    mean = x.mean(axis=-1, keepdims=True, dtype=dtype)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True, dtype=dtype)
    return (x - mean) / np.sqrt(var + dtype(EPS)) * g + b


def gelu(x, dtype=np.float64):
    x = np.asarray(x, dtype)
    return dtype(0.5) * x * (dtype(1.0) + np.tanh(dtype(np.sqrt(2.0 / np.pi)) * x * (dtype(1.0) + dtype(0.044715) * x * x)))


K_BLOCK = 256  # the yardstick's float32 sums: `@` over blocks of 256 columns, the block sums added in float32


def linear(a, W, bias=None, resid=None, dtype=np.float64):
    """A decode Linear is one matrix-vector product per sequence and is evaluated as one, row by row, as a BLOCKED sum: `@` over
    K_BLOCK columns at a time, the block sums added in the same precision.  Every kernel under test is a blocked sum (lanes,
    waves, K slices), and the yardstick is the error of such a sum, not of one BLAS's loop order: numpy's float32 `@` over all
    of K measured 1.9e-6 of the metric at K = 5120, blocked 7.8e-7, and its matrix-matrix product 2.4e-6 at K = 384 with eight
    rows against 5.8e-7 row by row — against 9e-6 for an activation plane lost, the bound of three yardsticks needs the latter."""
    a, W = np.atleast_2d(np.asarray(a, dtype)), np.asarray(W, dtype)
    K = W.shape[1]
    y = np.stack([np.stack([W[:, k:k + K_BLOCK] @ row[k:k + K_BLOCK] for k in range(0, K, K_BLOCK)]).sum(axis=0, dtype=dtype) for row in a])
    if bias is not None:
        y = y + np.asarray(bias, dtype)
    if resid is not None:
        y = y + np.asarray(resid, dtype)
    return y


def linear_scale(a, W, bias=None, resid=None):
    """s of the metric, float64: [M][N]."""
    a, W = np.asarray(a, np.float64), np.asarray(W, np.float64)
    s = np.sqrt((a * a) @ (W * W).T)
    if bias is not None:
        s = s + np.abs(np.asarray(bias, np.float64))
    if resid is not None:
        s = s + np.abs(np.asarray(resid, np.float64))
    return s


def split_qkv(y, E):
    """[M][3 E] -> q, k, v [M][E]; head h of k / v is columns 64 h .. 64 h + 63."""
    return y[:, :E], y[:, E:2 * E], y[:, 2 * E:]


def attention(q, K, V, dtype=np.float64, scale=0.125):
    """Softmax attention of one new position over the cache: q [B][H][D], K / V [B][H][T][D] -> out [B][H][D] and the l2
    norm of the weighted V terms (always float64).  scale = 1 / sqrt(D): 0.125 for the model tier's 64."""
    q, K, V = (np.asarray(t, dtype) for t in (q, K, V))
    sc = np.einsum("bhd,bhtd->bht", q, K) * dtype(scale)
    p = np.exp(sc - sc.max(axis=-1, keepdims=True))
    p = p / p.sum(axis=-1, keepdims=True, dtype=dtype)
    out = np.einsum("bht,bhtd->bhd", p, V)
    s = np.sqrt(np.einsum("bht,bhtd->bhd", p.astype(np.float64) ** 2, V.astype(np.float64) ** 2))
    return out, s


def merge_partials(part, n_splits, dtype=np.float64):
    """Split partials [B][H][max_splits][66] = (o[64] unnormalised, running maximum m, sum l) of the first n_splits splits ->
    merged heads [B][H][64]: sum_s w_s o_s / sum_s w_s l_s, w_s = exp(m_s - max m)."""
    part = np.asarray(part, dtype)[:, :, :n_splits]
    o, m, l = part[..., :64], part[..., 64], part[..., 65]
    w = np.exp(m - m.max(axis=-1, keepdims=True))
    return (w[..., None] * o).sum(axis=2, dtype=dtype) / (w * l).sum(axis=2, dtype=dtype)[..., None]


def metric(got, ref64, s):
    """Worst |got - ref64| / s over the outputs.  An output whose s is 0 (a query that sees one key whose V element is an exact
    zero) must be exact: 0 there if it is, infinite if not."""
    d, s = np.abs(np.asarray(got, np.float64) - ref64), np.asarray(s, np.float64)
    return float(np.max(np.where(s > 0, d / np.where(s > 0, s, 1.0), np.where(d == 0, 0.0, np.inf))))


# ---------------------------------------------------------------------------------------------- a Linear stage, both sides
def linear_stage(x, W, bias, *, ln=None, resid=None, act=None, x32=None):
    """One Linear launch from its input: ref64 [M][N], s [M][N], and y32, the float32 numpy evaluation of the same stage.
    ln = (g, b): LayerNorm in front; act = "gelu": behind (the metric's s stays the Linear's: |gelu'| <= 1.13); x32: the
    float32 side's input where it is itself computed from the taps (the merged heads) rather than read from them."""
    out = []
    for dt, xin in ((np.float64, x), (np.float32, x if x32 is None else x32)):
        a = layernorm(xin, ln[0], ln[1], dt) if ln is not None else np.asarray(xin, dt)
        y = linear(a, W, bias, resid, dt)
        if act == "gelu":
            y = gelu(y, dt)
        out.append((a, y))
    (a64, ref64), (_, y32) = out
    return ref64, linear_scale(a64, W, bias, resid), y32


# lm_head only.  The metric's s, an l2 norm, is the size of a sum of UNCORRELATED products.  wte is both the embedding and lm_head:
# the final hidden state of a sequence is correlated with the wte row of the token it was fed, so that token's own logit is a sum
# of like-signed products, |logit| about sqrt(K) / 2 times s (18 s at K = 1280), and every fp32 evaluation is off by its final
# rounding and by roundings of partial sums as large as the result: ulps of the LOGIT, not of s.  Measured on MI355X with the
# plain metric: all five Linears within 3 Y except lm_head in 8 of 59 cases, on every lm_head route (VALU, 16-wave, wave-per-tile)
# alike, worst 4.7 Y = 2.8 ulp of the logit; the yardstick itself is 1.2 ulp off there, which inflates Y up to 3.3e-6 — so
# that on the CPU a lost activation plane (9.2e-6) no longer exceeded 3 Y at E = 1600.  Both sides are therefore measured with
# four ulp of the logit's own fp32 value granted (metric_granted), the yardstick too: Y is then what the uncorrelated logits give,
# the bound has its teeth again (test_decode_stage_cases_cpu.py asserts it), and for a logit of the size of s the grant is 4.8e-7 s.
LOGIT_ULPS = 4 * 2.0 ** -23

# Attention where one key holds all of the mass (score_regimes: one-key, far-below).  There the float32 numpy evaluation returns
# V's row to the bit (p = exp(0) = 1, every other term underflows), so Y is what float64 sees of the other keys, 1e-12 and less,
# and measures nothing; a correct kernel is off by the roundings between p and the output, which are ulps of the OUTPUT, not of
# s.  Both sides therefore get ATTN_ULPS of the output granted (metric_granted, as LOGIT_ULPS), counted from the operations, not
# from a measurement: the numerator o takes four roundings of half an ulp (the fused multiply-add p v, the online softmax's
# rescale by exp(m_old - m_new), the merge's weight w_s o_s, the merge's sum), the denominator l the same four, 1 / l one ulp
# (v_rcp_f32: 1 ulp by the CDNA ISA reference; half where the compiler emits the correctly rounded division, as it does without
# fast-math), o x (1 / l) half an ulp, and one v_exp_f32 (1 ulp by the same reference; the kernels reach it through __expf and
# exp2f) for a kernel whose o and l do not carry the same exp value — where they do, the exp's error cancels in o / l.
# 2 + 2 + 1 + 0.5 + 1 = 6.5, taken as 8.  (hipcc's default mode keeps f32 subnormals — cdna_hip_programming.md, the MFMA f32 notes:
# "float_denorm_mode_32 = 3" — so a running maximum started at 0 does not get away with flushing: far-below puts every score
# under ln 2^-149.)  test_decode_stage_cases_cpu.py / test_pass_stage_cases_cpu.py assert that the emulated defects clear a grant half as wide again.
ATTN_ULPS = 8 * 2.0 ** -23


# The bound of a stage is BOUND_Y[route] x Y, 3 unless a route is named here with its reason.
# GR_LM_WPT (the wave-per-tile lm_head): one wave sums all of K for its tile in two accumulator chains of K / 64 x 3 matrix-core
# accumulations each (48 at K = 1024, smallest plane first) — correct by reading, but a long sequential fp32 chain where the
# yardstick is a blocked sum.  Measured: 11 launches, 10 within 3 Y, one (E = 1024, 8 rows) at 3.69 Y = 1.14e-6 on an ordinary
# logit.  Raised to 6 Y; the three defects still exceed that by 1.5 x at its widths (test_decode_stage_cases_cpu.py asserts it:
# 5.8 x 3 Y is the least any lm_head shape measures).
# PF_T128 / PF_S4 (the whole-prompt GEMMs of prefill.hip and gemm_s4.hip with bf16 weights, test_pass_stages_gpu.py): every output
# is ONE accumulator through the whole K loop, the planes of a 16-column K step one behind the other (lo, mid, hi): a sequential
# chain of 3 K / 16 v_mfma_f32_32x32x16_bf16 accumulations (24 at K = 128, 300 at K = 1600; K / slices on the sliced launches)
# — correct by reading, and every product is exact, but the yardstick is a blocked sum whose blocks numpy adds pairwise.
# Measured on MI355X over 176 launches of the two families: the kernels' worst value is 1.0e-6 .. 2.9e-6 of the metric whatever
# the shape, about 2e-7 x sqrt(chain length); seven launches lie above 3 Y — PF_T128 at K = 128 4.25 Y (c_attn at M = 1, where Y is
# one row's 2.5e-7), 3.23 Y, 3.07 Y; PF_S4 3.07 Y at K = 768 and 3.67 / 3.74 / 3.97 Y at K = 1600.  Raised to 6 Y for both;
# the five defects of test_pass_stage_cases_cpu.py still exceed that by 1.5 x at every width (asserted there: the least is 4.0 x 3 Y
# = 2.0 x 6 Y).  The three-pass kernel for fp32 / B24 weights (PF_T128_WP, 2.57 Y at the most) keeps 3.
# OP_S4 / OP_P8_192 / OP_P8_256 (the op tier's batch >= 16 Linear: six plane products of two fp32 operands on gemm_s4_kernel and the two
# gemm_p8_kernel widths, test_op_stages_gpu.py): the same one-accumulator chain as PF_S4 with twice the pairs, 6 K / 16 accumulations
# per output (48 at K = 128, 600 at K = 1600, 6144 at the K = 16384 fall-through), smallest products first — correct by reading, every
# product exact.  Measured on MI355X over 45 launches: the three kernels return the same bits for the same shape; K = 128 / 192 within
# 1.5 Y; K = 768 2.07 .. 3.19 Y; K = 1600 3.05 .. 3.80 Y (2.2e-6); K = 16384 4.11 Y (3.8e-6).  Raised to 6 Y for the three; the six
# defects of test_op_stage_cases_cpu.py measure 13.7 Y and more at K <= 1600, 2.3 x that bound (asserted there), and 9.1 Y at K = 16384,
# the one shape that test exempts by name.
# PF_ATTN_WIDE (attn_prefill.hip under the score regimes `trained` and far-below of score_regimes.py, test_pass_stages_gpu.py; the
# cases with N(0, 0.02) weights keep 3): a score is ONE accumulator through 4 steps of 16 d x 6 plane products, 24 sequential
# v_mfma_f32_32x32x16_bf16 accumulations, of a query that was multiplied by log2(e) / 8 and rounded before its split, where the
# yardstick's score is one float32 dot product scaled afterwards — the chain of PF_T128 / PF_S4 again.  With scores +-0.05 wide
# that error never showed (the P V sum carried the output's error); with scores tens of units wide it is the output's error:
# exp turns an absolute score error into a relative error of p.  Measured on MI355X over the 9 `trained` launches: the kernels'
# worst 3.2e-6 .. 7.7e-6 whatever the shape, 1.22 .. 2.70 Y and one launch (E 384, 3 x 43 rows) at 3.02 Y; far-below 2.63 Y; a CPU
# emulation of the pre-scaled query with a float32 dot product gives 0.6 .. 1.3 Y, with an exact dot product 0.25 .. 0.6 Y, so
# the chain is about half of what is measured — correct by reading.  Raised to 6 Y; the query cut to two planes still measures
# 3.96 x 3 Y = 1.98 x 6 Y at the least and scores of 16 mantissa bits 22 x 3 Y (test_pass_stage_cases_cpu.py asserts 1.5 x against 6 Y).
# The decode kernels (one lane-tree float32 dot product per score, attn_decode.h) stay within 1.6 Y under the same regimes and keep 3.
BOUND_Y = {"GR_LM_WPT": 6.0, "PF_T128": 6.0, "PF_S4": 6.0, "OP_S4": 6.0, "OP_P8_192": 6.0, "OP_P8_256": 6.0, "PF_ATTN_WIDE": 6.0}


def bound_y(route):
    return BOUND_Y.get(route.split()[0], 3.0)


def metric_granted(got, ref64, s, rel):
    """Worst (|got - ref64| - rel |ref64|)+ / s over the outputs."""
    return float(np.max(np.maximum(np.abs(np.asarray(got, np.float64) - ref64) - rel * np.abs(ref64), 0.0) / s))


# the tile statistics are sums of 16 fp32 terms: in any order the rounding error is at most 15 u sum |t| (and one more u for each
# square), sum |t| <= 4 sqrt(sum t^2) = 4 s: 64 u s with u = 2^-24.  A term left out or counted twice is about s / 4.
STATS_BOUND = 64 * 2.0 ** -24


def tile_stats(x):
    """x [M][E] -> (sum, sum of squares) per 16-column tile in float64 and the metric's s for each: ref [M][E/16][2], s likewise."""
    t = np.asarray(x, np.float64).reshape(x.shape[0], -1, 16)
    ref = np.stack([t.sum(axis=2), (t * t).sum(axis=2)], axis=-1)
    s = np.stack([np.sqrt((t * t).sum(axis=2)), np.sqrt((t ** 4).sum(axis=2))], axis=-1)
    return ref, s


# ---------------------------------------------------------------------------------------------- the whole-prompt pass
def decode_row_planes(raw_u16, M, K):
    """The pass's plane buffers are row-major, [M][3 K] = hi | mid | lo of a row side by side -> fp32 [3][M][K]."""
    raw = np.asarray(raw_u16, np.uint16)
    assert raw.size == 3 * M * K, (raw.size, M, K)
    return bf16_bits_to_f32(np.ascontiguousarray(raw.reshape(M, 3, K).transpose(1, 0, 2)))


def causal_attention(q, K, V, past, dtype=np.float64, shift=0):
    """Causal attention of n new positions behind `past` cached ones: q [B][H][n][64], K / V [B][H][past + n][64] — the values the
    device reads: the cache's stored values, or the unrounded qkv columns where the pass reads those.  Query t sees keys
    0 .. past + t (+ shift: the emulated off-by-one mask of the teeth test).  Returns out [B][H][n][64] and s, the l2 norm of the
    weighted V terms (always float64)."""
    q, K, V = (np.asarray(t, dtype) for t in (q, K, V))
    n, T = q.shape[2], K.shape[2]
    sc = np.einsum("bhqd,bhtd->bhqt", q, K) * dtype(0.125)
    seen = np.arange(T)[None, :] <= past + np.arange(n)[:, None] + shift
    sc = np.where(seen, sc, dtype(-np.inf))
    p = np.exp(sc - sc.max(axis=-1, keepdims=True))
    p = p / p.sum(axis=-1, keepdims=True, dtype=dtype)
    out = np.einsum("bhqt,bhtd->bhqd", p, V)
    s = np.sqrt(np.einsum("bhqt,bhtd->bhqd", p.astype(np.float64) ** 2, V.astype(np.float64) ** 2))
    return out, s


def layernorm_single_pass(x, g, b, dtype=np.float32):
    """The form ops.zig:88-101 and include/zgpt2.h prescribe for LayerNorm.forward: one pass of sum and sum of squares,
    std = sqrt(E[x^2] - E[x]^2 + eps).  Equal to layernorm() in exact arithmetic; in floating point the subtraction loses
    E[x^2] / var = 1 + (mean / sigma)^2 ulps of the variance."""
    x, g, b = (np.asarray(t, dtype) for t in (x, g, b))
    n = dtype(x.shape[-1])
    mean = x.sum(axis=-1, keepdims=True, dtype=dtype) / n
    std = np.sqrt((x * x).sum(axis=-1, keepdims=True, dtype=dtype) / n - mean * mean + dtype(EPS))
    return (x - mean) / std * g + b


def layernorm_stage(x, g, b, single_pass=False):
    """One LayerNorm launch from its input rows x [M][E]: ref64, the metric's s = |g| (|x| + |mean|) / sigma + |b| — the size of
    the terms the output is made of, so that a value near the mean is not held to a relative bound — and y32, the float32 numpy
    evaluation (the yardstick): of the two-pass definition, or (single_pass: the op tier, whose kernel is documented to evaluate
    that form) of layernorm_single_pass.  ref64 is the two-pass definition in float64 either way."""
    x64, g64, b64 = (np.asarray(t, np.float64) for t in (x, g, b))
    mean = x64.mean(axis=-1, keepdims=True)
    sd = np.sqrt(((x64 - mean) ** 2).mean(axis=-1, keepdims=True) + EPS)
    s = np.abs(g64) * (np.abs(x64) + np.abs(mean)) / sd + np.abs(b64)
    return layernorm(x, g, b), s, layernorm_single_pass(x, g, b) if single_pass else layernorm(x, g, b, np.float32)


def yardstick_rows(M, n_seq, seed=0, at_least=64):
    """The rows a pass Linear's yardstick is taken over: all of them up to 256; beyond, a fixed sample — the first and the last
    row, both sides of every 128- and 256-row tile edge and of every sequence boundary (rows are ordered (sequence, position): a
    boundary every n_seq rows), and seeded others up to `at_least`."""
    if M <= 256:
        return np.arange(M)
    rows = {0, M - 1}
    for edge in list(range(128, M, 128)) + list(range(n_seq, M, n_seq)):
        rows |= {edge - 1, edge}
    rest = np.setdiff1d(np.arange(M), sorted(rows))
    extra = np.random.default_rng(seed).choice(rest, max(at_least - len(rows), 0), replace=False)
    return np.array(sorted(rows | set(int(r) for r in extra)))


def pass_linear_stage(a, W, bias, *, resid=None, act=None, n_seq=1, yardstick=True):
    """A whole-prompt Linear from the activations a [M][K] the device fed it (the value of its planes): (ref64 [M][N], s [M][N],
    Y).  Y is linear_stage's — the blocked float32 sum, row by row — over yardstick_rows; ref64 and s cover every row, ref64 as
    one float64 matrix product (which differs from the blocked float64 sum by 1e-16 of s, nine orders below Y)."""
    a64, W64 = np.asarray(a, np.float64), np.asarray(W, np.float64)
    ref = a64 @ W64.T
    if bias is not None:
        ref = ref + np.asarray(bias, np.float64)
    if resid is not None:
        ref = ref + np.asarray(resid, np.float64)
    if act == "gelu":
        ref = gelu(ref)
    s = linear_scale(a64, W64, bias, resid)
    if not yardstick:
        return ref, s, None
    rows = yardstick_rows(a64.shape[0], n_seq)
    r64, rs, y32 = linear_stage(np.asarray(a)[rows], W, bias, resid=None if resid is None else np.asarray(resid)[rows], act=act)
    return ref, s, metric(y32, r64, rs)


# ---------------------------------------------------------------------------------------------- the op tier (test_op_stages_gpu.py)
def gelu_stage(x):
    """ops.gelu from its input: ref64, the metric's s = |x| (gelu(x) = x sigmoid(2u): an error of the sigmoid, which lies in 0 .. 1,
    is an error of that size relative to x), and y32, the float32 numpy evaluation of the same tanh formula."""
    return gelu(x), np.abs(np.asarray(x, np.float64)), gelu(x, np.float32)


def gelu_tail(x, dtype=np.float64):
    """The form the kernel evaluates, x / (1 + exp(-2u)), u = sqrt(2 / pi) x (1 + 0.044715 x^2): equal to the tanh form, and the
    one that keeps its relative accuracy where 1 + tanh cancels (x << 0)."""
    x = np.asarray(x, dtype)
    u = x * dtype(0.7978845608028654) * (dtype(1.0) + dtype(0.044715) * x * x)
    with np.errstate(over="ignore"):
        return x / (dtype(1.0) + np.exp(dtype(-2.0) * u))


def softmax_stage(x):
    """ops.softmax of rows x [R][n] (each row one call): ref64 = p, s = p — a probability is held relative to itself, the small
    ones too — and y32, exp(x - max) / sum in float32 numpy."""
    out = []
    for dt in (np.float64, np.float32):
        v = np.atleast_2d(np.asarray(x, dt))
        e = np.exp(v - v.max(axis=-1, keepdims=True))
        out.append(e / e.sum(axis=-1, keepdims=True, dtype=dt))
    return out[0], out[0], out[1]


def attention_stage(q, K, V, scale):
    """One attention launch from the q / K / V it read: ref64, s and the float32 numpy evaluation."""
    ref, s = attention(q, K, V, np.float64, scale)
    return ref, s, attention(q, K, V, np.float32, scale)[0]


# the six plane products of the op tier's batch >= 16 Linear as (activation plane, weight plane), 0 = hi, 1 = mid, 2 = lo: every
# a_i w_j with i + j <= 2 (api_ops.hip linear_mfma: pa_bits / pb_bits, one hex digit per pair, smallest product first)
SIX_PAIRS = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))


def plane_products(x, W, bias, pairs=SIX_PAIRS, x_planes=None):
    """sum over (i, j) in pairs of a_i w_j^T (+ bias) in float64 from the exact three-plane splits of x [M][K] and W [N][K] — what a
    matrix-core Linear that runs exactly these products in exact arithmetic returns."""
    a = (split3(x) if x_planes is None else x_planes).astype(np.float64)
    w = split3(W).astype(np.float64)
    y = sum(a[i] @ w[j].T for i, j in pairs)
    return y if bias is None else y + np.asarray(bias, np.float64)
