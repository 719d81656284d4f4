// api_ops.hip — op tier of the C ABI (include/zgpt2.h): one entry point per public decl of the reference's src/ops.zig, same
// argument meaning, Zig slices passed as (ptr, len); zg_gemm_bf16_nt and zg_f32_to_bf16; their launch helpers.  The runtime
// they stand on — ctx(), the staging scope Call, the device twin and the KV-cache mirrors — is zg_runtime.hip.
#include "zg_runtime.h"

namespace zg {

// Linear.forward for batch >= 16 on the matrix cores (ops.zig:21-46 with M = inputs.len / in_features, :22).
// The op tier is fp32 in, fp32 out, arbitrary fp32 weights: both operands are split EXACTLY into three bf16
// planes (x = hi + mid + lo, 3 x 8 mantissa bits) and the GEMM sums the six plane products whose weight is
// above 2^-24 of the leading one — every bf16 x bf16 product is exact in fp32 and accumulation is fp32, i.e. the
// result is fp32-sgemm grade (measured against the oracle at the reference's tolerance in the tests).
// Order: small products first.
static bool linear_mfma_ok(size_t in_f, size_t out_f, size_t m, size_t arena_left) {
    if (m < 16 || in_f < 128 || in_f % 64 != 0) return false;
    if (m * in_f * 3 >= (1u << 30) || out_f * in_f * 3 >= (1u << 30)) return false;
    // a ragged width (out_f % 4 != 0) is stored by the four-wave GEMM only, whose packed arguments end at K = 16384 per plane
    // and rows of 65535 elements (three planes side by side): such a Linear stays on the GEMV kernels
    if (out_f % 4 != 0 && (in_f * 3 >= 65536 || in_f / 64 >= 256)) return false;
    return (m + out_f) * in_f * 3 * sizeof(bf16_t) + 1024 <= arena_left;
}

static int linear_mfma(Call& call, size_t in_f, size_t out_f, const float* w, const float* bias, const float* x,
                       size_t m, float* y) {
    bf16_t *xp, *wp;
    ZG_TRY(call.scratch(m * in_f * 3, &xp));
    ZG_TRY(call.scratch(out_f * in_f * 3, &wp));
    ZG_TRY(launch_split3(x, m, (int)in_f, xp, call.stream()));
    ZG_TRY(launch_split3(w, out_f, (int)in_f, wp, call.stream()));
    GemmPlanes pl{};
    pl.lda = pl.ldb = (int)(3 * in_f);
    pl.kpp = (int)(in_f / 64);
    pl.npairs = 6;  // (x plane, w plane): lo*hi, mid*mid, hi*lo, mid*hi, hi*mid, hi*hi
    pl.pa_bits = 0x001012u;
    pl.pb_bits = 0x010210u;
    return launch_gemm_planes(xp, wp, bias, y, (int)m, (int)out_f, pl, (int)out_f, false, false, call.stream());
}

// One GEMV launch of the op tier: fp32 weights, no prologue, y[M][N] = W[N][K] x[M][K] (+ bias) (+ resid under EPI_RESIDUAL).
static int op_gemv(const float* W, const float* bias, size_t N, size_t K, size_t M, const float* x, size_t x_stride, float* y, size_t y_stride,
                   int epilogue, const float* resid, size_t resid_stride, hipStream_t s) {
    GemvArgs a{};
    a.W = W;
    a.bias = bias;
    a.N = (int)N;
    a.K = (int)K;
    a.M = (int)M;
    a.prologue = PRO_NONE;
    a.epilogue = epilogue;
    a.x = x;
    a.x_stride = (int)x_stride;
    a.y = y;
    a.y_stride = (int)y_stride;
    a.resid = resid;
    a.resid_stride = (int)resid_stride;
    a.zero = ctx().d_zero;
    return launch_gemv(a, gemv_plan(a, WT_F32), WT_F32, s);
}

static int linear_device(size_t in_f, size_t out_f, const float* w, const float* bias, const float* x,
                         size_t m, float* y, hipStream_t s) {
    if (m == 0 || out_f == 0) return ZG_OK;
    ZG_REQUIRE(in_f > 0 && in_f <= 8192, ZG_ERR_UNSUPPORTED, "Linear: in_features %zu outside 1..8192", in_f);
    size_t mb = 8;
    while (mb > 1 && (mb * in_f + 8 * mb + 64) * sizeof(float) > 160 * 1024) mb >>= 1;
    for (size_t m0 = 0; m0 < m; m0 += mb)
        ZG_TRY(op_gemv(w, bias, out_f, in_f, (m - m0 < mb) ? (m - m0) : mb, x + m0 * in_f, in_f, y + m0 * out_f, out_f, EPI_STORE, nullptr, 0, s));
    return ZG_OK;
}

// Linear.forward has no size limit (src/ops.zig:21-46).  The GEMV kernels keep a batch of input rows in LDS, which ends at
// in_features = 8192: a wider Linear runs as K chunks of <= 8192 — chunk 0 computes y = bias + W[:, chunk] x[chunk], every
// later chunk adds its product to y (the residual epilogue, y aliasing the residual) — over contiguous copies of the chunk's
// columns of W (blocks of rows, so that the copy stays a few tens of MB of the staging arena) and of x.  fp32 throughout; the
// partial sums of a row meet in chunk order.
static int linear_device_wide(Call& call, size_t in_f, size_t out_f, const float* w, const float* bias, const float* x, size_t m, float* y) {
    hipStream_t s = call.stream();
    if (in_f <= 8192) return linear_device(in_f, out_f, w, bias, x, m, y, s);
    if (m == 0 || out_f == 0) return ZG_OK;
    const size_t kc_max = 8192;
    size_t rows = (((size_t)64 << 20) / (kc_max * sizeof(float)));  // rows of W per block: 64 MiB of chunk copy
    if (rows > out_f) rows = out_f;
    float *wc, *xc;
    ZG_TRY(call.scratch(rows * kc_max, &wc));
    ZG_TRY(call.scratch(8 * kc_max, &xc));
    for (size_t m0 = 0; m0 < m; m0 += 8) {
        const size_t mb = m - m0 < 8 ? m - m0 : 8;
        // (the ragged chunk goes FIRST: only the plain store epilogue of the GEMV kernels takes a K that is not a multiple of 8,
        // the accumulating chunks behind it are whole — tools/fuzz_ops.py found in_features = 8192 j + 579 failing the other way round)
        const size_t first = in_f % kc_max ? in_f % kc_max : kc_max;
        for (size_t k0 = 0; k0 < in_f; k0 += (k0 == 0 ? first : kc_max)) {
            const size_t kc = k0 == 0 ? first : kc_max;
            ZG_HIP(hipMemcpy2DAsync(xc, kc * 4, x + m0 * in_f + k0, in_f * 4, kc * 4, mb, hipMemcpyDeviceToDevice, s));
            for (size_t n0 = 0; n0 < out_f; n0 += rows) {
                const size_t nb = out_f - n0 < rows ? out_f - n0 : rows;
                ZG_HIP(hipMemcpy2DAsync(wc, kc * 4, w + n0 * in_f + k0, in_f * 4, kc * 4, nb, hipMemcpyDeviceToDevice, s));
                float* yb = y + m0 * out_f + n0;
                ZG_TRY(op_gemv(wc, (k0 == 0 && bias) ? bias + n0 : nullptr, nb, kc, mb, xc, kc, yb, out_f, k0 == 0 ? EPI_STORE : EPI_RESIDUAL,
                               k0 == 0 ? nullptr : yb, out_f, s));
            }
        }
    }
    return ZG_OK;
}

static int attn_core(const float* q, const float* k, const float* v, long stride_b, long stride_h,
                     long stride_t, size_t batch, size_t n_heads, size_t seq_len, float* out, hipStream_t s, size_t head_dim = 64) {
    const auto& part = ctx().attn_part;
    if (batch == 0 || n_heads == 0) return ZG_OK;  // k.len below one sequence: the reference's loop over the batch does nothing (ops.zig:259-261)
    const int splits = (int)((seq_len + kAttnChunk - 1) / kAttnChunk);
    // (a shape whose split partials do not fit the op tier's buffer — very long sequences x many heads — takes the general kernel too)
    if (head_dim != 64 || batch * n_heads * splits * kPartStride > part.floats)
        return launch_attn_any_dim(q, k, v, stride_b, stride_h, stride_t, (int)batch, (int)n_heads, (int)head_dim, (int)seq_len, out, s);
    AttnArgs a{};
    a.q = q;
    a.k = k;
    a.v = v;
    a.stride_b = stride_b;
    a.stride_h = stride_h;
    a.stride_t = stride_t;
    a.n_heads = (int)n_heads;
    a.head_dim = 64;
    a.batch = (int)batch;
    a.ctrl = nullptr;
    a.seq_len = (int)seq_len;
    a.t_hi = (int)seq_len;
    a.max_splits = splits;
    a.part = part.buf;
    ZG_TRY(launch_attn_decode(a, s));
    return launch_attn_merge(part.buf, (int)batch, (int)n_heads, 64, splits, (int)seq_len, out, s);
}

}  // namespace zg

using namespace zg;

extern "C" {

// ------------------------------------------------------------------------------ Linear
int zg_linear_forward(size_t in_features, size_t out_features, const float* weight,
                      const float* bias_or_null, const float* inputs, size_t inputs_len,
                      float* outputs, size_t outputs_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(in_features > 0 && weight && (inputs || inputs_len == 0), ZG_ERR_ARG, "Linear: null argument");
    const size_t batch = inputs_len / in_features;  // ops.zig:22
    ZG_REQUIRE(outputs || batch * out_features == 0, ZG_ERR_ARG, "Linear: null outputs");
    ZG_REQUIRE(inputs_len == batch * in_features, ZG_ERR_SHAPE,
               "Linear: inputs.len %zu is not a multiple of in_features %zu", inputs_len, in_features);
    ZG_REQUIRE(outputs_len >= batch * out_features, ZG_ERR_SHAPE,
               "Linear: outputs.len %zu < batch %zu * out_features %zu", outputs_len, batch, out_features);
    Call call;
    const float *w, *b, *x;
    float* y;
    ZG_TRY(call.param(weight, in_features * out_features, &w));
    ZG_TRY(call.param(bias_or_null, out_features, &b));
    ZG_TRY(call.in(inputs, inputs_len, &x));  // (read by every workgroup: device memory)
    if (in_features <= 8192) ZG_TRY(call.out_once(outputs, batch * out_features, &y));  // every element stored once
    else ZG_TRY(call.out(outputs, batch * out_features, &y));                          // K chunks accumulate into y
    if (linear_mfma_ok(in_features, out_features, batch, call.arena_left()))
        ZG_TRY(linear_mfma(call, in_features, out_features, w, b, x, batch, y));
    else
        ZG_TRY(linear_device_wide(call, in_features, out_features, w, b, x, batch, y));
    return call.finish();
}

// ------------------------------------------------------------------------------ MFMA GEMM
int zg_gemm_bf16_nt(const uint16_t* A, const uint16_t* B, const float* bias_or_null, void* C, size_t M, size_t N,
                    size_t K, int gelu, int out_bf16) {
    ZG_TRY(require_init());
    ZG_REQUIRE(A && B && C, ZG_ERR_ARG, "gemm_bf16_nt: null argument");
    ZG_REQUIRE(is_device_ptr(A) && is_device_ptr(B) && is_device_ptr(C) && (!bias_or_null || is_device_ptr(bias_or_null)),
               ZG_ERR_ARG, "gemm_bf16_nt: operands must be device pointers");
    ZG_REQUIRE(M < (1u << 30) && N < (1u << 30) && K < (1u << 30), ZG_ERR_SHAPE, "gemm_bf16_nt: dimension too large");
    return launch_gemm_bf16_nt(A, B, bias_or_null, C, (int)M, (int)N, (int)K, (int)N, gelu != 0, out_bf16 != 0,
                               ctx().stream);
}

int zg_f32_to_bf16(const float* src, uint16_t* dst_device, size_t len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(src && dst_device && is_device_ptr(dst_device), ZG_ERR_ARG, "f32_to_bf16: bad argument");
    Call call;
    const float* s;
    ZG_TRY(call.in(src, len, &s));
    ZG_TRY(launch_f32_to_bf16(s, dst_device, len, call.stream()));
    return call.finish();
}

// ------------------------------------------------------------------------------ Embedding
int zg_embedding_forward(size_t emb_dim, const float* weight, size_t weight_len, const size_t* idxs,
                         size_t idxs_len, float* embeddings, size_t embeddings_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(emb_dim > 0 && weight && (idxs || idxs_len == 0) && (embeddings || idxs_len == 0), ZG_ERR_ARG, "Embedding: null argument");
    ZG_REQUIRE(embeddings_len >= idxs_len * emb_dim, ZG_ERR_SHAPE,
               "Embedding: embeddings.len %zu < %zu indices * emb_dim %zu", embeddings_len, idxs_len, emb_dim);
    Call call;
    const float* w;
    const size_t* ix;
    float* out;
    ZG_TRY(call.param(weight, weight_len, &w));
    ZG_TRY(call.in_once(idxs, idxs_len, &ix));
    ZG_TRY(call.out_once(embeddings, idxs_len * emb_dim, &out));
    ZG_TRY(launch_embedding(w, emb_dim, ix, idxs_len, weight_len / emb_dim, out, ctx().d_flag, call.stream(), call.reserve()));
    ZG_TRY(call.finish());
    if (*static_cast<volatile int*>(ctx().d_flag)) {  // raised by the kernel (pinned host word), read behind the call's drain
        *ctx().d_flag = 0;
        set_error("embedding: index out of range (>= %zu rows)", weight_len / emb_dim);
        return ZG_ERR_SHAPE;  // (the rows of valid indices were written, like the reference up to its bounds panic)
    }
    return ZG_OK;
}

// ------------------------------------------------------------------------------ LayerNorm
int zg_layernorm_forward(size_t n_features, const float* weight, const float* bias, float eps,
                         float* inputs, size_t inputs_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(n_features > 0 && weight && bias && (inputs || inputs_len == 0), ZG_ERR_ARG, "LayerNorm: null argument");
    const size_t rows = inputs_len / n_features;
    ZG_REQUIRE(inputs_len == rows * n_features, ZG_ERR_SHAPE,
               "LayerNorm: inputs.len %zu is not a multiple of n_features %zu", inputs_len, n_features);
    Call call;
    const float *g, *b;
    float* x;
    ZG_TRY(call.param(weight, n_features, &g));
    ZG_TRY(call.param(bias, n_features, &b));
    ZG_TRY(call.inout_once(inputs, inputs_len, &x));
    DoneSlot* done = call.reserve();
    Shadow& shadow = ctx().shadow;
    float* twin = shadow.offer(inputs, x, inputs_len * sizeof(float));
    ZG_TRY(launch_layernorm(x, (int)rows, (int)n_features, g, b, eps, call.stream(), done, twin));
    ZG_TRY(call.finish());
    if (twin) shadow.keep(inputs, inputs_len * sizeof(float));
    return ZG_OK;
}

// ------------------------------------------------------------------------------ gelu / softmax
int zg_gelu(float* inputs, size_t inputs_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(inputs || inputs_len == 0, ZG_ERR_ARG, "gelu: null argument");
    Call call;
    float* x;
    ZG_TRY(call.inout_once(inputs, inputs_len, &x));
    DoneSlot* done = call.reserve();
    Shadow& shadow = ctx().shadow;
    float* twin = shadow.offer(inputs, x, inputs_len * sizeof(float));
    ZG_TRY(launch_gelu(x, inputs_len, call.stream(), done, twin));
    ZG_TRY(call.finish());
    if (twin) shadow.keep(inputs, inputs_len * sizeof(float));
    return ZG_OK;
}

int zg_softmax(float* inputs, size_t inputs_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(inputs || inputs_len == 0, ZG_ERR_ARG, "softmax: null argument");
    Call call;
    float* x;
    ZG_TRY(call.inout_once(inputs, inputs_len, &x));
    ZG_TRY(launch_softmax(x, inputs_len, call.stream(), call.reserve()));
    return call.finish();
}

// ------------------------------------------------------------------------------ split / transpose
int zg_split_qkv(size_t n_embed, size_t seq_len, const float* inputs, size_t inputs_len,
                 size_t split_idx, float* outputs, size_t outputs_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(n_embed > 0 && seq_len > 0 && split_idx < 3, ZG_ERR_ARG, "split_qkv: bad argument");
    const size_t batch = inputs_len / (seq_len * 3 * n_embed);  // ops.zig:185
    const size_t rows = batch * seq_len;
    ZG_REQUIRE(rows == 0 || (inputs && outputs), ZG_ERR_ARG, "split_qkv: null argument");
    ZG_REQUIRE(outputs_len >= rows * n_embed, ZG_ERR_SHAPE, "split_qkv: outputs.len %zu < %zu", outputs_len,
               rows * n_embed);
    Call call;
    const float* in;
    float* out;
    ZG_TRY(call.in_once(inputs, inputs_len, &in));
    ZG_TRY(call.out_once(outputs, rows * n_embed, &out));
    ZG_TRY(launch_split_qkv(in, rows, n_embed, split_idx, out, call.stream()));
    return call.finish();
}

int zg_transpose(size_t seq_len, size_t n_heads, size_t head_dim, const float* inputs,
                 size_t inputs_len, float* outputs, size_t outputs_len) {
    ZG_TRY(require_init());
    const size_t per = seq_len * n_heads * head_dim;
    ZG_REQUIRE(per > 0, ZG_ERR_ARG, "transpose: empty shape");
    const size_t batch = inputs_len / per;  // ops.zig:203
    ZG_REQUIRE(batch == 0 || (inputs && outputs), ZG_ERR_ARG, "transpose: null argument");
    ZG_REQUIRE(outputs_len >= batch * per, ZG_ERR_SHAPE, "transpose: outputs.len %zu < %zu", outputs_len, batch * per);
    ZG_REQUIRE(n_heads <= 65535 && batch <= 65535, ZG_ERR_UNSUPPORTED, "transpose: n_heads/batch > 65535");
    Call call;
    const float* in;
    float* out;
    ZG_TRY(call.in_once(inputs, inputs_len, &in));
    ZG_TRY(call.out_once(outputs, batch * per, &out));
    ZG_TRY(launch_transpose(in, batch, seq_len, n_heads, head_dim, out, call.stream()));
    return call.finish();
}

// ------------------------------------------------------------------------------ sdpa
int zg_scaled_dot_product_attention(const float* q, size_t q_len, const float* k, size_t k_len,
                                    const float* v, size_t v_len, size_t n_heads, size_t seq_len,
                                    size_t head_dim, float* outputs, size_t outputs_len, float* _attn,
                                    size_t _attn_len) {
    ZG_TRY(require_init());
    (void)_attn;
    ZG_REQUIRE(n_heads > 0 && seq_len > 0 && head_dim > 0, ZG_ERR_ARG, "sdpa: empty shape");
    ZG_REQUIRE(head_dim <= 2048, ZG_ERR_UNSUPPORTED, "sdpa: head_dim %zu beyond 2048", head_dim);
    const size_t batch = k_len / (n_heads * seq_len * head_dim);  // ops.zig:259
    ZG_REQUIRE(batch == 0 || (q && k && v && outputs), ZG_ERR_ARG, "sdpa: null argument");
    ZG_REQUIRE(v_len >= k_len && q_len >= batch * n_heads * head_dim && outputs_len >= batch * n_heads * head_dim &&
                   _attn_len >= seq_len,
               ZG_ERR_SHAPE, "sdpa: slice lengths inconsistent with batch %zu", batch);
    Call call;
    const float *dq, *dk, *dv;
    float* out;
    ZG_TRY(call.in(q, batch * n_heads * head_dim, &dq));
    ZG_TRY(call.in(k, k_len, &dk));
    ZG_TRY(call.in(v, k_len, &dv));
    ZG_TRY(call.out_once(outputs, batch * n_heads * head_dim, &out));
    ZG_TRY(attn_core(dq, dk, dv, (long)(n_heads * seq_len * head_dim), (long)(seq_len * head_dim), (long)head_dim,
                     batch, n_heads, seq_len, out, call.stream(), head_dim));
    return call.finish();
}

// ------------------------------------------------------------------------------ CausalSelfAttention
int zg_attn_forward(size_t n_heads, size_t n_embed, const float* c_attn_weight, const float* c_attn_bias,
                    const float* c_proj_weight, const float* c_proj_bias, size_t seq_len,
                    const float* inputs, size_t inputs_len, float* k_cache, size_t k_cache_len,
                    float* v_cache, size_t v_cache_len, float* outputs, size_t outputs_len, float* _qkv,
                    size_t _qkv_len, float* _q, size_t _q_len, float* _k, size_t _k_len, float* _v,
                    size_t _v_len, float* _attn, size_t _attn_len) {
    ZG_TRY(require_init());
    (void)_k;
    (void)_v;
    (void)_attn;
    const size_t E = n_embed;
    ZG_REQUIRE(n_heads > 0 && E > 0 && seq_len > 0, ZG_ERR_ARG, "attn: empty shape");
    ZG_REQUIRE(E % n_heads == 0, ZG_ERR_SHAPE, "attn: n_embed %zu is not a multiple of n_heads %zu", E, n_heads);
    const size_t hd = E / n_heads;  // 64 for every GPT-2 configuration; anything else takes the op tier's general attention kernel
    ZG_REQUIRE(inputs_len == E, ZG_ERR_SHAPE, "attn: batch must be 1 (inputs.len %zu != n_embed %zu; ops.zig:126-128)",
               inputs_len, E);
    ZG_REQUIRE(k_cache_len >= seq_len * E && v_cache_len >= seq_len * E && outputs_len >= E &&
                   _qkv_len >= 3 * E && _q_len >= E && _k_len >= seq_len * E && _v_len >= seq_len * E &&
                   _attn_len >= seq_len,
               ZG_ERR_SHAPE, "attn: a slice is shorter than seq_len %zu * n_embed %zu requires", seq_len, E);
    ZG_REQUIRE(c_attn_weight && c_attn_bias && c_proj_weight && c_proj_bias && inputs && k_cache && v_cache && outputs && _qkv && _q, ZG_ERR_ARG,
               "attn: null argument");
    ZG_REQUIRE(hd <= 2048, ZG_ERR_UNSUPPORTED, "attn: head_dim %zu beyond 2048", hd);
    Call call;
    hipStream_t s = call.stream();
    const float *caw, *cab, *cpw, *cpb, *x;
    float *kc = nullptr, *vc = nullptr, *out, *qkv, *q;
    ZG_TRY(call.param(c_attn_weight, 3 * E * E, &caw));
    ZG_TRY(call.param(c_attn_bias, 3 * E, &cab));
    ZG_TRY(call.param(c_proj_weight, E * E, &cpw));
    ZG_TRY(call.param(c_proj_bias, E, &cpb));
    ZG_TRY(call.in(inputs, E, &x));
    // The caller owns the caches and appends one row per call (ops.zig:152,157); what it can observe afterwards is row T-1.
    // Host caches are mirrored on the device, keyed by their address: when this call continues the sequence the mirror holds
    // (same pointer, same width, seq_len = rows held + 1) nothing goes up and only the new row comes back; anything else
    // — a first sight, a restart, a jump — uploads rows 0 .. T-2 again.  A caller that EDITS earlier rows in place between two
    // consecutive positions must drop the mirror (zg_unregister_tensor(cache)).  No room in the pool: the whole cache is staged.
    KvMirrors& mirrors = ctx().mirrors;
    KvMirror* mir[2];
    float* const host_cache[2] = {k_cache, v_cache};
    mirrors.make_room(host_cache, seq_len, E);
    ZG_TRY(mirrors.attach(k_cache, seq_len, E, call, &kc, &mir[0]));
    ZG_TRY(mirrors.attach(v_cache, seq_len, E, call, &vc, &mir[1]));
    ZG_TRY(call.out_once(outputs, E, &out));  // stored once by c_proj
    ZG_TRY(call.out(_qkv, 3 * E, &qkv));      // read back by the append and the attention: device memory
    ZG_TRY(call.out(_q, E, &q));
    // c_attn (ops.zig:143)
    ZG_TRY(linear_device(E, 3 * E, caw, cab, x, 1, qkv, s));
    // cache append (ops.zig:151-152, :156-157): into the device cache, and — for mirrored host caches — row T-1 back to the caller
    ZG_TRY(launch_copy2_f32(qkv + E, kc + (seq_len - 1) * E, qkv + 2 * E, vc + (seq_len - 1) * E, E, s));
    if (mir[0]) ZG_TRY(call.also_out(k_cache + (seq_len - 1) * E, qkv + E, E * sizeof(float)));
    if (mir[1]) ZG_TRY(call.also_out(v_cache + (seq_len - 1) * E, qkv + 2 * E, E * sizeof(float)));
    // attention straight over the [T, H, hd] cache (replaces transposes + sdpa, ops.zig:153-171);
    // the merged heads land in _q like the reference's "untranspose" (ops.zig:171)
    ZG_TRY(attn_core(qkv, kc, vc, 0, (long)hd, (long)E, 1, n_heads, seq_len, q, s, hd));
    // c_proj (ops.zig:172)
    ZG_TRY(linear_device(E, E, cpw, cpb, q, 1, out, s));
    ZG_TRY(call.finish());
    for (KvMirror* m : mir)
        if (m) m->rows = seq_len;
    return ZG_OK;
}

}  // extern "C"
