/*
 * zgpt2.h — C ABI of libzgpt2_hip.so: the MI355X (gfx950) implementation of zig_gpt2's forward
 * hot path.  This is the drop-in boundary: every entry point below replaces one public decl of
 * the reference's src/ops.zig (op tier) or one method of src/main.zig (model tier); the Zig shim
 * zig_gpt2_amd/zig/ops.zig keeps the reference's decl signatures and forwards each slice as
 * (ptr, len).  Citations are file:line in /root/reference (EugenHotaj/zig_gpt2 @ v1).
 *
 * Conventions
 *   - All functions return 0 on success, a negative zg_status otherwise; zg_last_error() gives
 *     text.  The reference's ops return void and rely on Zig slice bounds checks; the length
 *     checks those imply are done here and reported as ZG_ERR_SHAPE.
 *   - Lengths are ELEMENT counts (Zig slice .len), not bytes.  f32 is IEEE binary32, usize is
 *     size_t (8 bytes).
 *   - Op tier: every pointer may be host memory or device memory (detected with
 *     hipPointerGetAttributes).  Host buffers are staged through arenas that are allocated once
 *     in zg_init — no *_forward call allocates device or host memory (the reference's
 *     "no allocations at runtime" contract, README.md:6, src/main.zig:46-64): a device arena
 *     (ZGPT2_STAGING_MB, 512), a pinned host arena (ZGPT2_PINNED_MB, 32) through which the caller's
 *     pageable buffers travel — small vectors that a kernel touches once are read / written by the
 *     kernel in place across PCIe, the rest moves by one DMA each way — and a device pool for the
 *     mirrors of caller-owned KV caches (ZGPT2_KV_MIRROR_MB, 1024; see zg_attn_forward).  Op-tier
 *     calls are synchronous on return, because the reference's host code reads the buffers next
 *     (src/main.zig:136-145).
 *   - Model tier: weights, KV cache and every scratch buffer live in one device arena created by
 *     zg_gpt_create; zg_gpt_forward/zg_gpt_generate_greedy only launch kernels.
 *   - Single-threaded like the reference: one call at a time per process.
 */
#ifndef ZGPT2_H
#define ZGPT2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    ZG_OK = 0,
    ZG_ERR_NOT_INITIALIZED = -1,
    ZG_ERR_SHAPE = -2,      /* a slice length does not match the shapes implied by the call */
    ZG_ERR_HIP = -3,        /* a HIP runtime call failed (text in zg_last_error) */
    ZG_ERR_STAGING = -4,    /* host buffers of one call exceed the staging arena */
    ZG_ERR_UNSUPPORTED = -5,
    ZG_ERR_ARG = -6
} zg_status;

/* ------------------------------------------------------------------ runtime ---------------- */

/* Select the device, create the stream and the host-staging arena (default 512 MiB, or
 * ZGPT2_STAGING_MB).  Idempotent. */
int zg_init(int device);
int zg_init_ex(int device, size_t staging_bytes);
/* Drain the library stream and free everything zg_init_ex made (arenas, registered tensors, KV-cache mirrors, the own stream).
 * Every zg_gpt handle must be destroyed BEFORE this call: the model tier stages through the runtime's arena and launches on its
 * stream.  A caller-owned stream given to zg_set_stream is drained, never destroyed.  Afterwards every entry that needs the
 * runtime returns ZG_ERR_NOT_INITIALIZED until zg_init is called again (a fresh runtime: nothing registered, no mirrors); a
 * second zg_shutdown is ZG_OK. */
int zg_shutdown(void);
const char* zg_last_error(void);
/* Launch on a caller-owned hipStream_t — a stream the caller created, e.g. a torch.cuda.Stream() made current — so that the
 * library's work is ordered with the caller's on that stream.  The stream the library leaves is drained first.  A NULL handle
 * means the library's OWN stream (and restores it): the legacy default stream, whose handle is 0 — torch's default stream — cannot
 * be selected, and work a caller queues there is NOT ordered with the library's (the own stream is non-blocking).  Handles without
 * a private stream follow the change: their decode graphs are captured again on the first call that sees the new stream.  The
 * stream must outlive its use: restore NULL (or shut down) before destroying it.  Same thread as every other call. */
int zg_set_stream(void* hip_stream);
int zg_synchronize(void);
/* Upload a host PARAMETER tensor (Linear / Embedding weight, bias, LayerNorm vectors) once and keep a
 * device mirror keyed by its host address: later op-tier calls that receive the same host pointer WITH THE
 * SAME LENGTH in a parameter position use the mirror instead of re-staging it (weights are borrowed for
 * the life of the arena in the reference, src/main.zig:349-351).  Activation arguments (inputs, idxs,
 * q / k / v) are never looked up, so a freed weight's address may be reused for them.  Re-registering an
 * address replaces its mirror; host weights changed in place after registration must be registered
 * again.  zg_unregister_tensor drops one mirror (the `defer allocator.free(weight)` moment of
 * src/tests.zig) — also the KV-cache mirror zg_attn_forward keeps for that address; zg_unregister_all
 * drops every mirror and empties the KV pool. */
int zg_register_tensor(const float* host_ptr, size_t len);
int zg_unregister_tensor(const float* host_ptr);
int zg_unregister_all(void);

/* ------------------------------------------------------------------ op tier: src/ops.zig --- */

/* Linear.forward — src/ops.zig:21-46.  weight is [out_features, in_features] row-major (the
 * reference's "column major", ops.zig:9); bias may be NULL; batch = inputs_len / in_features
 * (ops.zig:22); outputs [batch, out_features]. */
int zg_linear_forward(size_t in_features, size_t out_features, const float* weight,
                      const float* bias_or_null, const float* inputs, size_t inputs_len,
                      float* outputs, size_t outputs_len);

/* Embedding.forward — src/ops.zig:59-67.  weight [n_rows, emb_dim]; idxs are usize. */
int zg_embedding_forward(size_t emb_dim, const float* weight, size_t weight_len,
                         const size_t* idxs, size_t idxs_len, float* embeddings,
                         size_t embeddings_len);

/* LayerNorm.forward — src/ops.zig:82-104.  In place over inputs_len / n_features rows;
 * std = sqrt(E[x^2] - E[x]^2 + eps) (ops.zig:95). */
int zg_layernorm_forward(size_t n_features, const float* weight, const float* bias, float eps,
                         float* inputs, size_t inputs_len);

/* CausalSelfAttention.forward — src/ops.zig:129-173: one decode step with a caller-owned KV
 * cache, batch 1.  k_cache / v_cache are the caller's [seq_len, n_embed] slices (row t = token
 * t); row seq_len-1 is written by this call (ops.zig:152,157).  _qkv [3E], _q [E], _k/_v
 * [seq_len*E], _attn [seq_len] are the reference's scratch slices; on return _qkv holds the
 * c_attn output and _q the merged heads (ops.zig:171) as in the reference, while _k/_v/_attn
 * (pure scratch whose content no caller reads) are left untouched: the kernel attends over the
 * [T, H, hd] cache in place instead of re-transposing it every step (ops.zig:153,158).
 * HOST caches are mirrored on the device, keyed by the cache's address: a call that continues the
 * sequence the mirror holds (same pointer, same n_embed, seq_len = rows held + 1 — the only pattern
 * src/main.zig:331-338 produces) uploads nothing and returns only row seq_len-1 to the caller's
 * buffer; any other call (first sight, position 1 again, a jump, a repeated position) uploads rows
 * 0..seq_len-2 from the caller's buffer first.  A caller that EDITS rows it already handed over and
 * then continues with the next position must drop the mirror first (zg_unregister_tensor(cache)).
 * The pool is a bump allocator: when the caches of a call do not fit what is left of it, every mirror is dropped and the pool
 * starts over (live caches upload once more at their next call); a cache larger than the whole pool is staged whole on every
 * call, as before. */
int zg_attn_forward(size_t n_heads, size_t n_embed, const float* c_attn_weight,
                    const float* c_attn_bias, const float* c_proj_weight, const float* c_proj_bias,
                    size_t seq_len, const float* inputs, size_t inputs_len, float* k_cache,
                    size_t k_cache_len, float* v_cache, size_t v_cache_len, float* outputs,
                    size_t outputs_len, float* _qkv, size_t _qkv_len, float* _q, size_t _q_len,
                    float* _k, size_t _k_len, float* _v, size_t _v_len, float* _attn,
                    size_t _attn_len);

/* CausalSelfAttention.split_qkv — src/ops.zig:177-196: [B, T, 3E] -> [B, T, E]. */
int zg_split_qkv(size_t n_embed, size_t seq_len, const float* inputs, size_t inputs_len,
                 size_t split_idx, float* outputs, size_t outputs_len);

/* CausalSelfAttention.transpose — src/ops.zig:199-216: (b, t, n, h) -> (b, n, t, h). */
int zg_transpose(size_t seq_len, size_t n_heads, size_t head_dim, const float* inputs,
                 size_t inputs_len, float* outputs, size_t outputs_len);

/* scaled_dot_product_attention — src/ops.zig:249-307.  q [B,H,1,hd], k/v [B,H,T,hd],
 * outputs [B,H,1,hd]; B = k_len / (H*T*hd) (ops.zig:259); _attn_len must be >= seq_len.  Any head_dim up to 2048: 64 (every
 * GPT-2 configuration) runs the split-KV kernels, anything else a general fp32 kernel (one workgroup per sequence and head). */
int zg_scaled_dot_product_attention(const float* q, size_t q_len, const float* k, size_t k_len,
                                    const float* v, size_t v_len, size_t n_heads, size_t seq_len,
                                    size_t head_dim, float* outputs, size_t outputs_len,
                                    float* _attn, size_t _attn_len);

/* gelu — src/ops.zig:221-228, in place. */
int zg_gelu(float* inputs, size_t inputs_len);

/* softmax — src/ops.zig:231-241, in place; the whole slice is one vector. */
int zg_softmax(float* inputs, size_t inputs_len);

/* Batched-regime Linear on the matrix cores (MFMA): C[M,N] = A[M,K] * B[N,K]^T (+ bias) with an
 * optional fused GELU — the same contraction as Linear.forward's cblas_sgemm(NoTrans, Trans)
 * (src/ops.zig:30-45) for large batch (prefill), with both operands in ops.Linear's K-contiguous
 * layouts.  A, B are bf16 bit patterns and C is bf16 (out_bf16 != 0) or fp32, all DEVICE pointers;
 * any M; N a multiple of 8 for bf16 C, any N for fp32 C (an N that is not a multiple of 4 is stored by the four-wave kernel
 * only, whose packed arguments end at K = 16320: beyond that ZG_ERR_UNSUPPORTED — zg_linear_forward, which has no such limit,
 * takes such a Linear through its GEMV kernels); K a multiple of 64 and at least 128.  Asynchronous on
 * the library stream.  zg_linear_forward itself takes this path for batch >= 16 (fp32 operands split
 * exactly into bf16 planes, so the result stays fp32-sgemm grade).
 * zg_f32_to_bf16 converts a device or host fp32 array into a device bf16 array (round to nearest even; FLT_MAX rounds to inf; a
 * NaN stays a NaN of its sign, quiet, with its upper payload bits — as the bf16 weight upload of zg_gpt_load_*). */
int zg_gemm_bf16_nt(const uint16_t* A, const uint16_t* B, const float* bias_or_null, void* C, size_t M,
                    size_t N, size_t K, int gelu, int out_bf16);
/* Diagnostic: number of matrix-core GEMM launches so far in this process (tests assert which path a
 * Linear took; no reference counterpart). */
unsigned long long zg_debug_gemm_launches(void);
/* Diagnostic: shader-clock stamps {count, start, end} of workgroup 0 / wave 0 of the last GEMM launched with
 * ZGPT2_GEMM_DBG bit 256 (tools/microbench/gemm_bench.cpp: cycles vs wall time = the clock the chip ran at). */
int zg_debug_gemm_stamps(unsigned long long* out, size_t n_words);
/* Diagnostic (tests): the completion word of the op tier.  Every op-tier call polls a pinned word for its own 32-bit sequence
 * number (compared for equality); a call whose word never arrives drains the stream instead.  zg_debug_ops_set_done_seq sets the
 * number the next call continues from (tests: in front of its wrap); zg_debug_ops_done_state: out[0] = the sequence number last
 * given out, out[1] = the pinned word, out[2] = calls so far that polled to the end without seeing their number and drained
 * the stream.  n_out >= 3.  Both need zg_init. */
int zg_debug_ops_set_done_seq(unsigned seq);
int zg_debug_ops_done_state(unsigned long long* out, size_t n_out);
/* Diagnostic / test entry: ONE whole-prompt Linear exactly as zg_gpt_prefill launches it (src/ops.zig:21-46 for M = batch x
 * prompt rows).  A = the activation planes [M][3 K] bf16 (hi | mid | lo: the exact split of the fp32 rows), W = bf16 weights
 * [N][K], all device pointers.  epilogue: 0 fp32 C[M][N] = A W^T + bias; 1 C[M][N] += ... (residual add; ws required);
 * 2 bf16 planes C[M][3 N] of gelu(...).  force_kernel: 0 = the library's choice, 1 = the persistent four-wave GEMM
 * (gemm_s4.hip; slices = its K slices for epilogue 1, 0 = chosen), 2 = the 128-row prompt GEMM (prefill.hip).  ws: fp32
 * workspace of ws_floats elements for partial slabs.  The cache-append epilogue is exercised through zg_gpt_prefill. */
int zg_debug_prefill_linear(const uint16_t* A_planes, const uint16_t* W, const float* bias_or_null, void* C, size_t M, size_t N,
                            size_t K, int epilogue, int force_kernel, int slices, float* ws, size_t ws_floats);
/* Diagnostic / test entry: the causal prompt attention of zg_gpt_prefill alone (scaled_dot_product_attention of src/ops.zig:249-307
 * for all n_tokens positions of `batch` sequences at once).  qkv: fp32 [batch n_tokens][3 n_embed] rows (q | k | v columns);
 * out: bf16 planes [batch n_tokens][3 n_embed] = hi | mid | lo of the attention output; k_cache / v_cache: NULL (K and V are the
 * qkv columns) or head-major fp32 caches [batch][heads][ctx][64] holding the same rows; ws: fp32 workspace for the partials of
 * split key ranges (may be NULL: whole rows per workgroup); key_tiles: key tiles of 32 per workgroup, 0 = the library's choice.
 * Device pointers. */
int zg_debug_attn_prefill(const float* qkv, uint16_t* out, size_t batch, size_t n_tokens, size_t n_embed, size_t n_heads,
                          const float* k_cache, const float* v_cache, size_t ctx, float* ws, size_t ws_floats, int key_tiles);
/* ... of a continuation (zg_gpt_extend): qkv holds only the n_tokens new rows of every sequence, positions past_len .. past_len +
 * n_tokens - 1, and only their q columns are read.  EVERY key, cached and new, comes from the head-major caches
 * [batch][heads][ctx][64], which hold positions 0 .. past_len + n_tokens - 1 in storage format kv_mode: 0 fp32, 1 fp16, 2 B24 (a
 * bf16-shaped plane of batch heads ctx 64 elements, then a byte plane, as ZG_GPT_KV_B24 keeps it).  Rows behind the last
 * position may hold anything.  past_len + n_tokens <= ctx; the rest as zg_debug_attn_prefill. */
int zg_debug_attn_prefill_at(const float* qkv, uint16_t* out, size_t batch, size_t past_len, size_t n_tokens, size_t n_embed, size_t n_heads,
                             const void* k_cache, const void* v_cache, int kv_mode, size_t ctx, float* ws, size_t ws_floats, int key_tiles);
/* Test hook: pin the route of every whole-prompt Linear of this process until called again with (0, 0) — force_kernel / slices
 * as in zg_debug_prefill_linear; force_kernel >= 16: the library's rule with that many 256 x 192 tiles (x K slices) as the
 * threshold from which the persistent GEMM takes a Linear (default 192; tools/experiments/pf_route_ab.py).
 * tests/test_prefill_gpu.py runs small models through the persistent GEMM's epilogues with it. */
int zg_debug_prefill_route(int force_kernel, int slices);
/* Diagnostic: name of the kernel instantiation the last decode-kernel launcher of this thread picked (launches recorded
 * into a graph count; bench.py reports it as the symbol of the roofline kernel). */
int zg_debug_last_kernel(char* out, size_t n);
/* Diagnostic: the plan of a decode-regime Linear y[M][N] = x[M][K] W^T — which kernel it would take and how it is laid out —
 * without launching anything; works without a GPU and without zg_init.  prologue 0 none, 1 LayerNorm, 2 head merge; epilogue
 * 0 store, 1 residual, 2 GELU, 3 QKV + cache append, 4 partial argmax; weight_type 0 bf16, 1 fp32, 2 B24; operands: the optional
 * operands present (ZG_PLAN_*); sk_tiles: tiles of the split-K workspace (ZG_PLAN_SPLIT_K); t_hi: launch-time bound of the
 * sequence length (0 = none).  out[ZG_GEMV_PLAN_INTS]: route (0 VALU, 1 VALU in row groups, 2 generic K % 8 != 0, 3 K split,
 * 4 folded LayerNorm, 5 matrix cores 16-wave, 6 ... K-sliced, 7 plane-fed four-wave, 8 ... K-sliced, 9 lm_head wave per tile),
 * grid x, grid y = K slices, block threads, dynamic LDS bytes, batch rows held, lanes per row, chunks per lane, 32-k steps per
 * wave, waves (16-wave kernel), line loads, planes from global memory, aliased partials, 64-k pairs, steps per tile, rows per wave
 * or tiles per workgroup, waves per workgroup, row-group size, rows of W per workgroup and tiles as the prefetcher takes them,
 * supported, may take planes, may write planes, four-wave kernel when given planes. */
#define ZG_GEMV_PLAN_INTS 24
#define ZG_PLAN_LN_FOLDED 1u      /* ln_c2 / ln_c3: the LayerNorm folded out of the dot product */
#define ZG_PLAN_PLANES_IN 2u      /* pl_in */
#define ZG_PLAN_STATS_IN 4u       /* st_in */
#define ZG_PLAN_SPLIT_K 8u        /* sk_ws + sk_cnt with sk_tiles */
#define ZG_PLAN_RAGGED_STRIDES 16u /* row strides of x / y / residual wider than the rows */
int zg_debug_gemv_plan(int M, int N, int K, int prologue, int epilogue, int weight_type, unsigned operands, int sk_tiles, int t_hi, int* out,
                       size_t n_out);
/* Diagnostic: the plan of a whole-prompt Linear C[M][N] = A[M][3 K] W[N][K]^T as zg_gpt_prefill would launch it — which GEMM
 * family, which instantiation, its grid, and what finishes it — without launching anything; works without a GPU and without
 * zg_init.  epilogue: 0 fp32 store, 1 residual add, 2 GELU + split planes, 4 qkv store + cache append; nsplit: activation planes
 * multiplied (2 or 3), or 33 = fp32 weights as three planes; ws_floats: the split-K workspace; operands: what is present
 * (ZG_PFPLAN_*; the cache description has n_embed = N / 3); sk_ws_bytes / sk_flags_words: the stream-K hand-over's buffers;
 * force_kernel / force_slices as in zg_debug_prefill_linear (the pin of zg_debug_prefill_route is not read); ZGPT2_GEMM_WGS caps
 * the persistent kernel's workgroups as in a launch.  out[ZG_PREFILL_PLAN_INTS]: status (ZG_OK or the refusal a launch would
 * return; the rest is 0 then), family (1 persistent four-wave GEMM, 2 128-row kernel, 3 128-row three-pass kernel for fp32
 * weights), tail (0 none, 1 LayerNorm + split, 2 reduce, 3 reduce then LayerNorm + split, 4 reduce + residual + LayerNorm + split
 * in one), partial slabs through the workspace, grid x, grid y, block threads, dynamic LDS bytes, K slices, slabs the tail sums,
 * 128-row kernels: 64-column strips per wave, planes multiplied, rows of the XCD grid, tile columns; persistent kernel: epilogue
 * kind (1 partial slabs, 2 qkv, 3 GELU + split), stream-K hand-over, tile-order band width, plane pairs, A plane bits, B plane
 * bits, B plane-major. */
#define ZG_PREFILL_PLAN_INTS 21
#define ZG_PFPLAN_WS 1u        /* a split-K workspace */
#define ZG_PFPLAN_LN 2u        /* a LayerNorm follows (residual adds) */
#define ZG_PFPLAN_QKV 4u       /* the cache description of the qkv epilogue */
#define ZG_PFPLAN_SK_WS 8u     /* ... with a stream-K workspace */
#define ZG_PFPLAN_SK_FLAGS 16u /* ... and flag words */
int zg_debug_prefill_plan(int M, int N, int K, int ldc, int epilogue, int nsplit, size_t ws_floats, unsigned operands, size_t sk_ws_bytes,
                          unsigned sk_flags_words, int force_kernel, int force_slices, int* out, size_t n_out);
int zg_f32_to_bf16(const float* src, uint16_t* dst_device, size_t len);

/* ------------------------------------------------------------------ model tier: src/main.zig */

/* GPTConfig — src/main.zig:5-23, field for field. */
typedef struct {
    size_t vocab_size;
    size_t context_size;
    size_t n_layer;
    size_t n_heads;
    size_t n_embed;
} zg_gpt_config;

typedef struct zg_gpt zg_gpt;

enum {
    ZG_GPT_WEIGHTS_BF16 = 0,     /* Linear/embedding matrices stored bf16 (RNE) — default */
    ZG_GPT_WEIGHTS_F32 = 1 << 0, /* keep matrices in fp32 (exact with arbitrary checkpoints) */
    ZG_GPT_NO_GRAPH = 1 << 1,    /* launch kernels eagerly instead of replaying a hipGraph */
    ZG_GPT_KV_F16 = 1 << 2,      /* store the KV cache as fp16 instead of fp32 */
    ZG_GPT_NO_PREFILL = 1 << 3,  /* generate: feed prompts one position at a time, as main.zig:331-334 does */
    ZG_GPT_PREFILL_2PLANE = 1 << 4, /* whole-prompt GEMMs multiply two bf16 planes of the fp32 activations instead of the exact
                                      three: 2/3 of the matrix work, ~2e-5 of the logit scale (inside the 1e-3 parity bound,
                                      outside the tests' near-zero floor); bf16-weight handles only */
    ZG_GPT_NO_PREFETCH = 1 << 5, /* zg_gpt_generate_*: no side-stream L2 prefetcher beside the decode chain (results are
                                    identical either way; a measurement switch) */
    ZG_GPT_SAMPLED_GENERATE = 1 << 7, /* capture the decode graphs of zg_gpt_generate_sample_* at create as well.  The rule of all
                                      four *_GENERATE flags: create captures the greedy graphs and those the flags name; a
                                      generation that needs others captures them, for the 64-position buckets it touches, when it
                                      begins — before its first step: the one place a generate call may allocate */
    ZG_GPT_KV_B24 = 1 << 6,      /* store the KV cache as 24-bit floats (the fp32 value rounded to 16 mantissa bits, kept as a
                                    bf16 plane + a plane of 8 more mantissa bits): 3/4 of the fp32 cache's traffic, 2^-17 per
                                    cached element — inside the 1e-3 parity bound at full context, unlike ZG_GPT_KV_F16 (which
                                    it excludes) */
    ZG_GPT_TRUNCATED_GENERATE = 1 << 9, /* capture the decode graphs of zg_gpt_generate_sample_ex_* (top-k / top-p truncation) at
                                      create as well (the rule: ZG_GPT_SAMPLED_GENERATE) */
    ZG_GPT_PENALIZED_GENERATE = 1 << 10, /* capture the decode graphs of zg_gpt_generate_pen_enqueue (logit penalties in front of the
                                      sampler, all three sampler forms) at create as well (the rule: ZG_GPT_SAMPLED_GENERATE).
                                      context_size > 8192: ZG_ERR_UNSUPPORTED */
    ZG_GPT_LOGPROBS_GENERATE = 1 << 11, /* capture the decode graphs of zg_gpt_generate_logprobs_enqueue at create as well: the
                                      log-probability twins of every graph with lm_head that create captures (the greedy ones, and
                                      those of the ZG_GPT_SAMPLED_ / _TRUNCATED_ / _PENALIZED_GENERATE flags given beside it; the
                                      rule: ZG_GPT_SAMPLED_GENERATE) */
    ZG_GPT_SCORE = 1 << 12,      /* carve what zg_gpt_score needs behind everything else in the scratch region: the logits of one block
                                    of 256 rows on the GEMMs' 64-column grid, the chunk workspace of that block, and the lm_head
                                    operand beside the weight region (bf16 weights: the last vocab % 64 rows of wte as a [64][n_embed]
                                    strip; fp32 / B24 weights: wte's bf16 planes and the slab workspace of that launch).  54 MB at
                                    GPT-2 124M whatever the batch.  Without it zg_gpt_score is ZG_ERR_UNSUPPORTED and
                                    the handle has bit for bit the layout and behaviour it has without this flag's existence */
    ZG_GPT_STOP_GENERATE = 1 << 13, /* capture the decode graphs of zg_gpt_generate_stop_enqueue at create as well: the stop twins of
                                      every graph with lm_head that create captures (the greedy ones, those of the other *_GENERATE
                                      flags given beside it, their log-probability twins under ZG_GPT_LOGPROBS_GENERATE; the rule:
                                      ZG_GPT_SAMPLED_GENERATE) */
    ZG_GPT_EDITED_GENERATE = 1 << 14, /* capture the decode graphs of zg_gpt_generate_request_enqueue with edits at create as well: min-p
                                      alone, and the edit stage in front of all four sampler forms (plain, one filter, two filters,
                                      min-p alone), unpenalised; with ZG_GPT_LOGPROBS_ / _STOP_GENERATE beside it their twins too (the
                                      rule: ZG_GPT_SAMPLED_GENERATE; a penalised and edited generation captures its graphs when it begins) */
    ZG_GPT_GUIDED_GENERATE = 1 << 15, /* guided decoding (zg_guide): carve, behind everything else in the arena, the
                                      transition table (256 x vocab uint16), the keep bitmap of every state (256 x ceil(vocab / 32)
                                      words), the row states and the state record — about 27 MB at GPT-2 124M — and capture the guided
                                      twins of every sampler graph that create captures (the rule: ZG_GPT_SAMPLED_GENERATE; a greedy
                                      graph has no guided twin).  Without it zg_gpt_guide_load, zg_gpt_generate_guided_enqueue and
                                      zg_gpt_generate_fetch_guide_states are ZG_ERR_UNSUPPORTED and the handle has bit for bit the layout
                                      and behaviour it has without this flag's existence */
    ZG_GPT_BANNED_GENERATE = 1 << 16, /* capture at create the banned twins (zg_ban_rules) of every sampler graph the other
                                      flags name (the rule: ZG_GPT_SAMPLED_GENERATE; a greedy graph has no banned twin, and there is no
                                      guided + banned twin).  Without it zg_gpt_generate_banned_enqueue works all the same: the graphs
                                      are captured when the generation begins, as for penalties */
    ZG_GPT_BEAM_GENERATE = 1 << 17, /* capture at create the decode graphs of zg_gpt_generate_beam_enqueue (zg_beam_options; DESIGN
                                      §3.14): the one beam tail, which has no twins.  Without it the call works all the same: the
                                      graphs are captured when the generation begins, as for ZG_GPT_BANNED_GENERATE */
    ZG_GPT_WEIGHTS_B24 = 1 << 8 /* store the matrices (wte, wpe, c_attn, c_proj, c_fc, mlp c_proj) as 24-bit floats: each fp32
                                    value rounded to nearest even at 16 mantissa bits (never to inf), row r of an [out][in]
                                    matrix = [in bf16-shaped upper halves | in low bytes].  3/4 of fp32's weight bytes, 2^-17
                                    per weight — for fp32 checkpoints, which bf16 storage takes outside the 1e-3 bound.
                                    Vectors stay fp32.  Excludes ZG_GPT_WEIGHTS_F32 (ZG_ERR_ARG) */
};

/* Per-block tensor slots (load_block, src/main.zig:271-302) and top-level slots (load_gpt,
 * src/main.zig:304-314).  Linear weights are [out, in] like ops.Linear.weight. */
enum {
    ZG_LN_1_G = 0, ZG_LN_1_B, ZG_C_ATTN_W, ZG_C_ATTN_B, ZG_C_PROJ_W, ZG_C_PROJ_B,
    ZG_LN_2_G, ZG_LN_2_B, ZG_C_FC_W, ZG_C_FC_B, ZG_MLP_PROJ_W, ZG_MLP_PROJ_B, ZG_N_BLOCK_SLOTS
};
enum { ZG_WTE = 0, ZG_WPE, ZG_LN_F_G, ZG_LN_F_B, ZG_N_TOP_SLOTS };

/* State.init + load_gpt's allocations (src/main.zig:46-64, :298-299): one device arena holding
 * weights, `batch` private KV caches and all scratch.  batch = number of independent prompts
 * decoded in lock step (the reference supports 1, src/ops.zig:126-128). */
int zg_gpt_create(zg_gpt** out, const zg_gpt_config* config, size_t batch, unsigned flags);
int zg_gpt_destroy(zg_gpt* g);
/* Independent prompt GROUPS on one GPU (no reference counterpart: the reference decodes one sequence, src/ops.zig:126-128).
 * A decode step is a chain of dependent launches that leaves the chip idle across every launch boundary, and prompts are
 * independent units — so instead of one handle of 8 sequences in lock step, G handles of 8/G sequences each run their chains
 * side by side: own_stream gives a handle a private stream (stream_priority: 0 normal, > 0 high, < 0 low — streams of
 * different priorities never share a hardware queue), share_weights_with lets it read the weight region of another handle of
 * the same config and weight flags instead of holding a copy (that handle loads / broadcasts the weights and must be destroyed
 * last).  A handle with a private stream runs without the side-stream L2 prefetcher unless ZGPT2_PREFETCH=1 forces it (the
 * prefetcher's placement assumes one chain on the chip).  zg_gpt_create(...) == zg_gpt_create_ex(..., NULL). */
typedef struct {
    zg_gpt* share_weights_with; /* NULL: own weight region */
    int own_stream;             /* 0: the library stream (zg_set_stream applies); 1: a private stream made here */
    int stream_priority;
} zg_gpt_options;
int zg_gpt_create_ex(zg_gpt** out, const zg_gpt_config* config, size_t batch, unsigned flags, const zg_gpt_options* options_or_null);
/* The hipStream_t a handle launches on (its private stream, or the library stream of the moment). */
int zg_gpt_stream(zg_gpt* g, void** hip_stream_out);

/* Weight upload (replaces load_linear/load_layer_norm/load_embedding, src/main.zig:210-269).
 * src is fp32, host or device; matrices are converted to the arena's storage type on device. */
int zg_gpt_load_block_tensor(zg_gpt* g, size_t layer, int slot, const float* src, size_t len);
int zg_gpt_load_tensor(zg_gpt* g, int slot, const float* src, size_t len);

/* The weight region of the arena (for an RCCL broadcast to the other GPUs of a node). */
int zg_gpt_weight_arena(zg_gpt* g, void** device_ptr, size_t* bytes);
/* Multi-GPU (no reference counterpart — the reference is single-device): prompts are independent units, sharded
 * over ONE PROCESS PER GPU; the weights are replicated by one RCCL broadcast over xGMI, nothing is exchanged while tokens are
 * generated.  The host program (src/main.zig's role) starts one process per GPU; rank 0 makes the id, hands its 128 bytes to
 * the other ranks by any means (file, pipe, environment), every rank calls zg_init(its device) and zg_dist_init; rank 0 loads
 * the weights (zg_gpt_load_*), every rank calls zg_gpt_broadcast_weights on its handle of the same config and flags, then
 * generates its own prompts.  zg_dist_allgather collects equal-sized device buffers (the ranks' token matrices) in rank
 * order.  RCCL is bound at run time: on a box without librccl.so these return ZG_ERR_UNSUPPORTED, everything else works. */
#define ZG_DIST_ID_BYTES 128
/* Not a collective: ZG_OK when RCCL can be bound in this process.  zg_dist_init is a rendezvous — every rank must enter it or
 * none — so a launcher lets its ranks agree on this answer first (bench.py does, over torch.distributed). */
int zg_dist_available(void);
int zg_dist_unique_id(void* id_out, size_t id_bytes);
int zg_dist_init(const void* id, size_t id_bytes, int rank, int world_size);
int zg_dist_world(int* rank, int* world_size); /* world_size 0: no communicator */
int zg_gpt_broadcast_weights(zg_gpt* g, int root, float* ms_out_or_null);
int zg_dist_allgather(const void* send_device, void* recv_device, size_t bytes_per_rank);
int zg_dist_finalize(void);

/* Bytes one decode step must read at sequence length T: weights + KV. */
int zg_gpt_step_bytes(zg_gpt* g, size_t seq_len, size_t* weight_bytes, size_t* kv_bytes);

/* GPT.forward — src/main.zig:178-195, for all `batch` sequences at once: tokens[b] is fed at
 * position seq_len-1.  If logits_out != NULL (host or device, [batch, vocab]) it receives
 * state.logits and the call is synchronous; compute_logits == 0 skips lm_head (main.zig:192).
 * seq_len == 1 starts a new sequence: the KV caches are cleared first (so are they by zg_gpt_prefill and zg_gpt_generate_*) —
 * the reference's State is zero-initialised once and never reads a row it has not written; here the decode attention reads
 * the rows of its whole 64-position bucket with weight 0, and a NaN left behind by an earlier sequence must not survive. */
int zg_gpt_forward(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens,
                   int compute_logits, float* logits_out, size_t logits_len);
/* The prompt loop of generate (src/main.zig:331-334: gpt.forward(i + 1, prompt[i], ...) for every prompt
 * position) as ONE pass: positions 0..n_tokens-1 of all `batch` sequences go through each Block together
 * (Linears as matrix-core GEMMs, causal attention), filling the KV caches exactly as n_tokens calls of
 * zg_gpt_forward would.  tokens is [batch][token_stride].  With compute_logits != 0 the logits of position
 * n_tokens-1 are produced as zg_gpt_forward(n_tokens, ...) would (zg_gpt_argmax / logits_out as there).
 * Afterwards decoding continues with zg_gpt_forward(n_tokens + 1, ...).  Both weight modes: bf16-weight handles multiply the
 * exact three-plane split of the activations with the weights, ZG_GPT_WEIGHTS_F32 handles split both operands (six plane
 * products: fp32-sgemm grade).  Not available on handles created with ZG_GPT_NO_PREFILL. */
int zg_gpt_prefill(zg_gpt* g, const size_t* tokens, size_t token_stride, size_t n_tokens,
                   int compute_logits, float* logits_out, size_t logits_len);
/* ---- Continuing a sequence from its KV cache.  The handle records how many positions its caches hold (all `batch`
 * sequences in lock step): zg_gpt_forward sets the count to seq_len, zg_gpt_prefill / zg_gpt_extend to the end of their pass, the
 * generate calls to the last position they fed.  A continuation names the position it starts at: past_len beyond the recorded count
 * is ZG_ERR_ARG; past_len below it is a rollback — the positions from past_len on are discarded (the cache rows behind the
 * continuation are cleared, the rows below past_len are untouched).  None of these calls allocates. */
int zg_gpt_cached_len(zg_gpt* g, size_t* len_out);
/* zg_gpt_prefill at an offset: tokens [batch][token_stride], n_tokens >= 1 of each row go to positions past_len .. past_len +
 * n_tokens - 1 in ONE pass; the caches end up as n_tokens calls of zg_gpt_forward(past_len + i + 1, ...) would leave them.
 * compute_logits: the logits of the last new position (zg_gpt_argmax / logits_out as zg_gpt_prefill).  past_len == 0 is exactly
 * zg_gpt_prefill.  past_len + n_tokens <= context_size.  Not available on handles created with ZG_GPT_NO_PREFILL. */
int zg_gpt_extend(zg_gpt* g, size_t past_len, const size_t* tokens, size_t token_stride, size_t n_tokens, int compute_logits, float* logits_out,
                  size_t logits_len);
/* argmax of the logits of the last zg_gpt_forward(compute_logits=1) per sequence (lowest index
 * wins ties; logits that are all NaN give index 0) — the greedy replacement for GPT.sample (src/main.zig:198-207). */
int zg_gpt_argmax(zg_gpt* g, size_t* tokens_out, size_t n_tokens);
/* Diagnostic (tests): zg_gpt_forward(seq_len, tokens, compute_logits = 1) with every launch class of the step tapped.  The step is
 * launched eagerly on the handle's stream (no graph) with the arguments, plans and launch ids of a plain step; behind each launch
 * class device-to-device copies on the same stream save what it wrote, raw, in the storage the handle's modes use.  arena_out
 * (host) receives the copies, table_out one zg_tap_entry per copy, in launch order; info[ZG_TAP_INFO_INTS]: activation planes on,
 * tile statistics on, tagged hand-overs on, fused batch-1 launch on, max attention splits, lm_head grid, t_hi of the step, KV mode
 * (0 fp32, 1 fp16, 2 B24), weight type (0 bf16, 1 fp32, 2 B24).  arena_out == NULL: nothing runs; *arena_used and *n_entries
 * report what a call needs.  Classes: -1 the layer's caches as the step finds them, 0 embed, 1 ln_1 + c_attn, 2 attention,
 * 3 attn c_proj, 4 ln_2 + c_fc, 5 mlp c_proj, 6 lm_head.  What is tapped:
 *   0, 3, 5  x [B][E]; planes on: xp (plane layout, element (p, m, k) at (((k >> 5) * 3 + p) * 8 + m) * 32 + (k & 31), 3 x 8 x E
 *            bf16) and, statistics on, xst [8][E / 16][2] (sum, sum of squares).  Behind class 5 of the last layer the planes and
 *            statistics are tapped with ZG_TAP_NOT_WRITTEN: that launch must leave them alone
 *   -1, 1    K and V rows of positions < seq_len, [B][H][seq_len][64]: fp32, fp16, or B24 as a bf16 plane (ZG_TAP_K / _V) and a
 *            byte plane (ZG_TAP_K_LO / _V_LO); class 1 also q [B][E]
 *   2        planes off: the attention partials [B][H][max_splits][66] (o[64], m, l; splits at or beyond ceil(t_hi / 256) are not
 *            written); planes on: the merged heads ap (plane layout)
 *   4        h4 [B][4 E], or planes on: hp (plane layout, 3 x 8 x 4 E)
 *   6        logits [B][V], and the argmax partials (value, index) [B][lm_head grid]
 * ZG_TAP_FUSED: classes 1 and 2 ran as the one batch-1 launch (attn_qkv): both are tapped behind it; it writes q, the new K / V
 * rows and the partials as the two launches do. */
typedef struct zg_tap_entry {
    int cls, layer, buffer, type; /* ZG_TAP_X ..., ZG_TAP_F32 ... */
    size_t offset, count;         /* bytes from the arena's start, elements */
    unsigned flags, pad;
} zg_tap_entry;
enum { ZG_TAP_X = 0, ZG_TAP_XP, ZG_TAP_XST, ZG_TAP_Q, ZG_TAP_K, ZG_TAP_K_LO, ZG_TAP_V, ZG_TAP_V_LO, ZG_TAP_PART, ZG_TAP_AP, ZG_TAP_H4, ZG_TAP_HP,
       ZG_TAP_LOGITS, ZG_TAP_PART_VAL, ZG_TAP_PART_IDX,
       /* zg_debug_gpt_pass_taps only */ ZG_TAP_A, ZG_TAP_QKV_KV, ZG_TAP_PLAN, ZG_TAP_GEO };
enum { ZG_TAP_F32 = 0, ZG_TAP_F16, ZG_TAP_BF16, ZG_TAP_U8, ZG_TAP_I32 };
#define ZG_TAP_FUSED 1u
#define ZG_TAP_NOT_WRITTEN 2u
#define ZG_TAP_INFO_INTS 9
int zg_debug_gpt_step_taps(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, void* arena_out, size_t arena_bytes, size_t* arena_used,
                           zg_tap_entry* table_out, size_t table_len, size_t* n_entries, int* info, size_t n_info);
/* Diagnostic (tests): the whole-prompt pass with every launch tapped — zg_gpt_extend(past_len, tokens, compute_logits, logits_out)
 * (past_len 0: zg_gpt_prefill), or with score != 0 zg_gpt_score(past_len, tokens, top_n, logits_out [batch][n][vocab]) on a
 * ZG_GPT_SCORE handle — with the arguments, plans and launches of the plain call; behind each launch device-to-device copies on
 * the same stream save what it wrote, raw.  The same zg_tap_entry table as zg_debug_gpt_step_taps, in launch order.  arena_out ==
 * NULL: nothing runs; *arena_used and *n_entries report an upper bound of what a call needs (a call returns what it used).
 * Rows are ordered (sequence, new position): M = batch * n_tokens rows, row b n + t at position past_len + t.  A plane buffer is
 * row-major [M][3 K] bf16: the hi, mid and lo plane of a row side by side.  T = min(context, past_len + n_tokens +
 * ZG_PASS_TAP_ROWS_BEHIND).  Classes and what is tapped (layer: the Block; class 7: the 256-row block of the score stage):
 *   -1  in front of c_attn: the layer's K / V rows of positions < T as the pass finds them, [B][H][T][64] in storage format
 *       (ZG_TAP_K / _V and, B24, ZG_TAP_K_LO / _V_LO as in the step taps); the rows at and behind past_len are what an earlier
 *       call or the clearing left
 *    0  embed: x = pf_x [M][E] fp32
 *    1  the first LayerNorm + split: a = pf_a [M][3 E] planes (the ln_1 planes of later Blocks are class 6 of the Block before)
 *    2  c_attn: its plan; q [M][E] fp32 and qkv_kv [M][2 E] fp32, the q and the k | v columns of pf_qkv — ZG_TAP_NOT_WRITTEN on
 *       qkv_kv where the epilogue stores those columns to the cache alone (the persistent GEMM with an fp32 cache); the K / V
 *       rows of positions < T, which now hold the appended rows past_len .. past_len + n_tokens - 1
 *    3  attention (+ merge): geo = 3 ints — the geometry word (key tiles per range | max splits << 8 | query groups << 16), the
 *       kernel (0 the whole-prompt kernel, 1 / 2 / 3 the continuation kernel for an fp32 / fp16 / B24 cache), merge kernel
 *       launched; a = pf_a [M][3 E] planes of the heads
 *    4  attn c_proj + residual (and its tail): its plan; x; a = the ln_2 planes
 *    5  c_fc + GELU + split: its plan; hp = pf_h [M][12 E] planes
 *    6  mlp c_proj + residual (and its tail): its plan; x; a = the next Block's ln_1 planes, ZG_TAP_NOT_WRITTEN in the last Block
 *    7  score: layer 0 first a = the ln_f planes of all rows; then per block each lm_head GEMM's plan (fp32 / B24 weights: one;
 *       bf16: the whole 64-row groups of wte, then the strip) and logits = the block's rows of sc_logits [rows][V64] fp32
 * plan: the ZG_PREFILL_PLAN_INTS ints of zg_debug_prefill_plan, of the plan the launch used.  A pass whose last Block stops behind
 * its cache append (compute_logits == 0) taps nothing behind class 2 of that Block.
 * info[ZG_PASS_INFO_INTS]: activation planes multiplied (2 or 3), KV mode, weight type, pf_ws_floats, stream-K operands given
 * to c_attn, V64 (the vocabulary on the score GEMMs' 64-column grid), rows of a score block. */
#define ZG_PASS_TAP_ROWS_BEHIND 4
#define ZG_PASS_INFO_INTS 7
int zg_debug_gpt_pass_taps(zg_gpt* g, size_t past_len, const size_t* tokens, size_t token_stride, size_t n_tokens, int compute_logits, int score, size_t top_n,
                           float* logits_out, size_t logits_len, void* arena_out, size_t arena_bytes, size_t* arena_used, zg_tap_entry* table_out,
                           size_t table_len, size_t* n_entries, int* info, size_t n_info);
/* Diagnostic (tests): the hand-over state that changes only over a handle's lifetime ("What ages").  A decode tag is
 * (device epoch << 8 | launch id): 24 bits of the step counter the embed kernel advances; the host counts the steps it enqueues
 * and zeroes the tagged words every 2^23 of them.  The stream-K c_attn GEMM of the whole-prompt pass stamps its flag words with a
 * per-launch epoch of 32 bits.
 * zg_debug_gpt_age: act as if n_steps decode steps had been enqueued and run, none of which wrote a tagged slot — the host's
 * own counting and clearing rule runs for n_steps, and a one-thread kernel on the handle's stream adds n_steps (mod 2^32) to the
 * device epoch.  A handle with neither tagged hand-overs nor the fused launch has no such state: nothing happens.  set_sk_epoch
 * != 0 (any handle): the epoch the next stream-K launch is handed follows sk_epoch.
 * zg_debug_gpt_age_state: drains the stream; out[ZG_AGE_STATE_WORDS] = device epoch word, steps counted since the tagged words
 * were last zeroed, steps counted in total, clears of the tagged words enqueued, the stream-K epoch last handed to a launch (or
 * set), restarts of the stream-K epoch (its flag words zeroed on the stream).
 * zg_debug_gpt_tag_census: drains the stream, copies the words to the host and counts there: counts[0..2] = words of the split-K
 * tags, the attention-partial tags and the fused launch's q / k / v tags whose tag is valid (launch id != 0) and carries epoch24
 * in its epoch field; counts[3] = stream-K flag words equal to sk_flag_value (0 on a handle without a whole-prompt path). */
#define ZG_AGE_STATE_WORDS 6
int zg_debug_gpt_age(zg_gpt* g, size_t n_steps, int set_sk_epoch, unsigned sk_epoch);
int zg_debug_gpt_age_state(zg_gpt* g, unsigned long long* out, size_t n_out);
int zg_debug_gpt_tag_census(zg_gpt* g, unsigned epoch24, unsigned sk_flag_value, size_t* counts, size_t n_counts);
/* GPT.sample — src/main.zig:198-207 for all sequences: zg_gpt_forward(seq_len, tokens, logits), then
 * logits /= temp, softmax, and an index drawn with probability proportional to the result
 * (std.rand weightedIndex: first index whose running sum exceeds u * total).  The reference re-seeds
 * its PRNG from the wall clock on every call; here the uniforms u[b] in [0,1) are supplied by the
 * caller (uniforms == NULL: derived from `seed`, seq_len and b with the library's counter PRNG), so a
 * run is reproducible.  probs_out (host or device, [batch, vocab]) optionally receives the softmax. */
int zg_gpt_sample(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, float temp,
                  const float* uniforms, uint64_t seed, size_t* tokens_out, float* probs_out, size_t probs_len);

/* ln_f output of the last forward, [batch, n_embed] (state.x, main.zig:189): of the last zg_gpt_forward / zg_gpt_sample* step,
 * of the last position of a zg_gpt_prefill / zg_gpt_extend / zg_gpt_score pass, of the last step of a generation.  The device
 * keeps the residual stream in front of ln_f (ln_f runs folded into lm_head), so the vector is computed here, out of place:
 * what the next zg_gpt_argmax, step or continuation reads is untouched.  Behind a pass without logits — whose last Block stops
 * at its cache append — this call runs the rest of that Block first, from what the pass left in the handle and with the weights
 * the handle holds at that moment: a zg_gpt_load_* between such a pass and this call is the caller's to avoid.  Drains the handle's
 * stream; no step or pass pays for it. */
int zg_gpt_hidden(zg_gpt* g, float* x_out, size_t len);

/* generate — src/main.zig:322-342 with greedy argmax instead of the sampler, for `batch`
 * prompts in lock step.  prompts is [batch, prompt_stride] (usize), prompt_lens[b] >= 1 tokens
 * are used from row b.  Runs n_steps (<= context_size; the reference always runs context_size,
 * main.zig:330) decode steps without any host round trip per token; out_tokens [batch, n_steps]
 * receives the token after every step (prompt tokens included, main.zig:339-340).
 * As in the reference the last prompt token is fed twice (main.zig:334,337). */
int zg_gpt_generate_greedy(zg_gpt* g, const size_t* prompts, size_t prompt_stride,
                           const size_t* prompt_lens, size_t n_steps, size_t* out_tokens,
                           size_t out_len);
/* Asynchronous form used by the benchmark: enqueue the same n_steps on the stream and return;
 * results stay on the device until zg_gpt_generate_fetch. */
int zg_gpt_generate_enqueue(zg_gpt* g, const size_t* prompts, size_t prompt_stride,
                            const size_t* prompt_lens, size_t n_steps);
int zg_gpt_generate_fetch(zg_gpt* g, size_t n_steps, size_t* out_tokens, size_t out_len);
/* generate AS THE REFERENCE RUNS IT (src/main.zig:322-342 with GPT.sample, :198-207, temp 0.8 in main): every token behind the prompt is
 * drawn — softmax(logits / temp), first index whose running sum exceeds u x total — with the whole loop on the device (the sampler
 * is a node of the captured decode step).  The reference re-seeds from the wall clock per token; here the uniform of (sequence b,
 * position T) is the library's counter PRNG of (seed, T, b), the one zg_gpt_sample uses for uniforms == NULL: the call returns
 * exactly the tokens of the host loop `tok = zg_gpt_sample(g, T, &tok, 1, temp, NULL, seed, ...)`, without a host round trip per
 * token (4.6 k tokens/s at 124M; the per-token call: 4.0 k).  Results through zg_gpt_generate_fetch. */
int zg_gpt_generate_sample_enqueue(zg_gpt* g, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens, size_t n_steps,
                                   float temp, uint64_t seed);
int zg_gpt_generate_sample(zg_gpt* g, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens, size_t n_steps, float temp,
                           uint64_t seed, size_t* out_tokens, size_t out_len);
/* Sampler options of the *_ex calls: per call here, per row through zg_row_sampling.  temp > 0.  top_k: keep the top_k largest logits of a row
 * (0 or >= vocab: off).  top_p in (0, 1]: of what top-k kept, keep the smallest set of largest logits whose probability mass
 * reaches top_p (1: off) — the sequential order HF, vLLM and llama.cpp use.  For a row x: tau_k = the k-th largest value counting
 * duplicates; e = exp(x / temp - max / temp) over K = { x >= tau_k }; tau_p = the largest value v of K with
 * sum{ e : x >= v } >= top_p * sum{ e : K }; kept = { x >= max(tau_k, tau_p) }.  Ties at a threshold are all kept (the result never
 * depends on a sort order; -0.0 and +0.0 are a tie), the most probable token always is.  The draw is zg_gpt_sample's over the
 * kept weights (dropped indices weigh 0); probabilities are renormalised, exactly 0 where dropped.  The thresholds are found
 * exactly (a radix select on the device, integer sums): the same inputs give the same tokens on every run.  A row holding a
 * NaN gives some token < vocab. */
typedef struct {
    float temp;
    size_t top_k;
    float top_p;
} zg_sample_options;
/* zg_gpt_sample with options.  Both filters off: exactly zg_gpt_sample (bit-identical tokens and probabilities).  Bad options
 * (NULL, temp <= 0, top_p <= 0, > 1 or NaN): ZG_ERR_ARG before anything is enqueued. */
int zg_gpt_sample_ex(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, const zg_sample_options* options,
                     const float* uniforms, uint64_t seed, size_t* tokens_out, float* probs_out, size_t probs_len);
/* zg_gpt_generate_sample_* with options: the device loop with the selection kernels in front of the sampler node (graphs of
 * their own: ZG_GPT_TRUNCATED_GENERATE; the option values live in device memory, one graph serves them all).  Returns exactly the
 * tokens of the host loop over zg_gpt_sample_ex(..., options, NULL, seed, ...).  Both filters off: zg_gpt_generate_sample_*
 * itself.  Bad options: ZG_ERR_ARG before anything is enqueued.  Results through zg_gpt_generate_fetch. */
int zg_gpt_generate_sample_ex_enqueue(zg_gpt* g, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens, size_t n_steps,
                                      const zg_sample_options* options, uint64_t seed);
int zg_gpt_generate_sample_ex(zg_gpt* g, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens, size_t n_steps,
                              const zg_sample_options* options, uint64_t seed, size_t* out_tokens, size_t out_len);
/* generate (src/main.zig:322-342) entered at s = past_len with `prompts` = the new tokens of each row: positions past_len ..
 * past_len + n_steps - 1; prompt_lens[b] >= 1 new tokens are fed first (the last of them twice, as main.zig:334,337 does in the first
 * turn too), the rest is picked.  options NULL: greedy; otherwise the sampler of zg_gpt_generate_sample_ex (uniform of (seed,
 * absolute T, b)).  past_len + n_steps <= context_size.  Works on ZG_GPT_NO_PREFILL handles (through the decode loop). */
int zg_gpt_generate_from_enqueue(zg_gpt* g, size_t past_len, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens,
                                 size_t n_steps, const zg_sample_options* options_or_null, uint64_t seed);
/* ---- Penalties on tokens the sequence already holds: per call here, per row through zg_row_sampling.  Let x be a logit of a row
 * and c the number of times its index occurs in that row's history:
 *   c == 0: x is untouched, bit for bit.
 *   c >= 1: y = (x > 0 ? x / repetition : x * repetition); y = y - (presence + frequency * (float)c) — four separately rounded fp32
 *           operations, the division correctly rounded, nothing contracted into an fma: bitwise the same expression in numpy
 *           float32.  -0.0, +0.0 and negative logits take the product; a NaN logit stays NaN.
 * Each distinct token is penalised exactly once however often it occurs (HF's gather-and-scatter; repetition is the CTRL / HF
 * repetition_penalty, presence and frequency are the OpenAI-style pair).  Counts are exact integers: the same inputs give the same
 * tokens on every run.  The penalties act on the raw logits, before temperature, top-k and top-p (HF's order); everything behind
 * them is the sampler of zg_gpt_sample_ex on the penalised row.  repetition > 0 (1: off), presence and frequency finite (0: off),
 * else ZG_ERR_ARG.  All three off: the call is exactly its unpenalised twin — identical tokens and probabilities, no launch added, the
 * same graphs.  A history can hold at most context_size tokens, and the counting kernel keeps a row's distinct tokens in an LDS table
 * of twice that many slots: handles with context_size > 8192 get ZG_ERR_UNSUPPORTED from these entry points (every GPT-2: 1024). */
typedef struct {
    float repetition; /* > 0; 1 = off.  CTRL / HF: x > 0 ? x / r : x * r */
    float presence;   /* 0 = off.  x -= presence for a token that occurs in the history */
    float frequency;  /* 0 = off.  x -= frequency * count */
} zg_logit_penalties;
/* zg_gpt_sample_ex with the penalty stage in front.  The caller passes the history: history [batch][history_stride] (host),
 * history_lens[b] tokens of row b (history may be NULL when every length is 0).  options and penalties must be non-NULL; greedy
 * picking with penalties is top_k = 1.  NULL or bad penalties: ZG_ERR_ARG; a length beyond history_stride or context_size, or a
 * token >= vocab: ZG_ERR_SHAPE — before anything is enqueued and before the handle's state (zg_gpt_cached_len included) is touched.
 * zg_gpt_argmax behind this call is the argmax of the penalised row. */
int zg_gpt_sample_pen(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, const zg_sample_options* options,
                      const zg_logit_penalties* penalties, const size_t* history, size_t history_stride, const size_t* history_lens,
                      const float* uniforms, uint64_t seed, size_t* tokens_out, float* probs_out, size_t probs_len);
/* zg_gpt_generate_from_enqueue with penalties (past_len == 0: a fresh generation; the same rules for past_len, rollback and n_steps).
 * When the pick of step s is drawn, the history of row b is prior[b] followed by the tokens recorded at positions past_len .. s - 1:
 * the row's new prompt tokens and every pick so far.  The reference's second feeding of the last prompt token (main.zig:334,337) is
 * not a second occurrence.  Tokens recorded below past_len by earlier calls are not read: a caller who wants them (the second turn
 * of a conversation) passes them as prior [batch][prior_stride] (host), prior_lens[b] tokens of row b; both NULL: no prior.
 * prior_lens[b] <= prior_stride and prior_lens[b] + n_steps <= context_size (the history never outgrows the context), tokens <
 * vocab, else ZG_ERR_SHAPE; bad options / penalties: ZG_ERR_ARG — all before anything is enqueued or the handle's state is touched.
 * Returns exactly the tokens of the host loop over T of zg_gpt_sample_pen(g, T, &tok, ..., history = prior ++ the tokens recorded
 * on [past_len, T - 1), NULL, seed, ...) that feeds the row's own prompt token while the prompt lasts.  The penalty stage is a node
 * of the captured step (graphs of their own: ZG_GPT_PENALIZED_GENERATE); values, past_len and prior live in device memory, so one
 * graph serves them all.  Does not allocate beyond that capture.  Results through zg_gpt_generate_fetch / _fetch_range. */
int zg_gpt_generate_pen_enqueue(zg_gpt* g, size_t past_len, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens,
                                size_t n_steps, const zg_sample_options* options, const zg_logit_penalties* penalties,
                                const size_t* prior_or_null, size_t prior_stride, const size_t* prior_lens_or_null, uint64_t seed);
/* Test entry: the penalty kernels alone on the caller's rows, logits [batch <= 64, vocab <= 262144] (host or device, as logits_out
 * and counts_out [batch, vocab]: how often each index occurs in its row's history; may be NULL); history and history_lens are host
 * arrays as for zg_gpt_sample_pen, a history of more than 8192 tokens is ZG_ERR_UNSUPPORTED.  Needs zg_init only.  Allocates its
 * workspace per call. */
int zg_debug_penalize_rows(const float* logits, size_t batch, size_t vocab, const zg_logit_penalties* penalties, const size_t* history,
                           size_t history_stride, const size_t* history_lens, float* logits_out, unsigned* counts_out_or_null);
/* ---- Per-token log-probabilities and top-N alternatives from the device loop.  Step p (sequence length p + 1)
 * records the pick of column p of row b.  Let x be that row of logits as the sampler stage receives it: the raw lm_head output, or,
 * in a penalised generation, the row as the penalties leave it — always at temperature 1 and before any truncation (OpenAI and
 * vLLM report the same: what the model, with the caller's penalties, thought — not what the sampler's temperature and filters
 * made of it; with penalties off it is the model's own distribution).  With m = max x and S = sum exp(x_i - m):
 *   logprob[b][p]         = (x[tok] - m) - log S, tok the token column p records.
 *   top_ids[b][p][j]      = the indices of the top_n largest x, value descending, index ascending on ties (-0.0 and +0.0 tie, -inf
 *                           is an ordinary value); exact, comparisons only.
 *   top_logprobs[b][p][j] = the same expression for top_ids[b][p][j] with the same m and S: where the id is tok, bit for bit logprob.
 * A column that records a prompt token (p < past_len + prompt_lens[b], the whole-prompt pass included) reads logprob = NaN and its
 * ids mean nothing.  A row holding NaN or +inf gives unspecified values; its ids are still < vocab and nothing faults.  All sums run
 * in a fixed order without atomics: the same inputs give the same bits on every run.  fp32 throughout: within
 * 1e-5 + 2.5e-7 |logprob| of the float64 value.  top_n in 0 .. ZG_LOGPROBS_TOP_MAX and <= vocab_size, else ZG_ERR_ARG before anything
 * is enqueued or the handle's state is touched. */
#define ZG_LOGPROBS_TOP_MAX 20
/* zg_gpt_generate_pen_enqueue / _from_enqueue with the log-probability stage.  options NULL: greedy (penalties must be NULL then,
 * else ZG_ERR_ARG; greedy with penalties is top_k = 1).  penalties NULL or all off: none.  Tokens are exactly those of the same
 * call without log-probabilities.  Two more launches per step in graphs of their own (ZG_GPT_LOGPROBS_GENERATE); top_n lives in
 * device memory, one graph serves every value.  Does not allocate beyond that capture. */
int zg_gpt_generate_logprobs_enqueue(zg_gpt* g, size_t past_len, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens,
                                     size_t n_steps, const zg_sample_options* options_or_null, const zg_logit_penalties* penalties_or_null,
                                     const size_t* prior_or_null, size_t prior_stride, const size_t* prior_lens_or_null, uint64_t seed,
                                     size_t top_n);
/* Columns first .. first + n - 1, as zg_gpt_generate_fetch_range: logprobs_out [batch, n]; top_ids_out / top_logprobs_out
 * [batch, n, top_n] (both NULL when top_n == 0).  top_n above the recording generation's, or no log-probability generation
 * since the last generation without: ZG_ERR_ARG.  Columns below a continuation's past_len hold what earlier calls recorded. */
int zg_gpt_generate_fetch_logprobs(zg_gpt* g, size_t first, size_t n, size_t top_n, float* logprobs_out, size_t logprobs_len,
                                   size_t* top_ids_out, float* top_logprobs_out, size_t top_len);
/* Test entry: the two kernels alone on the caller's rows, logits [batch <= 64, vocab <= 262144] and tokens [batch] (host or
 * device), a small kernel standing in for lm_head's partials as in zg_debug_sample_rows.  A workgroup of the first kernel owns 1024
 * consecutive elements of a row.  top_n > 20 or > vocab: ZG_ERR_ARG; a token >= vocab: ZG_ERR_SHAPE.  Needs zg_init only. */
int zg_debug_logprob_rows(const float* logits, size_t batch, size_t vocab, const size_t* tokens, size_t top_n, float* logprobs_out,
                          size_t* top_ids_out_or_null, float* top_logprobs_out_or_null);
/* ---- Scoring a given text: the pass of zg_gpt_extend(g, past_len, tokens, token_stride, n_tokens, compute_logits = 1,
 * NULL, 0) — the same checks, rollback rule, launches, cache effect and refusal on ZG_GPT_NO_PREFILL; zg_gpt_argmax and a generation
 * continued behind it behave as behind zg_gpt_extend, bit for bit — which also records, for every position it feeds, how likely
 * the token there was.  Row b of the pass at position p (past_len <= p < past_len + n_tokens - 1) holds the logits x that predict
 * position p + 1; with tok = tokens[b][p + 1 - past_len], column p + 1 of row b of the log-probability record receives
 *   logprob = (x[tok] - m) - log S  and  top_ids / top_logprobs of that x,
 * m, S, the order of the ids and the bit-for-bit equality where an id is tok exactly as defined above for the device loop.  Column
 * past_len reads NaN: its predicting row is not part of the pass — to score a continuation behind a cached context, or the second
 * chunk of a long text, roll back by one: past_len = len - 1 and the last cached token first.  Columns below past_len keep what
 * earlier calls recorded.  The call counts as a log-probability generation with this top_n: the results leave through
 * zg_gpt_generate_fetch_logprobs, and zg_gpt_generate_logprobs_enqueue(past_len = the end, ...) behind it continues the same record.
 * top_n in 0 .. ZG_LOGPROBS_TOP_MAX and <= vocab_size, else ZG_ERR_ARG.  logits_out (host or device, [batch][n_tokens][vocab];
 * logits_len below that: ZG_ERR_SHAPE; may be NULL) receives the logits of every position as the pass computed them — the lm_head
 * of all rows on the matrix cores, 256 rows at a time; the logits of all positions are never held at once.  Needs a handle created
 * with ZG_GPT_SCORE (else ZG_ERR_UNSUPPORTED).  Every refusal happens before anything is enqueued or the handle's state
 * (zg_gpt_cached_len, the record) is touched.  Synchronous; allocates nothing.  fp32 sums in a fixed order without atomics: the same
 * inputs give the same bits on every run, within 1e-5 + 2.5e-7 |logprob| of the float64 value of the pass's own logits. */
int zg_gpt_score(zg_gpt* g, size_t past_len, const size_t* tokens, size_t token_stride, size_t n_tokens, size_t top_n, float* logits_out_or_null,
                 size_t logits_len);
/* Test entry: the two statistics kernels of zg_gpt_score alone on the caller's rows, logits [rows <= 4096][row_stride >= vocab] (host
 * or device, as targets [rows] and the outputs [rows] / [rows, top_n]); only columns < vocab of a row are read.  A workgroup of the
 * first kernel owns 1024 consecutive columns of a row and the row maximum comes from the chunks.  The error codes of
 * zg_debug_logprob_rows: top_n > 20 or > vocab, or a bad argument: ZG_ERR_ARG; a target >= vocab: ZG_ERR_SHAPE.  Needs zg_init only.
 * Allocates its workspace per call. */
int zg_debug_score_rows(const float* logits, size_t rows, size_t vocab, size_t row_stride, const size_t* targets, size_t top_n, float* logprobs_out,
                        size_t* top_ids_out_or_null, float* top_logprobs_out_or_null);
/* ---- Stop tokens and stop sequences in the device loop, with an early end.
 * Matching.  Row b picks the tokens of columns p >= past_len + prompt_lens[b]; columns below that record prompt tokens.  The
 * conditions are numbered over the concatenated list: j < n_ids is stop token ids[j], n_ids + k is stop sequence k (seq_lens[k]
 * tokens at seqs + k * seq_stride).  Condition j matches at column p of row b when p is a picked column and either it is a stop
 * token and the token recorded at p equals ids[j], or it is a stop sequence of L tokens, columns p - L + 1 .. p are ALL picked
 * columns of the row and hold the L tokens of the sequence — a match never reaches into the prompt (OpenAI and vLLM match generated
 * text only).  finish_col[b] is the lowest column at which any condition matches and reason[b] the lowest j matching there; a row
 * that never matches has finish_col[b] = ZG_STOP_NONE and reason[b] = -1.  Once a row has finished its values do not change.
 * Matching is exact integer comparison of recorded tokens: the same inputs give the same finish_col and reason on every run.
 * The loop.  Rows stay in lock step and a finished row keeps decoding.  The stop stage is one more launch per step, last in the
 * step's tail; it only reads, so every column below `end` holds, bit for bit, the token (and, with log-probabilities, the record)
 * the same call without stop conditions leaves there.  When the last unfinished row finishes at column f the loop is fed no
 * further: the generation ends at `end` (exclusive, absolute) with f + 1 <= end <= min(past_len + n_steps, f + 1 + lookahead + 64);
 * if some row never finishes, end = past_len + n_steps.  `end` may differ from run to run inside that bound; nothing else may.
 * Afterwards zg_gpt_cached_len == end, the caches hold positions < end, zg_gpt_generate_fetch / _fetch_range / _fetch_logprobs serve
 * columns < end (columns from `end` on keep what earlier calls left there), and a continuation rolls back with past_len <= end as
 * after any other call.  The host learns of the device's progress from two words in pinned memory that the stop kernel stores to;
 * it feeds a piece of the loop (up to 64 steps) only while it is at most `lookahead` steps ahead of them, so the device never idles
 * and never waits for the host, and no step costs a host round trip.  lookahead 0: the library's default. */
#define ZG_STOP_MAX_IDS 16
#define ZG_STOP_MAX_SEQS 8
#define ZG_STOP_MAX_SEQ_LEN 16
#define ZG_STOP_NONE ((size_t)-1)
typedef struct {
    const size_t* ids;      size_t n_ids;      /* stop tokens */
    const size_t* seqs;     size_t seq_stride; /* [n_seqs][seq_stride] */
    const size_t* seq_lens; size_t n_seqs;     /* 1..ZG_STOP_MAX_SEQ_LEN tokens each */
    size_t lookahead;                          /* steps the host may run ahead of the device; 0 = the library's default */
} zg_stop_conditions;
/* zg_gpt_generate_logprobs_enqueue's arguments; logprobs == 0: no log-probability stage (top_n ignored).  stop NULL, or n_ids ==
 * n_seqs == 0: exactly zg_gpt_generate_logprobs_enqueue (logprobs != 0) or zg_gpt_generate_pen_enqueue / _from_enqueue (logprobs ==
 * 0) — the same graphs, no added launch, no pacing, end = past_len + n_steps.  n_ids > 16, n_seqs > 8, a sequence length of 0, above
 * 16 or above seq_stride, a NULL array with a non-zero count, greedy with penalties: ZG_ERR_ARG; a stop token or sequence token >=
 * vocab_size: ZG_ERR_SHAPE — all before anything is enqueued or the handle's state (zg_gpt_cached_len, the log-probability record)
 * is touched.  With conditions the call does NOT return immediately: it returns when the last step it will run has been enqueued,
 * at most lookahead + 64 steps of device work before the end.  Graphs of their own (ZG_GPT_STOP_GENERATE); the conditions live in
 * device memory, one graph serves every set.  Does not allocate beyond that capture.  A stop generation runs without a stall strike
 * against the side-stream prefetcher: an early end reaches it as the ordinary end of a generation. */
int zg_gpt_generate_stop_enqueue(zg_gpt* g, size_t past_len, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens,
                                 size_t n_steps, const zg_sample_options* options_or_null, const zg_logit_penalties* penalties_or_null,
                                 const size_t* prior_or_null, size_t prior_stride, const size_t* prior_lens_or_null, uint64_t seed,
                                 int logprobs, size_t top_n, const zg_stop_conditions* stop_or_null);
/* Drains the stream and reports `end`, finish_col [batch] and reason [batch] of the last generation, which must have been one with
 * stop conditions: before any, or behind a generation without, ZG_ERR_ARG. */
int zg_gpt_generate_stop_result(zg_gpt* g, size_t* end_out, size_t* finish_cols_out, int* reasons_out);
/* Test entry: the stop kernel alone.  For s = 0 .. n_cols - 1 it is launched once per column, eagerly, over the caller's host
 * tokens [batch <= 8][stride >= n_cols]: the pick of column s is tokens[b][s] and first_cols[b] plays past_len + prompt_lens[b].
 * done_col_out: the highest finish column + 1, or 0 when some row never finishes.  The refusals of zg_gpt_generate_stop_enqueue on
 * the conditions (a token of 2^31 - 1 or above standing for the vocabulary).  Needs zg_init only.  Allocates per call. */
int zg_debug_stop_rows(const size_t* tokens, size_t batch, size_t stride, const size_t* first_cols, size_t n_cols,
                       const zg_stop_conditions* stop, size_t* finish_cols_out, int* reasons_out, size_t* done_col_out);
/* Test entry: the greedy pick alone.  The caller's host partials part_val / part_idx [batch][n_part] — (maximum, index) pairs as
 * lm_head's argmax epilogue leaves them — go to the device and the decode step's head kernel picks from them in the form
 * zg_gpt_argmax launches: the first pair in the order "greater value first, lower index on ties", starting from (-3.0e38, 2^31 - 1);
 * picks_out [batch] receives its index, or 0 when that is not in [0, vocab).  batch 1 .. 8, n_part 1 .. 4096, vocab 1 .. 2^31 - 1,
 * anything else: ZG_ERR_ARG.  Needs zg_init only.  Allocates per call. */
int zg_debug_pick_rows(const float* part_val, const int32_t* part_idx, size_t batch, size_t n_part, size_t vocab, size_t* picks_out);
/* ---- Edits of the logit row by token id, and min-p: OpenAI / vLLM logit_bias, vLLM allowed_token_ids (HF
 * prefix_allowed_tokens_fn in its static form), vLLM bad_words / HF bad_words_ids for single tokens, and min_p (vLLM, HF, llama.cpp).
 * The three lists are per call; min_p is per call here, per row through zg_row_sampling.
 * Row edit.  Let x be the row as the stage finds it: the raw lm_head output, or the penalised row when the call penalises —
 * penalties come first, then the edits, then temperature, top-k, top-p and min-p (HF's processor and warper order).  With
 * keep[i] = (n_allowed == 0 or i is in allowed_ids) and i is not in banned_ids:
 *   y[i] = keep[i] ? (i in bias_ids ? x[i] + v_i : x[i]) : -inf
 * The addition is one rounded fp32 add: bitwise numpy float32.  An index that is kept and unbiased is untouched bit for bit (-0.0,
 * NaN and -inf stay what they are); a bias on a token that is not kept leaves it -inf.  Everything behind the stage sees y: the
 * sampler, zg_gpt_argmax, the log-probability stage (the logprob of a banned token is -inf; the top-N order treats -inf as an
 * ordinary value) and the stop stage.
 * min-p belongs to the sampler, not to the row (the log-probability record stays at temperature 1 and before truncation).  The host
 * computes once per call d = (float)((double)temp * log((double)min_p)) (-inf when min_p == 0; zg_debug_min_p_offset); on the device
 * tau_m = m + d is one fp32 add, m the row maximum of y, and kept = { y >= max(tau_k, tau_p, tau_m) } with tau_k and tau_p exactly as
 * in zg_sample_options (HF applies min-p last; its test p_i >= min_p * p_max is a ratio, so the renormalisation before it does not
 * matter).  Ties at the threshold stay together, the top token is always kept, probabilities are renormalised and exactly 0 where
 * dropped.  The threshold is comparison-only: the same inputs give the same tokens on every run.
 * Refusals, all before anything is enqueued or the handle's state is touched.  ZG_ERR_ARG: NULL edits where edits are required,
 * n_bias > ZG_EDIT_MAX_BIAS, a duplicate bias id, a non-finite bias value, min_p < 0, >= 1 or NaN, a NULL array with a non-zero
 * count, an empty kept set (both lists are the host's: a row of -inf alone never reaches a kernel), greedy (options == NULL) with
 * any edit on — as with penalties, greedy with edits is top_k = 1.  ZG_ERR_SHAPE: an id >= vocab_size.
 * Everything off (n_bias, n_allowed, n_banned and min_p all 0): the call is exactly its twin without edits — identical tokens,
 * probabilities and records, no added launch, the same graphs.
 * Cost: ONE added launch per step, which edits every row and leaves the row-maximum partials rebuilt from what it wrote; min-p adds
 * none to a truncated sampler and, alone, swaps the sampler's two tail kernels for their threshold-aware twins.  The keep set lives
 * in device memory as a bitmap of vocab_size bits built by the host (the lists have no count limit), the bias as pairs sorted by
 * id; both are read on the device, so one captured graph serves every set. */
#define ZG_EDIT_MAX_BIAS 512
typedef struct {
    const size_t* bias_ids; const float* bias_values; size_t n_bias; /* <= ZG_EDIT_MAX_BIAS, ids distinct, values finite */
    const size_t* allowed_ids; size_t n_allowed;                     /* 0: every token is allowed; any count up to vocab */
    const size_t* banned_ids;  size_t n_banned;                      /* any count; duplicates are harmless */
    float min_p;                                                     /* in [0, 1); 0 = off */
} zg_logit_edits;
/* zg_gpt_sample_pen with the edit stage behind the penalties.  penalties_or_null NULL (history is not read then) or all off: no
 * penalty stage.  options and edits must be non-NULL.  Everything off: zg_gpt_sample_pen / zg_gpt_sample_ex itself, bit for bit.
 * zg_gpt_argmax behind this call is the argmax of the edited row. */
int zg_gpt_sample_edit(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens,
                       const zg_sample_options* options, const zg_logit_penalties* penalties_or_null,
                       const size_t* history, size_t history_stride, const size_t* history_lens,
                       const zg_logit_edits* edits, const float* uniforms, uint64_t seed,
                       size_t* tokens_out, float* probs_out, size_t probs_len);
/* The request form of the generate call, the superset from now on: every argument of zg_gpt_generate_stop_enqueue by name, plus
 * edits.  size must be sizeof(zg_generate_request) (else ZG_ERR_ARG).  edits NULL: zg_gpt_generate_stop_enqueue exactly.  With edits
 * it returns exactly the tokens of the host loop over zg_gpt_sample_edit (history as zg_gpt_generate_pen_enqueue states it).  The
 * edit stage is a node of the captured step (graphs of their own: ZG_GPT_EDITED_GENERATE).  Does not allocate beyond that capture.
 * Results through zg_gpt_generate_fetch / _fetch_range / _fetch_logprobs / _stop_result. */
typedef struct {
    size_t size;
    size_t past_len;
    const size_t* prompts; size_t prompt_stride; const size_t* prompt_lens;
    size_t n_steps;
    const zg_sample_options* options;     /* NULL: greedy */
    const zg_logit_penalties* penalties;  /* NULL: none */
    const size_t* prior; size_t prior_stride; const size_t* prior_lens;
    uint64_t seed;
    int logprobs; size_t top_n;
    const zg_stop_conditions* stop;       /* NULL: none */
    const zg_logit_edits* edits;          /* NULL: none */
} zg_generate_request;
int zg_gpt_generate_request_enqueue(zg_gpt* g, const zg_generate_request* r);
/* ---- Sampling parameters per row.  A handle decodes its rows in lock step, and the rows may belong to different
 * requests: one zg_row_sampling per row carries everything that shapes a pick.  Sequences never interact, so row b of a per-row
 * call is, BIT FOR BIT, row b of the uniform call on the same handle that is given rows[b].options, rows[b].min_p,
 * rows[b].penalties and rows[b].seed for every row — tokens, probabilities, thresholds, the log-probability record, finish columns
 * and reasons.  Every row has the sampler form its own parameters ask for (plain, one filter, both, min-p alone) and that form's
 * arithmetic, whatever its neighbours run; a row whose penalties are off is not touched by the penalty stage.  The chain is
 * launched once for all rows, in the union of their needs: the selection launches of the row that needs most (0 / 3 / 6), the
 * threshold-aware tail if any row has a filter or min-p, the penalty stage if any row is penalised — the graphs of
 * ZG_GPT_TRUNCATED_ / _PENALIZED_ / _EDITED_ / _LOGPROBS_ / _STOP_GENERATE serve these calls as they are.  There is no per-row
 * greedy flag: greedy is top_k = 1 (it differs from zg_gpt_generate_greedy only on exact fp32 ties of the row maximum).
 * Per call, not per row: the edit lists, the stop conditions, top_n, n_steps, past_len and the prior's layout.
 * Refusals, all before anything is enqueued or the handle's state (zg_gpt_cached_len, the records) is touched, the message naming
 * the row.  ZG_ERR_ARG: a row with bad options (temp <= 0, top_p outside (0, 1]), bad penalties or min_p outside [0, 1); n_rows !=
 * the handle's batch; NULL rows; options, penalties or a non-zero edits->min_p given beside rows.  ZG_ERR_UNSUPPORTED: any row
 * penalised on a handle with context_size > 8192. */
typedef struct {
    zg_sample_options options;     /* temp > 0; top_k (0 or >= vocab: off); top_p in (0, 1] (1: off) */
    float min_p;                   /* in [0, 1); 0 = off */
    zg_logit_penalties penalties;  /* {1, 0, 0} = off */
    uint64_t seed;                 /* the row's draws: counter PRNG of (seed, absolute T, b), b the row's index in the handle */
} zg_row_sampling;
/* zg_gpt_generate_request_enqueue with the sampler parameters taken per row: rows [n_rows], n_rows == the handle's batch.
 * r->options and r->penalties must be NULL, r->edits (if given) must have min_p == 0, r->seed is not read; prior, logprobs / top_n,
 * stop, the three edit lists and past_len stay per call and work as there. */
int zg_gpt_generate_each_enqueue(zg_gpt* g, const zg_generate_request* r, const zg_row_sampling* rows, size_t n_rows);
/* zg_gpt_sample_edit with rows (the per-token twin).  uniforms NULL: the draw of row b is the counter PRNG of (rows[b].seed,
 * seq_len, b).  edits_or_null: the three lists (min_p must be 0).  The history is read when any row is penalised. */
int zg_gpt_sample_each(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, const zg_row_sampling* rows, size_t n_rows,
                       const size_t* history, size_t history_stride, const size_t* history_lens, const zg_logit_edits* edits_or_null,
                       const float* uniforms, size_t* tokens_out, float* probs_out, size_t probs_len);
/* Test entries: zg_debug_edit_rows and zg_debug_penalize_rows with one zg_row_sampling per row (n_rows == batch <= 64, vocab <=
 * 262144; edits_or_null: the three lists, min_p 0).  thresholds_out: -inf for a row that truncates nothing.  Need zg_init only. */
int zg_debug_sample_rows_each(const float* logits, size_t batch, size_t vocab, const zg_row_sampling* rows, size_t n_rows,
                              const zg_logit_edits* edits_or_null, const float* uniforms, float* edited_out_or_null, size_t* tokens_out,
                              float* probs_out_or_null, float* thresholds_out_or_null);
int zg_debug_penalize_rows_each(const float* logits, size_t batch, size_t vocab, const zg_row_sampling* rows, size_t n_rows,
                                const size_t* history, size_t history_stride, const size_t* history_lens, float* logits_out,
                                unsigned* counts_out_or_null);
/* What a table of rows is launched as (needs neither a GPU nor zg_init): out[0] = the sampler form of the chain — 1 plain, 2 one
 * filter, 3 two filters, 4 min-p alone —, out[1] = whether the penalty stage runs, out[2 + b] = the form row b itself has; n_out >=
 * 2 + n_rows, n_rows <= 64.  Returns the refusal a call over `vocab` logits would return for the table. */
int zg_debug_each_plan(const zg_row_sampling* rows, size_t n_rows, size_t vocab, int* out, size_t n_out);
/* Test entry: the edit stage and the sampler behind it alone on the caller's rows, logits [batch <= 64, vocab <= 262144] (host or
 * device, as uniforms [batch] and the outputs), a small kernel standing in for lm_head's row-maximum partials.  edited_out
 * [batch, vocab]: the rows as the stage leaves them; tokens_out, probs_out and thresholds_out (max(tau_k, tau_p, tau_m) of each
 * row; -inf when nothing truncates) as zg_debug_sample_rows.  Everything off: zg_debug_sample_rows bit for bit.  Needs zg_init only.
 * Allocates its workspace per call. */
int zg_debug_edit_rows(const float* logits, size_t batch, size_t vocab, const zg_sample_options* options,
                       const zg_logit_edits* edits, const float* uniforms,
                       float* edited_out_or_null, size_t* tokens_out,
                       float* probs_out_or_null, float* thresholds_out_or_null);
/* d of min-p as the library computes it (temp > 0, min_p in [0, 1), else ZG_ERR_ARG).  Needs neither a GPU nor zg_init. */
int zg_debug_min_p_offset(float temp, float min_p, float* d_out);
/* ---- Guided decoding: a token-level automaton in the device loop — "one of these labels", "digits, then a newline",
 * a regex or a JSON schema compiled to a finite-state machine over tokens (Outlines; vLLM guided_choice / guided_regex).  The static
 * form is zg_logit_edits.allowed_ids: one keep set per call.  Here the keep set depends on where in the grammar a row stands.
 * An automaton is n_states states (1 .. ZG_GUIDE_MAX_STATES) and a dense table next [n_states][vocab] of uint16_t:
 * next[s][i] == ZG_GUIDE_DEAD: token i is not allowed in state s; any other value (< n_states) is the state behind picking i.  Every
 * state allows at least one token — a finished row keeps decoding in lock step, and a row of -inf alone never reaches a kernel:
 * "done" is a state that loops on the end token, and ending the generation stays the stop stage's business (stop token ids).  One
 * table may hold several automata in disjoint state ranges: every row names its own start state, so per-row grammars are free.
 * The stage.  state[b] is the row's state when a picked column p (p >= past_len + prompt_lens[b]) is drawn.  The guide comes last
 * among the stages that rewrite the row — penalties, then edits, then the guide, then temperature / top-k / top-p / min-p:
 *   y[i] = next[state[b]][i] != ZG_GUIDE_DEAD ? x[i] : -inf
 * with x the row as the edit stage leaves it; a kept index is not written (its bits are untouched).  Everything behind the stage
 * sees y: the sampler, zg_gpt_argmax, the log-probability record and the stop stage.  Behind the pick tok of that column,
 * state[b] = next[state[b]][tok].  Prompt columns neither mask nor advance.  A row whose start state is ZG_GUIDE_NONE is unguided:
 * the stage does not write it and it keeps its bits beside guided neighbours (its row-maximum partials may be rebuilt in another
 * slicing, as for an unpenalised row of §3.11).  A pick whose transition is dead or out of range can only come from a row holding
 * NaN; it leaves the state unchanged.  Nothing read from device memory becomes an address before it is clamped.
 * The oracle: row b of a guided call returns, BIT FOR BIT — tokens, the log-probability record, finish columns and reasons — what
 * the host loop over zg_gpt_sample_edit (per-row parameters: zg_gpt_sample_each) returns that passes allowed_ids = the call's
 * allow-list intersected with { i : next[state][i] != ZG_GUIDE_DEAD } and walks the automaton itself; at batch > 1 that loop is run
 * once per row on the same handle and that row compared (sequences never interact).
 * Cost: with a guide the tail has one launch in the edit stage's place (or one more where the call has no edits) and one small
 * launch behind the sampler; with edits AND a guide the row is still rewritten by ONE launch.  The table and the bitmaps live in
 * device memory: one captured graph serves every grammar.  There is no per-token twin: a caller who draws token by token has
 * allowed_ids and walks the automaton on the host. */
#define ZG_GUIDE_MAX_STATES 256
#define ZG_GUIDE_DEAD 0xFFFFu
#define ZG_GUIDE_NONE ((size_t)-1)
typedef struct {
    size_t n_states;       /* 1 .. ZG_GUIDE_MAX_STATES */
    const uint16_t* next;  /* [n_states][vocab_size], host memory */
} zg_guide;
/* Check a table, build the keep bitmap of every state on the host, upload both, and keep the host bitmaps for the checks of later
 * calls.  Synchronous (it drains the handle's stream first): the one slow call, once per grammar and not per request.  NULL
 * unloads.  ZG_ERR_ARG: n_states 0 or above ZG_GUIDE_MAX_STATES, NULL next, a transition >= n_states that is not ZG_GUIDE_DEAD, a
 * state that allows nothing (the message names it) — the table the handle held stays loaded.  Needs ZG_GPT_GUIDED_GENERATE. */
int zg_gpt_guide_load(zg_gpt* g, const zg_guide* guide_or_null);
/* zg_gpt_generate_request_enqueue (rows_or_null NULL) or zg_gpt_generate_each_enqueue (rows given; n_rows == the handle's batch)
 * with a guide: start_states [batch], the state each row is in when its first picked column is drawn, or ZG_GUIDE_NONE.  Every
 * other argument follows those calls' rules; zg_generate_request is unchanged.  All start states ZG_GUIDE_NONE: exactly the unguided
 * call — the same graphs, no added launch.  A second turn (past_len > 0) continues a row from next[state[p]][tok[p]] of its last
 * picked column p: the caller computes it from zg_gpt_generate_fetch_guide_states and the tokens, and passes it as the start state.
 * Refusals, all before anything is enqueued or the handle's state is touched.  ZG_ERR_UNSUPPORTED: the handle lacks
 * ZG_GPT_GUIDED_GENERATE.  ZG_ERR_ARG: NULL start_states; a guided row with no table loaded; a start state >= n_states; greedy
 * (options NULL without rows) with any guided row — as with edits, greedy is top_k = 1; an empty kept set: with an allow or ban list
 * beside a guided row, EVERY state of the table (whichever the rows can reach) must keep a token the lists keep. */
int zg_gpt_generate_guided_enqueue(zg_gpt* g, const zg_generate_request* r, const zg_row_sampling* rows_or_null, size_t n_rows,
                                   const size_t* start_states);
/* states_out [batch][n] (len >= batch * n): for columns first .. first + n - 1, the state in which the column's pick was drawn, or
 * ZG_GUIDE_NONE for a prompt column and for an unguided row.  Serves columns < end of the last generation, which must have come
 * through zg_gpt_generate_guided_enqueue (else ZG_ERR_ARG); columns below a continuation's past_len hold what earlier calls recorded. */
int zg_gpt_generate_fetch_guide_states(zg_gpt* g, size_t first, size_t n, size_t* states_out, size_t len);
/* Test entry: the mask kernel — with the edit stage's part in the same launch when edits (the three lists; min_p 0) are given —
 * and then the advance kernel, alone on the caller's rows: logits [batch <= 64][vocab <= 262144] (host or device, as edited_out),
 * states [batch] (ZG_GUIDE_NONE: unguided) and picks [batch] on the host; every row stands at a picked column.  edited_out
 * [batch][vocab]: the rows as the stage leaves them; part_val_out / part_idx_out [batch][n_part], n_part = min(64, ceil(vocab /
 * 256)): the rebuilt partials, slice j = the indices i with (i / 256) mod n_part == j; next_states_out [batch]: the states behind the
 * picks (a pick >= vocab or a dead transition: unchanged).  The refusals of a load and of a call.  Needs zg_init only. */
int zg_debug_guide_rows(const float* logits, size_t batch, size_t vocab, const zg_guide* guide, const size_t* states,
                        const zg_logit_edits* edits_or_null, const size_t* picks, float* edited_out, float* part_val_out,
                        int32_t* part_idx_out, size_t* next_states_out);
/* The refusal zg_gpt_guide_load of `guide` on a handle of `vocab` tokens, followed (n >= 1) by a guided call with these edits, start
 * states [n] and — greedy != 0 — without sampler options would return, or ZG_OK.  Needs neither a GPU nor zg_init. */
int zg_debug_guide_check(const zg_guide* guide, size_t vocab, const zg_logit_edits* edits_or_null, const size_t* start_states, size_t n,
                         int greedy);
/* ---- History-dependent token bans in the device loop: HF no_repeat_ngram_size, multi-token vLLM bad_words / HF
 * bad_words_ids (zg_logit_edits.banned_ids covers single tokens only), and vLLM min_tokens / HF min_new_tokens.  The ban stage sits
 * between the penalties and the edits: for every row it computes, on the device and from the row's history, the set of tokens
 * forbidden at the column in flight, and writes -inf there.  Everything behind it sees the row it leaves: the edits (a bias on a
 * banned token leaves it -inf), the sampler, zg_gpt_argmax, the log-probability record (-inf, an ordinary value in the top-N order)
 * and the stop stage.  -inf masks commute with each other and with the edit stage, so the placement changes no result.
 * The history h[0 .. L) of row b at step s is what zg_gpt_generate_pen_enqueue defines for the penalties, read IN ORDER: prior[b]
 * followed by the tokens recorded at positions past_len .. s - 1 (the second feeding of the last prompt token is not a second
 * occurrence; tokens recorded below past_len are not read).  picked = (column in flight) - (past_len + prompt_lens[b]), negative
 * on a prompt column.
 *   n-gram, n = no_repeat_ngram[b] (0: off; 1 .. ZG_BAN_MAX_NGRAM): if L >= n - 1, for every i in 0 .. L - n with
 *     h[i .. i + n - 1) == h[L - n + 1 .. L), ban h[i + n - 1].  n == 1 bans every token of the history.
 *   bad words: up to ZG_BAN_MAX_WORDS words of 1 .. ZG_BAN_MAX_WORD_LEN tokens, per call; word k is words[k * word_stride ..
 *     + word_lens[k]).  A word w of m tokens bans w[m - 1] when L >= m - 1 and h[L - m + 1 .. L) == w[0 .. m - 1); a word of one
 *     token is always banned.  Unlike a stop sequence, a match may reach into the prompt and the prior (HF's semantics).
 *   min tokens: while 0 <= picked < min_tokens[b], every id of suppress_ids (up to ZG_BAN_MAX_SUPPRESS, per call) is banned.  Stop
 *     SEQUENCES are not affected.
 * A history token >= vocab matches nothing and bans nothing; it never becomes an address.  Several matches may ban the same token:
 * all store the same -inf.  A row whose rules are all off is not written: it keeps its bits (a NaN payload, -0.0) beside active
 * neighbours.
 * The oracle: the device loop returns, token for token, the host loop over zg_gpt_sample_edit / zg_gpt_sample_each that passes
 * banned_ids = the call's own list united with the set above (tests/ban_ref.py; zig_gpt2_amd/bans.py banned_now is the host twin
 * for callers who draw token by token — there is no per-token C entry).
 * Cost: two launches per step (the ban launch and the rebuild of the row-maximum partials), one beside edits, whose launch
 * rebuilds.  The rules live in device memory (about 5 KB) and are read there: one captured graph serves every rule set. */
#define ZG_BAN_MAX_NGRAM 16
#define ZG_BAN_MAX_WORDS 64
#define ZG_BAN_MAX_WORD_LEN 16
#define ZG_BAN_MAX_SUPPRESS 16
typedef struct {
    size_t size;                       /* sizeof(zg_ban_rules), else ZG_ERR_ARG */
    const size_t* no_repeat_ngram;     /* [batch] or NULL (all off) */
    const size_t* words; size_t word_stride; const size_t* word_lens; size_t n_words;
    const size_t* suppress_ids; size_t n_suppress;
    const size_t* min_tokens;          /* [batch] or NULL (all 0) */
} zg_ban_rules;
/* zg_gpt_generate_request_enqueue (rows_or_null NULL) or zg_gpt_generate_each_enqueue (rows given; n_rows == the handle's batch)
 * with the ban stage.  Results through the existing fetch calls.  bans NULL or all off (every n 0, no word, and no suppress id or
 * every min_tokens 0): exactly the call without them — the same graphs, no added launch, identical bits.
 * Refusals, all before anything is enqueued or the handle's state is touched; the message names the row or word.  ZG_ERR_ARG: a
 * wrong size; a NULL array with a non-zero count; n above ZG_BAN_MAX_NGRAM; a word length of 0, above ZG_BAN_MAX_WORD_LEN or above
 * word_stride; counts above the maxima; greedy (options NULL without rows) with any rule on — as with edits, greedy is top_k = 1;
 * and rules that could leave a row without a token: with kept the size of the call's static keep set (vocab_size without allow /
 * ban lists) and D(b) = (n_b > 0 ? min(prior_lens[b] + n_steps, vocab_size) : 0) + n_words + (min_tokens[b] > 0 ? n_suppress : 0),
 * the call is refused when kept < 1 + max_b D(b) — a conservative bound: a row of -inf alone never reaches a kernel.  ZG_ERR_SHAPE: a
 * word or suppress token >= vocab_size.  ZG_ERR_UNSUPPORTED: context_size > 8192 (the history sits in the LDS, as for the
 * penalties).  A guide goes through its own entry: bans and a guide cannot be combined (a grammar compiles its bad words into the
 * table). */
int zg_gpt_generate_banned_enqueue(zg_gpt* g, const zg_generate_request* r, const zg_row_sampling* rows_or_null, size_t n_rows,
                                   const zg_ban_rules* bans);
/* The refusal a banned call with these rules on a handle of `batch` rows, `vocab` tokens and `context` positions would return —
 * with these edits, n_steps and prior lengths (NULL: none), greedy != 0: without sampler options, guided != 0: beside a guided row
 * (ZG_ERR_ARG) — or ZG_OK.  Needs neither a GPU nor zg_init. */
int zg_debug_ban_check(const zg_ban_rules* bans, size_t batch, size_t vocab, size_t context, const zg_logit_edits* edits_or_null,
                       size_t n_steps, const size_t* prior_lens_or_null, int greedy, int guided);
/* Test entry: the ban launch, then either the rebuild of the partials or (edits given: the three lists, min_p 0) the edit launch,
 * alone on the caller's rows: logits [batch <= 64][vocab <= 262144] (host or device, as edited_out), history [batch][history_stride]
 * with history_lens [batch] (each <= 8192) and picked [batch] (int64_t, negative: a prompt column) on the host.  edited_out
 * [batch][vocab]: the rows as the stages leave them; part_val_out / part_idx_out [batch][n_part], n_part = min(64, ceil(vocab /
 * 256)): the rebuilt partials, slices as zg_debug_guide_rows documents them.  The argument refusals of a call.  Needs zg_init only. */
int zg_debug_ban_rows(const float* logits, size_t batch, size_t vocab, const zg_ban_rules* bans, const size_t* history,
                      size_t history_stride, const size_t* history_lens, const int64_t* picked, const zg_logit_edits* edits_or_null,
                      float* edited_out, float* part_val_out, int32_t* part_idx_out);
/* ---- Forking rows of the KV caches.  Row b's caches — positions [0, zg_gpt_cached_len) of every layer, K and V,
 * in whatever format the handle stores them — become byte for byte those of row src_rows[b].  Rows with src_rows[b] == b are not
 * touched, and neither is any position at or beyond the cached length.  One launch on the handle's stream: no host round trip,
 * nothing allocated, nothing drained.  Only the caches are copied: logits, the residual stream and recorded tokens stay each row's
 * own, so a forked row is continued with zg_gpt_forward(cached_len + 1, ...) / zg_gpt_extend on tokens the caller chooses — "prefill
 * once, draw n continuations", or a tree search driven from the host.
 * Refusals, before anything is enqueued: n_rows != batch or a NULL array: ZG_ERR_ARG; src_rows[b] >= batch: ZG_ERR_SHAPE; a source
 * that is itself a destination (src_rows[src_rows[b]] != src_rows[b]): ZG_ERR_ARG — with every source a fixed point no workgroup
 * reads what another writes, and the copy needs no second buffer. */
int zg_gpt_kv_fork(zg_gpt* g, const size_t* src_rows, size_t n_rows);
/* Diagnostic (tests): the raw cache bytes of positions first_pos .. first_pos + n_pos - 1 of one row of one layer's K (which 0) or
 * V (which 1) cache: [n_heads][n_pos][64] elements in storage format (fp32, fp16, or the bf16 plane of a 24-bit cache), followed
 * for a 24-bit cache by its byte plane [n_heads][n_pos][64].  Drains the handle's stream.  out is host memory of out_bytes >= that. */
int zg_debug_gpt_kv_rows(zg_gpt* g, size_t layer, int which, size_t row, size_t first_pos, size_t n_pos, void* out, size_t out_bytes);

/* ---- Beam search in the device loop.  The handle's batch B is split into G = B / num_beams groups of W = num_beams
 * slots; group g owns rows g W .. g W + W - 1, whose prompts must be equal (all prompt_lens equal n_p).  Picked columns are p >= c0 =
 * past_len + n_p, under the library's column convention (step p picks column p).  Every slot carries a cumulative fp32 score; at c0
 * only the first slot of a group is live, with score 0.  A step of a group that is not done:
 *   - candidates (score[s] + top_logprobs[s][p][j], s, j) over its live slots and the top 2 W entries j of each slot's row (the
 *     log-probability stage's lists, raw logits at temperature 1): one rounded fp32 add.  Order: value descending, s ascending, j
 *     ascending; NaN never wins.  The first 2 W are kept and walked in order, rank r = 0 ...
 *   - a candidate whose token is eos_id is offered to the group's pool of finished hypotheses if r < W and skipped otherwise (the
 *     rule of HF generate); its normalised score is value / lenpow[p - c0 + 1], lenpow[L] = (float)pow((double)L, (double)
 *     length_penalty), one correctly rounded fp32 division.  Any other candidate becomes the next beam until W are taken.
 *   - the pool holds at most W entries (sum, norm, parent slot, column); a full pool takes an offer only if its norm is strictly
 *     greater than the worst entry's, in its place.  The worst entry is the one of lowest norm and, among equal norms, the one at
 *     the highest index of the pool.
 *   - slots in rank order: a beam keeps its parent's slot unless an earlier beam took it; the beams left over take the free slots
 *     in ascending order.  Every slot's caches then become its parent's (the kernel of zg_gpt_kv_fork, its table read on the device).
 *   - the group is done when its pool is full and (early_stopping != 0, or worst norm >= best new beam's score / lenpow[p - c0 +
 *     1]).  The slots of a done group keep decoding in lock step; nothing of theirs is read afterwards.
 * The recorded lists of column p are indexed by the slot as it stood BEFORE step p — the parent's slot; the recorded token, parent
 * and score of column p by the slot after it.
 * The generation ends early once every group is done, paced as a stop generation is (zg_stop_conditions.lookahead; 0: the
 * library's default): with f the column at which the last group was done, f + 1 <= end <= min(past_len + n_steps, f + 1 +
 * lookahead + 64).  Without eos_id (ZG_BEAM_NO_EOS) nothing ends early and nothing is paced.  Afterwards zg_gpt_cached_len == end.
 * The request carries past_len, prompts, prompt_stride, prompt_lens and n_steps; options, penalties, prior, logprobs, top_n, stop
 * and edits must be NULL / 0 (ZG_ERR_ARG): beams over a penalised, edited, guided or banned distribution need a per-slot history
 * that follows the fork.  Further refusals, all before anything is enqueued or the handle's state is touched —
 * ZG_ERR_ARG: a wrong size field; num_beams outside 1 .. ZG_BEAM_MAX; batch % num_beams != 0; 2 num_beams > vocab_size; a
 * length_penalty that is not finite; unequal prompt lengths, or unequal prompts within a group; n_steps <= n_p (nothing would be
 * picked).  ZG_ERR_SHAPE: eos_id >= vocab_size
 * (and not ZG_BEAM_NO_EOS).  The batch <= 8 rows of a handle are the home of up to 8 beams. */
#define ZG_BEAM_MAX 8
#define ZG_BEAM_NO_EOS ((size_t)-1)
typedef struct {
    size_t size;           /* sizeof(zg_beam_options), else ZG_ERR_ARG */
    size_t num_beams;
    size_t eos_id;         /* ZG_BEAM_NO_EOS: none */
    float length_penalty;
    int early_stopping;
    size_t lookahead;
} zg_beam_options;
int zg_gpt_generate_beam_enqueue(zg_gpt* g, const zg_generate_request* r, const zg_beam_options* beam);
/* The n_return <= num_beams best hypotheses of every group of the last beam generation, best first.  Drains the stream and
 * finalises on the host: a group that is not done offers the beams in its slots as hypotheses of length end - c0 (norm = score /
 * lenpow[end - c0]) to its pool under the pool's rule, in slot order; the pool is sorted by norm descending (equal norms: pool
 * index ascending) and each entry is backtracked through the recorded parents and tokens.  tokens_out [G][n_return][stride]
 * receives the picked tokens only, eos last where there is one; lens_out [G][n_return] their count (0 for a hypothesis the group
 * does not have, with score and sum NaN); scores_out the norms, sum_logprobs_out the cumulative scores.  ZG_ERR_ARG unless the
 * last generation was a beam generation and 1 <= n_return <= num_beams; ZG_ERR_SHAPE when stride is below a length to store. */
int zg_gpt_generate_fetch_beams(zg_gpt* g, size_t n_return, size_t* tokens_out, size_t stride, size_t* lens_out, float* scores_out,
                                float* sum_logprobs_out);
/* The recorded parents (the slot, as a row of the handle, each slot's beam came from) and cumulative scores of columns first ..
 * first + n - 1 of the last beam generation: parents_out, scores_out [batch][n], len >= batch * n.  Columns below c0 or at and
 * beyond end hold what an earlier call left.  The top-2W lists leave through zg_gpt_generate_fetch_logprobs with top_n = 2 num_beams. */
int zg_gpt_generate_fetch_beam_trace(zg_gpt* g, size_t first, size_t n, int* parents_out, float* scores_out, size_t len);
/* The refusal zg_gpt_generate_beam_enqueue would return for these options and this request on a handle of `batch` rows, `vocab`
 * tokens and `context` positions with cached_len cached positions — or ZG_OK.  Needs neither a GPU nor zg_init. */
int zg_debug_beam_check(const zg_generate_request* r, const zg_beam_options* beam, size_t batch, size_t vocab, size_t context, size_t cached_len);
/* Test entry: the beam kernel alone, launched once per column c0 .. c0 + n_cols - 1 over the caller's lists top_ids (int32) and
 * top_logprobs [n_cols][batch][2 num_beams] (host), state carried from column to column; c0 = first_col.  Outputs (host): tokens_out,
 * parents_out (int32) and scores_out [n_cols][batch] by the slot after each step, logprobs_out [n_cols][batch] the chosen entries'
 * bits; pool_out [batch][4] floats (sum, norm, parent, column of entry g W + k; NaN rows beyond pool_n), pool_n_out and
 * done_cols_out [batch / num_beams] (int32; -1: not done), *done_col_out the host word (0: not every group is done).  eos_id,
 * length_penalty and early_stopping from `beam`.  The refusals of the options.  Needs zg_init only. */
int zg_debug_beam_rows(const int32_t* top_ids, const float* top_logprobs, size_t n_cols, size_t batch, size_t vocab, size_t first_col,
                       const zg_beam_options* beam, int32_t* tokens_out, int32_t* parents_out, float* scores_out, float* logprobs_out, float* pool_out,
                       int32_t* pool_n_out, int32_t* done_cols_out, size_t* done_col_out);
/* tokens of positions first .. first + n - 1 of the last generation(s): out_tokens [batch, n] */
int zg_gpt_generate_fetch_range(zg_gpt* g, size_t first, size_t n, size_t* out_tokens, size_t out_len);
/* Test entry: the sampler kernels of zg_gpt_sample_ex on the caller's logits [batch <= 64, vocab <= 262144] (host or device, as
 * uniforms [batch] and the outputs), a small kernel standing in for lm_head's row-maximum partials.  Needs zg_init only.
 * probs_out [batch, vocab] and thresholds_out [batch] (max(tau_k, tau_p) of each row; a zero threshold is +0.0; -inf with both
 * filters off) may be NULL.  Allocates its workspace per call. */
int zg_debug_sample_rows(const float* logits, size_t batch, size_t vocab, const zg_sample_options* options, const float* uniforms,
                         size_t* tokens_out, float* probs_out_or_null, float* thresholds_out_or_null);
/* The same for the prompts of several handles at once (handles on distinct streams: zg_gpt_create_ex): prompts is
 * [sum of the handles' batches, prompt_stride], rows in handle order, prompt_lens alike; every handle generates its own rows.
 * A graph launch returns only when its hardware queue has room, so the handles are fed by one short-lived feeder thread each
 * (inside this call; a single handle is fed by the calling thread) — no queue starves while another one is being filled.
 * zg_gpt_generate_fetch_many drains every handle and returns out_tokens [sum of batches, n_steps] in the same row order.
 * Token for token the result equals one handle per prompt (sequences never interact). */
int zg_gpt_generate_enqueue_many(zg_gpt* const* handles, size_t n_handles, const size_t* prompts, size_t prompt_stride,
                                 const size_t* prompt_lens, size_t n_steps);
int zg_gpt_generate_fetch_many(zg_gpt* const* handles, size_t n_handles, size_t n_steps, size_t* out_tokens, size_t out_len);

/* ------------------------------------------------------------------ measurement helpers ---- */

/* Replay one kernel class of the decode step (layer 0; classes numbered as in
 * zg_gpt_profile_step: 0 embed ... 6 lm_head) `iters` times back to back from a hipGraph at
 * seq_len = context/2 and return the average device time per launch in microseconds (launch
 * boundary included) and the kernel's algorithmic weight bytes.  A warm-cache microbenchmark: the
 * in-situ numbers are zg_gpt_profile_step's.  Options ride in the upper bits of the class argument: ZG_TIME_WALK_LAYERS walks
 * the layers (launch i takes layer i mod n_layer, so that no launch finds its weights in the L2s: the memory-side cost of the
 * real step), ZG_TIME_AT(t) runs the chain at sequence length t (t < 32768: the option field is 15 bits wide). */
#define ZG_TIME_WALK_LAYERS 0x100
#define ZG_TIME_AT(t) ((int)((unsigned)(t) << 16))
int zg_gpt_time_kernel(zg_gpt* g, int which_and_options, int iters, float* avg_us, size_t* algorithmic_bytes);

/* Run `iters` consecutive decode steps starting at sequence length seq_len as EAGER launches with a
 * HIP event between every two kernels, and return the average device time in microseconds that
 * one step spends per kernel class (classes 1-5 summed over the layers):
 *   [0] token select + embedding   [1] ln_1 + c_attn + KV append   [2] decode attention
 *   [3] head merge + attn c_proj + residual   [4] ln_2 + c_fc + gelu   [5] mlp c_proj + residual
 *   [6] ln_f + lm_head + argmax     [7] sum of all intervals
 *   [8] (when n_out >= 9) the interval of a one-element copy kernel recorded the same way: the launch
 *       boundary + event overhead contained in every interval above.
 * Intervals are event-to-event, so each includes the boundary to the next kernel. */
int zg_gpt_profile_step(zg_gpt* g, size_t seq_len, int iters, float* us_out, size_t n_out);

/* Diagnostic: how the side-stream prefetcher of the last zg_gpt_generate_* call ended (waits for both streams).
 * out[0] = 1 when the handle has a prefetcher (2: it found no concurrency with the decode stream once and is no longer
 * launched); then per XCD x = 0..7: out[1 + x] prefetcher workgroups that ran
 * there, out[9 + x] why they left (1 = stop behind the last step, 2 = progress stalled), out[17 + x] launches they
 * fetched for.  n_out >= 25.  No reference counterpart. */
int zg_debug_prefetch_stats(zg_gpt* g, unsigned* out, size_t n_out);

/* ------------------------------------------------------------------------------------------------
 * Tokenizer — src/bpe.zig (host side).  Encoder.init takes the two JSON objects of
 * models/<size>/encoder.json (token string -> id) and byte_encoder.json (unicode char -> byte,
 * download_weights.py:69-90) as parallel arrays of NUL-terminated UTF-8 keys and their values.
 * encode / decode keep bpe.zig:60-118's behaviour, including its deviations from GPT-2 BPE (greedy longest
 * prefix instead of merges, POSIX character classes, runs of spaces become their own word).  A word longer
 * than the reference's 20-byte buffer (bpe.zig:73) returns ZG_ERR_SHAPE; n_out receives the count. */
typedef struct zg_bpe zg_bpe;
int zg_bpe_create(zg_bpe** out, const char* const* tokens, const size_t* token_ids, size_t n_tokens,
                  const char* const* unicode_chars, const unsigned char* bytes, size_t n_bytes);
int zg_bpe_destroy(zg_bpe* e);
int zg_bpe_encode(zg_bpe* e, const char* text, size_t text_len, size_t* out, size_t out_cap, size_t* n_out);
int zg_bpe_decode(zg_bpe* e, const size_t* ids, size_t n_ids, char* out, size_t out_cap, size_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* ZGPT2_H */
