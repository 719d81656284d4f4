// api_kernels_debug.hip — test faces of the kernel tiers (include/zgpt2.h zg_debug_*): the whole-prompt Linear and attention with
// their route forced, the GEMM launch counter and stamps, the two planners, the last noted kernel.  None of them stages anything
// or touches the op tier; the two planner faces need neither zg_init nor a GPU.
#include <stdio.h>
#include <string.h>

#include "zg_runtime.h"

using namespace zg;

extern "C" {

int zg_debug_prefill_linear(const uint16_t* A, const uint16_t* W, const float* bias, void* C, size_t M, size_t N, size_t K, int epilogue,
                            int force_kernel, int slices, float* ws, size_t ws_floats) {
    ZG_TRY(require_init());
    ZG_REQUIRE(A && W && C && is_device_ptr(A) && is_device_ptr(W) && is_device_ptr(C) && (!bias || is_device_ptr(bias)) && (!ws || is_device_ptr(ws)),
               ZG_ERR_ARG, "debug_prefill_linear: device pointers");
    ZG_REQUIRE(M >= 1 && M < (1u << 30) && N >= 64 && N < (1u << 30) && K >= 64 && K < (1u << 30) && epilogue >= 0 && epilogue <= 2 && force_kernel >= 0 &&
                   force_kernel <= 2 && slices >= 0,
               ZG_ERR_ARG, "debug_prefill_linear: arguments");
    const int epi = epilogue == 0 ? PF_F32 : epilogue == 1 ? PF_RESID : PF_GELU_SPLIT;
    const PrefillForce force{force_kernel, slices};
    return launch_prefill_gemm(A, W, bias, C, (int)M, (int)N, (int)K, epi == PF_GELU_SPLIT ? 0 : (int)N, epi, ws, ws_floats, nullptr, ctx().stream, nullptr,
                               kSplit, &force);
}

int zg_debug_attn_prefill(const float* qkv, uint16_t* out, size_t batch, size_t n_tokens, size_t n_embed, size_t n_heads, const float* k_cache,
                          const float* v_cache, size_t ctx_len, float* ws, size_t ws_floats, int key_tiles) {
    ZG_TRY(require_init());
    ZG_REQUIRE(qkv && out && is_device_ptr(qkv) && is_device_ptr(out) && (!k_cache || (v_cache && is_device_ptr(k_cache) && is_device_ptr(v_cache))) &&
                   (!ws || is_device_ptr(ws)),
               ZG_ERR_ARG, "debug_attn_prefill: device pointers");
    ZG_REQUIRE(batch >= 1 && n_tokens >= 1 && n_heads >= 1 && n_embed == 64 * n_heads && batch * n_tokens < (1u << 24) && n_embed < (1u << 16) && (!k_cache || ctx_len >= n_tokens) &&
                   key_tiles >= 0 && key_tiles <= 255,
               ZG_ERR_ARG, "debug_attn_prefill: arguments");
    return launch_attn_prefill(qkv, out, (int)batch, 0, (int)n_tokens, (int)n_embed, (int)n_heads, ws, ws_floats, PrefillKv{k_cache, v_cache, 0, 0, (int)ctx_len},
                               ctx().stream, key_tiles);
}

int zg_debug_attn_prefill_at(const float* qkv, uint16_t* out, size_t batch, size_t past_len, size_t n_tokens, size_t n_embed, size_t n_heads,
                             const void* k_cache, const void* v_cache, int kv_mode, size_t ctx_len, float* ws, size_t ws_floats, int key_tiles) {
    ZG_TRY(require_init());
    ZG_REQUIRE(qkv && out && k_cache && v_cache && is_device_ptr(qkv) && is_device_ptr(out) && is_device_ptr(k_cache) && is_device_ptr(v_cache) &&
                   (!ws || is_device_ptr(ws)),
               ZG_ERR_ARG, "debug_attn_prefill_at: device pointers");
    ZG_REQUIRE(batch >= 1 && n_tokens >= 1 && n_heads >= 1 && n_embed == 64 * n_heads && batch * n_tokens < (1u << 24) && n_embed < (1u << 16) &&
                   ctx_len < (1u << 22) && past_len + n_tokens <= ctx_len && kv_mode >= 0 && kv_mode <= 2 && key_tiles >= 0 && key_tiles <= 255,
               ZG_ERR_ARG, "debug_attn_prefill_at: arguments");
    return launch_attn_prefill(qkv, out, (int)batch, (int)past_len, (int)n_tokens, (int)n_embed, (int)n_heads, ws, ws_floats,
                               PrefillKv{k_cache, v_cache, kv_mode, batch * ctx_len * n_embed * 2, (int)ctx_len}, ctx().stream, key_tiles);
}

int zg_debug_prefill_route(int force_kernel, int slices) {
    ZG_REQUIRE(force_kernel >= 0 && (force_kernel <= 2 || force_kernel >= 16) && slices >= 0, ZG_ERR_ARG, "debug_prefill_route: arguments");
    prefill_force_route(force_kernel, slices);
    return ZG_OK;
}

unsigned long long zg_debug_gemm_launches(void) { return gemm_mfma_launch_count(); }
int zg_debug_gemm_stamps(unsigned long long* out, size_t n_words) { return gemm_debug_stamps(out, n_words); }
int zg_debug_last_kernel(char* out, size_t n) {
    if (!out || n == 0) return ZG_ERR_ARG;
    snprintf(out, n, "%s", last_kernel());
    return ZG_OK;
}

// Plans a described decode-regime Linear (gemv_plan) without a GPU or zg_init.  Only null / non-null of the operands matters to
// the planner, so present ones are any non-null address; nothing is dereferenced.
int zg_debug_gemv_plan(int M, int N, int K, int prologue, int epilogue, int weight_type, unsigned operands, int sk_tiles, int t_hi, int* out,
                       size_t n_out) {
    ZG_REQUIRE(out != nullptr && n_out >= ZG_GEMV_PLAN_INTS, ZG_ERR_ARG, "debug_gemv_plan: %d ints of output", ZG_GEMV_PLAN_INTS);
    static float some[2];
    const bool ragged = (operands & ZG_PLAN_RAGGED_STRIDES) != 0;  // row strides wider than the rows
    GemvArgs a{};
    a.M = M;
    a.N = N;
    a.K = K;
    a.prologue = prologue;
    a.epilogue = epilogue;
    a.head_dim = 64;
    a.t_hi = t_hi;
    a.x_stride = K + (ragged ? 8 : 0);
    a.y_stride = a.resid_stride = N + (ragged ? 8 : 0);
    if (operands & ZG_PLAN_LN_FOLDED) a.ln_c2 = a.ln_c3 = some;
    if (operands & ZG_PLAN_PLANES_IN) a.pl_in = reinterpret_cast<const bf16_t*>(some);
    if (operands & ZG_PLAN_STATS_IN) a.st_in = some;
    if (operands & ZG_PLAN_SPLIT_K) {
        a.sk_ws = some;
        a.sk_cnt = reinterpret_cast<int*>(some);
        a.sk_tiles = sk_tiles;
    }
    const GemvPlan p = gemv_plan(a, weight_type);
    const int v[ZG_GEMV_PLAN_INTS] = {p.route, p.grid, p.kslices, p.block, p.lds, p.mt, p.lpr, p.cpl, p.ks, p.nw, p.line, p.gpl, p.alias, p.pairs,
                                      p.steps, p.rows_per_wave, p.waves_per_wg, p.row_group, p.rows_per_wg, p.pf_tiles, p.supported,
                                      p.can_take_planes, p.can_write_planes, p.pl4_with_planes};
    memcpy(out, v, sizeof(v));
    return ZG_OK;
}

// Plans a described whole-prompt Linear (prefill_gemm_plan) without a GPU or zg_init.  Presence flags stand in for the operands;
// nothing is dereferenced.  The process-wide pin of zg_debug_prefill_route is not read: the force is this call's.
int zg_debug_prefill_plan(int M, int N, int K, int ldc, int epilogue, int nsplit, size_t ws_floats, unsigned operands, size_t sk_ws_bytes,
                          unsigned sk_flags_words, int force_kernel, int force_slices, int* out, size_t n_out) {
    ZG_REQUIRE(out != nullptr && n_out >= ZG_PREFILL_PLAN_INTS, ZG_ERR_ARG, "debug_prefill_plan: %d ints of output", ZG_PREFILL_PLAN_INTS);
    PrefillGemmShape sh{M, N, K, ldc, epilogue, nsplit, ws_floats, (operands & ZG_PFPLAN_WS) != 0, (operands & ZG_PFPLAN_LN) != 0,
                        (operands & ZG_PFPLAN_QKV) ? N / 3 : 0, (operands & ZG_PFPLAN_SK_WS) != 0, (operands & ZG_PFPLAN_SK_FLAGS) != 0, sk_ws_bytes,
                        sk_flags_words, PrefillForce{force_kernel, force_slices}};
    const PrefillGemmPlan p = prefill_gemm_plan(sh);
    static_assert(ZG_PREFILL_PLAN_INTS == 21, "prefill_plan_ints packs 21");
    prefill_plan_ints(p, out);
    return ZG_OK;
}

}  // extern "C"
