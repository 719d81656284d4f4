// gemv.hip — the decode-regime Linear: y[M,N] = x[M,K] * W[N,K]^T (+ bias) for M <= 8.
//
// Replaces the cblas_sgemm call of Linear.forward (reference src/ops.zig:21-46) when the batch
// is tiny (decode: M = number of lock-step sequences).  HBM-bandwidth bound: every weight byte is
// read exactly once, 16 B per lane, K-contiguous rows ([out,in] layout of ops.Linear.weight), so
// one row is read by a group of LPR lanes with fully coalesced 16-B loads and reduced with DPP
// row rotations (M == 1: no barrier, except where a workgroup shares one copy of a wide input).
//
// Fused around the dot products (the reference does these as separate host loops / ops):
//   prologue  PRO_LAYERNORM   LayerNorm.forward of the input row   (src/ops.zig:82-104)
//             PRO_ATTN_MERGE  combine split-KV attention partials  (src/ops.zig:284-305 tail)
//   epilogue  EPI_RESIDUAL    state.o + state.x residual adds      (src/main.zig:136-145)
//             EPI_GELU        ops.gelu                             (src/ops.zig:221-228)
//             EPI_QKV         split_qkv + KV-cache append          (src/ops.zig:146-157)
//             EPI_ARGMAX      greedy sampler partial argmax        (replaces src/main.zig:198-207)
//
// This file: gemv_plan decides, once per launch, which kernel a Linear takes and how it is laid out (a GemvPlan, zg_kernels.h);
// every shape threshold and instantiation ladder of the GEMV units lives here.  launch_gemv carries the plan out: it writes the
// layout into the kernel argument and switches on the route; the units' launchers only map the plan's template choice to an
// instantiation.  The kernels: gemv_valu.hip (any prologue / epilogue, M <= 8, vector ALUs), gemv_ksplit.hip (M == 1: K-split
// and linearised-LayerNorm forms), gemv_mfma16.hip / gemv_pl4.hip (2..8 sequences on the matrix cores: 16-wave and four-wave
// plane-fed forms, wave-per-tile lm_head); shared device helpers in gemv_internal.h.
#include "gemv_internal.h"

namespace zg {

namespace {

struct Rung {  // an instantiation serves up to `max` 16-byte chunks (per row, or per K quarter) with LPR lanes x CPL chunks
    int max, lpr, cpl;
};
constexpr Rung kValuLadder[] = {{32, 16, 2}, {64, 16, 4}, {96, 16, 6}, {128, 16, 8}, {192, 32, 6}, {256, 32, 8}, {384, 64, 6}, {512, 64, 8}, {1024, 64, 16}};
constexpr Rung kKsplitLadder[] = {{32, 16, 2}, {96, 32, 3}, {160, 32, 5}, {224, 32, 7}, {256, 64, 4}};
constexpr Rung kLnkLadder[] = {{32, 16, 2}, {64, 32, 2}, {96, 32, 3}, {128, 64, 2}};
template <int N>
inline Rung rung(const Rung (&ladder)[N], int chunks) {
    for (const Rung& r : ladder)
        if (chunks <= r.max) return r;
    return Rung{0, 64, 0};  // beyond the ladder: no instantiation (cpl == 0)
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ---- VALU kernel: the batch rows (rounded up to 1, 2, 4, 8) stay in LDS
inline int valu_mt(int M) { return M <= 1 ? 1 : (M <= 2 ? 2 : (M <= 4 ? 4 : 8)); }
inline size_t valu_lds(int strips, int mt, int K) { return ((size_t)strips * K + 4 * mt * 2 + 64) * sizeof(float); }

// Rows per wave: enough waves to cover the chip (256 CUs x 4 SIMDs x 2) without dropping below one double pass
// (2 * 64/LPR rows) per wave.  Also the layout of one row group, and of K % 8 != 0 (the slow generic kernel, op tier only).
void plan_valu(const GemvArgs& a, GemvPlan& p) {
    const Rung r = rung(kValuLadder, a.K / 8);
    p.route = GR_VALU, p.lpr = r.lpr, p.cpl = r.cpl;
    p.mt = a.M <= 8 ? valu_mt(a.M) : 0;
    const int rpp2 = 2 * (64 / r.lpr);
    const int target_waves = 256 * 4 * 2;
    p.rows_per_wave = ceil_div(ceil_div(a.N, target_waves), rpp2) * rpp2;
    if (p.rows_per_wave < rpp2) p.rows_per_wave = rpp2;
    const int waves = ceil_div(a.N, p.rows_per_wave);
    // M == 1 without the argmax tail: one-wave workgroups while the matrix has at most ~8 waves per CU
    int wpw = 4;
    if (a.M == 1 && a.epilogue != EPI_ARGMAX) {
        wpw = waves <= 2048 ? 1 : 4;
        if (a.prologue == PRO_NONE && a.K >= 2048 && a.K <= 8192) wpw = 2;  // measured in situ: 2 >= 4 at K = 3072 (124M) and K = 6400 (XL)
        if (a.prologue == PRO_ATTN_MERGE) wpw = 4;
    }
    p.waves_per_wg = wpw;
    p.grid = ceil_div(waves, wpw), p.kslices = 1, p.block = 64 * wpw;
    const int mt = valu_mt(a.M);
    p.lds = (int)valu_lds(mt == 1 ? wpw : mt, mt, a.K);
    p.rows_per_wg = a.M > 1 ? 0 : wpw * p.rows_per_wave;
    p.pf_tiles = a.M > 1 ? 0 : p.grid;
    p.supported = p.mt != 0 && p.cpl != 0 && (size_t)p.lds <= kGemvLdsMax;
    if (a.K % 8 != 0) {  // one wave per row, four rows per workgroup: nothing of the layout above
        p = GemvPlan{};
        p.route = GR_GENERIC, p.grid = ceil_div(a.N, 4), p.kslices = 1, p.block = 256, p.waves_per_wg = 4;
        p.supported = a.prologue == PRO_NONE && a.epilogue == EPI_STORE;
    }
}

// ---- matrix cores (gemv_mfma16.hip, gemv_pl4.hip): the lock-step batch of the model tier
inline size_t mfma_lds(int K, int nw, bool alias, bool line, bool gpl) {
    const size_t planes = gpl ? 0 : (size_t)3 * kMfmaRows * (2 * K + 16);
    return planes + 64 * sizeof(float) + (alias ? 0 : (size_t)2 * nw * 64 * 4 * sizeof(float)) + (line ? (size_t)nw * 2048 : 0);
}

// bf16 weights, 2..8 rows.  Returns false (p untouched) for a launch that stays on the vector ALUs.
bool plan_mfma(const GemvArgs& a, int off, GemvPlan& p) {
    const bool argmax = a.epilogue == EPI_ARGMAX, ln = a.prologue == PRO_LAYERNORM;
    const int ntiles = ceil_div(a.N, 16);
    // Wide, thin, un-normalised Linears (mlp c_proj) are cut into four K slices over as many workgroups when the caller
    // provided the combine workspace.
    const bool sliced = a.sk_ws != nullptr && a.sk_cnt != nullptr && a.prologue == PRO_NONE && !argmax && a.epilogue != EPI_QKV &&
                        a.K >= 2048 && a.K % 128 == 0 && a.K / 4 <= 3072 && ntiles <= a.sk_tiles;
    if (!sliced) {
        // K a multiple of 32 whose three input planes fit in LDS, a fused LayerNorm no wider than 2048
        if (a.K % 32 != 0 || a.K / 32 < 4 || a.K / 32 > 96 || (ln && a.K > 2048)) return false;
        // wide K: only as single-tile workgroups whose partial tiles alias the planes
        const bool wide_ok = !argmax && ntiles <= 768 && mfma_lds(a.K, 16, true, false, false) <= kGemvLdsMax;
        if (mfma_lds(a.K, argmax ? 4 : 16, false, false, false) > kGemvLdsMax && !wide_ok) return false;
    }
    p.supported = true;
    p.can_write_planes = !argmax;
    p.can_take_planes = !argmax && (a.prologue == PRO_NONE || (ln && a.ln_c2 != nullptr && a.ln_c3 != nullptr && a.K <= 2048));
    p.kslices = sliced ? 4 : 1;
    const int Ks = a.K / p.kslices, steps = Ks / 32;
    // the wave-per-tile lm_head: the K values whose tile fits a wave's registers
    const bool wpt = !(off & kOffLmWpt) && argmax && ln && (steps == 12 || steps == 24 || steps == 32);
    // tiles per workgroup: one per workgroup and slice; eight for the four waves of the wave-per-tile kernel (a multiple of
    // four; sweep: profiles/round4_lm_head_tiles_sweep.txt); otherwise at most 768 workgroups, ~4 per CU for the widest matrices
    p.rows_per_wave = sliced ? 1 : (wpt ? 8 : ceil_div(ntiles, 768));
    if (p.rows_per_wave < 1) p.rows_per_wave = 1;
    p.grid = ceil_div(ntiles, p.rows_per_wave);
    p.rows_per_wg = sliced ? 0 : 16 * p.rows_per_wave;
    p.pf_tiles = sliced ? 0 : p.grid;
    // Plane-fed Linears as four-wave workgroups (gemv_pl4_kernel): one tile per workgroup, whole 64-k pairs, at most five
    // pairs per wave and slice (K <= 1280 per slice: every GPT-2 size but XL, which stays on the 16-wave kernel).
    const int pairs = (Ks / 64 + 3) / 4;
    const bool pl4_shape = !(off & kOffPl4) && !argmax && p.rows_per_wave == 1 && a.N <= 0xffff && !(ln && a.x_stride != a.K) &&
                           !(a.epilogue == EPI_RESIDUAL && a.resid_stride != a.N) && !(a.st_in != nullptr && a.K / 16 > 128) &&
                           a.K % (64 * p.kslices) == 0 && pairs >= 1 && pairs <= 5;
    p.pl4_with_planes = p.can_take_planes && pl4_shape;
    p.waves_per_wg = 4;
    p.block = 256;
    const bool planes = a.pl_in != nullptr && p.can_take_planes;  // (planes it cannot take: launch_gemv refuses the launch)
    if (planes && pl4_shape) {
        p.route = sliced ? GR_PL4_KS : GR_PL4;
        p.pairs = pairs;
    } else if (wpt) {
        p.route = GR_LM_WPT;
        p.steps = steps;
        p.lds = (int)((size_t)3 * kMfmaRows * (2 * a.K + 16) + 4 * kMfmaRows * 8 + 4 * 4096);  // planes, four waves' best (value, index), four 4-KiB slots
    } else {
        p.route = sliced ? GR_MFMA16_KS : GR_MFMA16;
        p.nw = argmax ? 4 : 16;  // lm_head: 4 waves
        const int per_wave = ceil_div(steps, p.nw);
        if (argmax) p.ks = per_wave <= 3 ? 3 : (per_wave <= 6 ? 6 : (per_wave <= 13 ? 13 : 24));
        else p.ks = per_wave <= 2 ? 2 : (per_wave <= 4 ? 4 : 6);
        p.gpl = planes;  // input planes in global memory: no LDS planes, nothing to alias
        // single-tile workgroups let the partial tiles alias the planes when both do not fit (see the kernel)
        p.alias = !p.gpl && !sliced && !argmax && p.rows_per_wave == 1 && mfma_lds(a.K, 16, false, false, false) > kGemvLdsMax;
        // full-line weight loads (LINE instantiations): whole pairs of 32-k steps and room for one 2-KiB slot per wave
        p.line = !(off & kOffLineLoads) && !p.alias && Ks % 64 == 0 && mfma_lds(Ks, p.nw, false, true, p.gpl) <= kGemvLdsMax;
        p.lds = (int)mfma_lds(Ks, p.nw, p.alias, p.line, p.gpl);
        p.waves_per_wg = p.nw;
        p.block = 64 * p.nw;
    }
    return true;
}

}  // namespace

GemvPlan gemv_plan(const GemvArgs& a, int weight_type) {
    GemvPlan p{};
    const int off = decode_paths_off();  // read once per plan, and per plan: tests flip it between handles
    if (weight_type == WT_BF16 && a.M >= 2 && a.M <= kMfmaRows && plan_mfma(a, off, p)) return p;
    plan_valu(a, p);
    const bool plain_epi = a.epilogue == EPI_STORE || a.epilogue == EPI_RESIDUAL || a.epilogue == EPI_GELU;
    const int nchq = a.K / 32;  // 16-byte chunks per K quarter
    auto take = [&p](int route, const Rung& r, int passes) { p.route = route, p.lpr = r.lpr, p.cpl = r.cpl, p.rows_per_wg = passes * (64 / r.lpr); };
    if (a.M == 1 && plain_epi && a.K % 32 == 0 &&
        (a.prologue == PRO_ATTN_MERGE
             // head merge folded into the lanes' own chunks: model tier, <= 4 splits known at launch; wider rows (XL, K = 1600:
             // three chunks per lane) measured slower than the shared strip
             ? a.head_dim == 64 && a.t_hi > 0 && ceil_div(a.t_hi, kAttnChunk) <= 4 && a.K <= 1024
             // plain Linear over a wide input (measured against the shared-strip form in situ)
             : a.prologue == PRO_NONE && a.K >= 2048 && nchq <= 256)) {
        take(GR_KSPLIT, rung(kKsplitLadder, nchq), 2);  // two passes of 64 / LPR rows per workgroup (four measured slower: 2.65 -> 3.3 us for mlp c_proj)
        p.merge_generic = (off & kOffMergeByCount) != 0, p.merge_ml_vector = (off & kOffMergeMlScalar) != 0;  // (launch_ksplit: which merge prologue)
    } else if (a.M == 1 && a.prologue == PRO_LAYERNORM && a.ln_c2 != nullptr && a.ln_c3 != nullptr &&
               (a.epilogue == EPI_STORE || a.epilogue == EPI_GELU || a.epilogue == EPI_QKV) && a.K % 32 == 0 && nchq <= 128 && a.N <= 16384) {
        take(GR_LNK, rung(kLnkLadder, nchq), 4);  // four passes (2.93 against 3.2 us per launch with two; +1 % tokens/s in situ)
    } else if (a.M > 1 && valu_lds(valu_mt(a.M), valu_mt(a.M), a.K) > kGemvLdsMax && a.prologue == PRO_NONE && plain_epi) {
        // Rows of a plain (no prologue) Linear are independent: when M rows of K floats exceed the LDS the batch is run as
        // row groups that fit (the weights are streamed once per group).
        int g = valu_mt(a.M);
        while (g > 1 && valu_lds(g, g, a.K) > kGemvLdsMax) g >>= 1;
        GemvArgs b = a;
        b.M = g;
        plan_valu(b, p);
        p.route = GR_VALU_GROUPS, p.row_group = g;
        p.rows_per_wg = p.pf_tiles = 0;
    }
    if (p.route != GR_KSPLIT && p.route != GR_LNK) return p.supported ? p : GemvPlan{};  // nothing else of an unsupported plan has a meaning
    // the two K-split kernels: four waves, every wave streams all rows of the workgroup over its K quarter; no LDS strip
    p.rows_per_wave = p.rows_per_wg, p.waves_per_wg = 4;
    p.grid = ceil_div(a.N, p.rows_per_wg), p.block = 256, p.lds = 0;
    p.supported = true;
    return p;
}

int launch_gemv(const GemvArgs& a, const GemvPlan& p, int weight_type, hipStream_t s) {
    ZG_REQUIRE(a.pl_in == nullptr || p.can_take_planes, ZG_ERR_UNSUPPORTED, "gemv: input planes given to a launch outside the matrix-core path");
    ZG_REQUIRE(a.pl_out == nullptr || p.can_write_planes, ZG_ERR_UNSUPPORTED, "gemv: output planes asked of a launch outside the matrix-core path");
    ZG_REQUIRE(p.supported, ZG_ERR_UNSUPPORTED,
               "gemv: no kernel for M=%d x K=%d, prologue %d, epilogue %d (at most 8 rows per launch that fit the LDS, whole or in groups; K <= 8192; "
               "K not a multiple of 8 only for a plain Linear)", a.M, a.K, a.prologue, a.epilogue);
    GemvArgs b = a;  // the layout fields of the kernel argument come from the plan, here and nowhere else
    b.rows_per_wave = p.rows_per_wave;
    b.waves_per_wg = p.alias ? -1 : p.waves_per_wg;
    b.kslices = p.kslices;
    switch (p.route) {
        case GR_KSPLIT: return gemv_launch_ksplit(b, p, weight_type, s);
        case GR_LNK: return gemv_launch_lnk(b, p, weight_type, s);
        case GR_MFMA16: case GR_MFMA16_KS: return gemv_launch_mfma16(b, p, s);
        case GR_PL4: case GR_PL4_KS: return gemv_launch_pl4(b, p, s);
        case GR_LM_WPT: return gemv_launch_lm_wpt(b, p, s);
        case GR_VALU_GROUPS:
            for (int m0 = 0; m0 < a.M; m0 += p.row_group) {
                b.M = a.M - m0 < p.row_group ? a.M - m0 : p.row_group;
                b.x = a.x + (size_t)m0 * a.x_stride;
                b.y = a.y + (size_t)m0 * a.y_stride;
                if (a.resid) b.resid = a.resid + (size_t)m0 * a.resid_stride;
                GemvPlan q{};
                plan_valu(b, q);  // M == 1 groups are laid out differently
                b.rows_per_wave = q.rows_per_wave, b.waves_per_wg = q.waves_per_wg;
                ZG_TRY(gemv_launch_valu(b, q, weight_type, s));
            }
            return ZG_OK;
        default: return gemv_launch_valu(b, p, weight_type, s);  // GR_VALU, GR_GENERIC
    }
}

}  // namespace zg
