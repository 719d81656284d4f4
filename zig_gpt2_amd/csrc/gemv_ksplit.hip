// gemv_ksplit.hip — M == 1: the K-split kernel (wide plain inputs, the head-merging c_proj) and the linearised-LayerNorm kernel; see gemv.hip
#include <algorithm>

#include "gemv_internal.h"

namespace zg {

namespace {

// ================================================================================================
// M == 1, wide un-normalised input (mlp c_proj: K = 4 E): the four waves of a workgroup SPLIT K.
//
// In the kernel above a wide input row is as many bytes per wave as the wave's weight rows, so it went through a
// shared LDS strip behind a barrier — a memory round trip, an LDS round trip and a barrier in front of the first
// FMA.  Here wave w owns columns [w K/4, (w+1) K/4) of every row of the workgroup: its quarter of the input goes
// straight from global memory into registers (fetched next to the weights, no LDS, no barrier), every wave streams
// the same 2 * RPP rows (quarter-row segments of >= 1.5 KB, fully coalesced), and the four partial sums per row
// meet in LDS after the arithmetic, where one thread per row runs the epilogue.
//
// The input prologue is the compile-time NS (launch_ksplit picks it; a captured graph has one t_hi per bucket, so one NS):
//   NS == 0               plain input row (mlp c_proj): no merge code in the instantiation
//   NS == 1 .. 4          attn c_proj: the input is the head merge of exactly NS attention split partials
//   NS == kNsGeneric      the merge as it was before NS existed: four slots whatever the split count, read from `em` — kept as
//                         the reference of tests/test_merge_splits_gpu.py and the A/B switch (ZGPT2_DECODE_PATHS_OFF kOffMergeByCount)
// NH (NS 1..4 only): how the (m, l) words of a partial reach the lanes.  0: every lane loads those of its own chunks (vector
// loads).  1..4: they are the same for every lane whose chunk lies in the same head, and a wave's K quarter touches at most NH
// heads, so the wave fetches NH x NS pairs with wave-uniform (scalar) loads and every lane selects its head's.
constexpr int kNsGeneric = 5;

// One chunk's 8 merged-input elements from the partials: the loads of split partial `ps` (d0 = the chunk's offset in its head)
__device__ __forceinline__ W8 load_part8(const float* ps, int d0) {
    const float2 a0 = *reinterpret_cast<const float2*>(ps + d0), a1 = *reinterpret_cast<const float2*>(ps + d0 + 2);
    const float2 a2 = *reinterpret_cast<const float2*>(ps + d0 + 4), a3 = *reinterpret_cast<const float2*>(ps + d0 + 6);
    W8 o;
    o.v[0] = a0.x; o.v[1] = a0.y; o.v[2] = a1.x; o.v[3] = a1.y;
    o.v[4] = a2.x; o.v[5] = a2.y; o.v[6] = a3.x; o.v[7] = a3.y;
    return o;
}

template <typename WT, int LPR, int CPL, int NP, int NS, int NH>  // NP passes of 64 / LPR rows per workgroup
__global__ __launch_bounds__(256) void gemv_ksplit_kernel(const void* __restrict__ Wv, const float* __restrict__ xin, int N,
                                                          int K, unsigned em, const float* __restrict__ part_in, int max_splits,
                                                          const float* __restrict__ bias, const float* __restrict__ resid,
                                                          const GemvArgs a) {
    // 14 preloaded dwords: Wv, xin, N, K, em = epilogue | merge_splits << 8 | has_bias << 16 | has_resid << 17, the attention
    // partials and their split stride, bias and residual (a few zero floats when absent: read at index 0)
    const int epilogue = (int)(em & 0xffu), merge_splits = (int)((em >> 8) & 0xffu);
    const int has_bias = (int)((em >> 16) & 1u), has_resid = (int)((em >> 17) & 1u);
    ZG_STAMP_DECL();
    ZG_STAMP(0);
    // NS > 0 (attn c_proj): the input is the head merge of the attention partials — every lane combines
    // the <= 4 split partials of ITS OWN 8-element chunks (a chunk lies inside one head), all loads issued with the
    // weights; no shared strip, no barrier in front of the FMAs (the merge through an LDS strip cost 3.9 us per
    // launch against 2.55 us for the plain K-split kernel).
    static_assert(NS >= 0 && NS <= kNsGeneric && NH >= 0 && NH <= 4 && (NH == 0 || (NS >= 1 && NS <= 4)), "see the table above");
    constexpr int RPP = 64 / LPR, ROWS = NP * RPP;
    __shared__ float part[4][ROWS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane % LPR, rsub = lane / LPR;
    const int Kq = K >> 2, nchq = Kq >> 3;
    const auto W = wmat<WT>(Wv, (size_t)wave * Kq);
    const int row0 = blockIdx.x * ROWS;
    // all loads of the kernel up front: NP passes of weights, the input quarter, the epilogue operands
    Raw<WT> wq[NP][CPL];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const auto pr = wrow(W, (size_t)min(row0 + p * RPP + rsub, N - 1), K);
#pragma unroll
        for (int i = 0; i < CPL; ++i) wq[p][i] = load_raw(pr, min(lr + LPR * i, nchq - 1));
    }
    W8 xr[CPL];
    if constexpr (NS >= 1 && NS < kNsGeneric) {
        // Exactly NS partials per chunk, every load unconditional.  The arithmetic is the generic prologue's (next branch), term
        // by term — the maximum over the present m, weights __expf(m_s - mx), FMAs in split order, one reciprocal — without its
        // surplus slots.  Those re-read a present partial with m = -1e30: weight __expf(-1e30 - mx) == 0 for every mx > -1e30
        // (any finite attention score), so each added fmaf(0, finite, r) == r to l and to every element (r starts at +0, and an
        // FMA onto +0 never yields -0).  The condition is a finite partial; a non-finite one poisons the result through its own
        // term in both forms.
        float2 mlh[NH > 0 ? NH : 1][NS];
        const int h0w = (wave * Kq) >> 6;  // first head of this wave's K quarter: wave-uniform (`wave` went through readfirstlane)
        if constexpr (NH > 0) {
            const int hlast = (K >> 6) - 1;
#pragma unroll
            for (int j = 0; j < NH; ++j) {
                const int hj = min(h0w + j, hlast);  // (a quarter that touches fewer heads re-reads its last)
#pragma unroll
                for (int sp = 0; sp < NS; ++sp)
                    mlh[j][sp] = *reinterpret_cast<const float2*>(part_in + ((size_t)hj * max_splits + sp) * kPartStride + 64);
            }
        }
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int e0 = wave * Kq + min(lr + LPR * i, nchq - 1) * 8;
            const int h = e0 >> 6, d0 = e0 & 63;  // head_dim 64
            const float* p = part_in + ((size_t)h * max_splits) * kPartStride;
            float ms[NS], ls[NS];
            W8 o[NS];
#pragma unroll
            for (int sp = 0; sp < NS; ++sp) {
                const float* ps = p + sp * kPartStride;
                o[sp] = load_part8(ps, d0);
                if constexpr (NH == 0) {
                    ms[sp] = ps[64];
                    ls[sp] = ps[65];
                } else {
                    float2 ml = mlh[0][sp];
#pragma unroll
                    for (int j = 1; j < NH; ++j)
                        if (h - h0w >= j) ml = mlh[j][sp];
                    ms[sp] = ml.x;
                    ls[sp] = ml.y;
                }
            }
            float mx = ms[0];
            if constexpr (NS == 2) mx = fmaxf(ms[0], ms[1]);
            if constexpr (NS == 3) mx = fmaxf(fmaxf(ms[0], ms[1]), ms[2]);
            if constexpr (NS == 4) mx = fmaxf(fmaxf(ms[0], ms[1]), fmaxf(ms[2], ms[3]));
            float l = 0.0f;
            W8 r = zero_w8();
#pragma unroll
            for (int sp = 0; sp < NS; ++sp) {
                const float w = __expf(ms[sp] - mx);
                l = fmaf(w, ls[sp], l);
#pragma unroll
                for (int j = 0; j < 8; ++j) r.v[j] = fmaf(w, o[sp].v[j], r.v[j]);
            }
            const float inv = 1.0f / l;
#pragma unroll
            for (int j = 0; j < 8; ++j) xr[i].v[j] = r.v[j] * inv;
        }
    } else if constexpr (NS == kNsGeneric) {
        constexpr int MAXS = 4;
        const int nsplit = merge_splits;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int e0 = wave * Kq + min(lr + LPR * i, nchq - 1) * 8;
            const int h = e0 >> 6, d0 = e0 & 63;  // head_dim 64
            const float* p = part_in + ((size_t)h * max_splits) * kPartStride;
            float ms[MAXS], ls[MAXS];
            W8 o[MAXS];
#pragma unroll
            for (int sp = 0; sp < MAXS; ++sp) {  // branch-free: surplus splits re-read the last valid one, weight 0 below
                const float* ps = p + min(sp, nsplit - 1) * kPartStride;
                ms[sp] = ps[64];
                ls[sp] = ps[65];
                o[sp] = load_part8(ps, d0);
            }
#pragma unroll
            for (int sp = 0; sp < MAXS; ++sp)
                if (sp >= nsplit) ms[sp] = -1e30f;
            const float mx = fmaxf(fmaxf(ms[0], ms[1]), fmaxf(ms[2], ms[3]));
            float l = 0.0f;
            W8 r = zero_w8();
#pragma unroll
            for (int sp = 0; sp < MAXS; ++sp) {
                const float w = __expf(ms[sp] - mx);
                l = fmaf(w, ls[sp], l);
#pragma unroll
                for (int j = 0; j < 8; ++j) r.v[j] = fmaf(w, o[sp].v[j], r.v[j]);
            }
            const float inv = 1.0f / l;
#pragma unroll
            for (int j = 0; j < 8; ++j) xr[i].v[j] = r.v[j] * inv;
        }
    } else {
#pragma unroll
        for (int i = 0; i < CPL; ++i) xr[i] = load_x8(xin + (size_t)wave * Kq + (size_t)min(lr + LPR * i, nchq - 1) * 8);
    }
    float bias_n = 0.0f, resid_n = 0.0f;
    // (absent operands are a few zero words read at index 0: the loads are unconditional — a load inside a uniform branch
    // whose result is merged with a constant makes the compiler wait at the join for every load issued before it)
    if (tid < ROWS) {
        const int n = min(row0 + tid, N - 1);
        bias_n = bias[n * has_bias];
        resid_n = resid[n * has_resid];
    }
    ZG_STAMP(1);
    ZG_PIN(a.y);  // the tail's argument-block fields, fetched under the vector loads (zg_common.h ZG_PIN)
    ZG_PIN(a.progress);
    pf_count(a.progress);
    ZG_STAMP(2);
#pragma unroll
    for (int i = 0; i < CPL; ++i)
        if (lr + LPR * i >= nchq) xr[i] = zero_w8();  // clamped surplus chunks multiply zeros
    auto dot = [&](const Raw<WT>(&w)[CPL]) {
        float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const W8 u = unpack(w[i]);
            p0 = fmaf(u.v[0], xr[i].v[0], p0); p1 = fmaf(u.v[1], xr[i].v[1], p1);
            p2 = fmaf(u.v[2], xr[i].v[2], p2); p3 = fmaf(u.v[3], xr[i].v[3], p3);
            p0 = fmaf(u.v[4], xr[i].v[4], p0); p1 = fmaf(u.v[5], xr[i].v[5], p1);
            p2 = fmaf(u.v[6], xr[i].v[6], p2); p3 = fmaf(u.v[7], xr[i].v[7], p3);
        }
        return group_allsum<LPR>((p0 + p1) + (p2 + p3));
    };
    float sp[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) sp[p] = dot(wq[p]);
    ZG_STAMP(3);
    if (lr == 0) {
#pragma unroll
        for (int p = 0; p < NP; ++p) part[wave][p * RPP + rsub] = sp[p];
    }
    __syncthreads();
    ZG_STAMP(4);
    if (tid < ROWS && row0 + tid < N) {
        const int n = row0 + tid;
        const float v = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) + bias_n;
        a.y[n] = epilogue == EPI_RESIDUAL ? v + resid_n : (epilogue == EPI_GELU ? gelu_ref(v) : v);
    }
    ZG_STAMP(5);
    ZG_STAMP(6);
    ZG_STAMP(7);
    ZG_STAMP_FLUSH();
}

template <typename WT>
int launch_ksplit(const GemvArgs& a, const GemvPlan& pl, hipStream_t s) {
    const int merge_splits = a.prologue == PRO_ATTN_MERGE ? (a.t_hi + kAttnChunk - 1) / kAttnChunk : 0;
    const unsigned has_resid = a.epilogue == EPI_RESIDUAL ? 1u : 0u;
    const unsigned em = (unsigned)a.epilogue | ((unsigned)merge_splits << 8) | ((a.bias ? 1u : 0u) << 16) | (has_resid << 17);
    // The merge prologue's instantiation: NS = the split count (gemv_plan admits the merge for 1..4 splits only), or the generic
    // four-slot form where the plan keeps it.  NH = the most heads a wave's K quarter touches, where the scalar fetch of (m, l)
    // pays: at most Kq / 64 + 1 of them (whole heads, E = 768 / 1024; inside one head, E = 128; E = 384 straddles into 2) and
    // at most the 4 the kernel is instantiated for — otherwise 0, the lanes' own vector loads.
    int ns = merge_splits, nh = 0;
    if (merge_splits > 0 && (pl.merge_generic || merge_splits > 4)) ns = kNsGeneric;
    if (ns >= 1 && ns <= 4 && !pl.merge_ml_vector) {
        const int Kq = a.K >> 2;
        for (int w = 0; w < 4; ++w) nh = std::max(nh, (((w + 1) * Kq - 1) >> 6) - ((w * Kq) >> 6) + 1);
        if (nh > Kq / 64 + 1 || nh > 4) nh = 0;
    }
    // two passes of 64 / LPR rows per workgroup
#define ZG_KS(LPR_, CPL_, NS_, NH_)                                                                                      \
    if (pl.lpr == LPR_ && pl.cpl == CPL_ && ns == NS_ && nh == NH_) {                                                    \
        note_kernel("gemv_ksplit_kernel<%s, %d, %d, 2, %d, %d>", wt_name<WT>(), LPR_, CPL_, NS_, NH_);                   \
        hipLaunchKernelGGL((gemv_ksplit_kernel<WT, LPR_, CPL_, 2, NS_, NH_>), dim3(pl.grid), dim3(256), 0, s, a.W, a.x,  \
                           a.N, a.K, em, a.part ? a.part : a.zero, a.max_splits, a.bias ? a.bias : a.zero,              \
                           has_resid ? a.resid : a.zero, a);                                                             \
        ZG_HIP(hipGetLastError());                                                                                       \
        return ZG_OK;                                                                                                    \
    }
#define ZG_KS_MERGE(NS_) ZG_KS(16, 2, NS_, 0) ZG_KS(16, 2, NS_, 1) ZG_KS(16, 2, NS_, 2) ZG_KS(16, 2, NS_, 3) ZG_KS(16, 2, NS_, 4)
    // the merge (K <= 1024: at most 32 chunks per quarter) lives on the first rung, the wide plain inputs (K >= 2048) on the others
    ZG_KS_MERGE(1)
    ZG_KS_MERGE(2)
    ZG_KS_MERGE(3)
    ZG_KS_MERGE(4)
    ZG_KS(16, 2, kNsGeneric, 0)
    ZG_KS(32, 3, 0, 0)
    ZG_KS(32, 5, 0, 0)
    ZG_KS(32, 7, 0, 0)
    ZG_KS(64, 4, 0, 0)
#undef ZG_KS_MERGE
#undef ZG_KS
    zg::set_error("gemv (K split): no instantiation for K=%d, %d merge splits", a.K, merge_splits);
    return ZG_ERR_UNSUPPORTED;
}


// ================================================================================================
// M == 1, LayerNorm in front (ln_1 + c_attn, ln_2 + c_fc): the LayerNorm is LINEARISED out of the dot product.
//
//   y_n = sum_k W_nk ((x_k - mu) r g_k + b_k) + bias_n  =  r (S1_n - mu c2_n) + c3_n
//   S1_n = sum_k W_nk (g_k x_k),   c2_n = sum_k W_nk g_k,   c3_n = sum_k W_nk b_k + bias_n
//
// c2 / c3 depend on the weights only (launch_ln_fold, once after loading); S1 needs no statistics, so the kernel
// has the shape of the K-split kernel above — every load issued at entry, wave w owns K quarter w, FMAs straight
// from registers — and mu, r (single pass sum / sum of squares, std = sqrt(E[x^2] - mean^2 + eps): ops.zig:88-101)
// are needed only by the one thread per row that combines the four partial sums.  The kernel it replaces spent a
// third of its time in the dependent chain load x -> two wave reductions -> normalise -> LDS -> registers before
// its first FMA.  (Same real-number result; in floating point r (S1 - mu c2) cancels when |mu| >> sigma, which costs
// log2(|mu| / sigma) bits of the fp32 product sums — far inside the 1e-3 bound for any LayerNorm input.)
template <typename WT, int LPR, int CPL, int NP = 2>  // NP passes of 64 / LPR rows per workgroup
__global__ __launch_bounds__(256) void gemv_lnk_kernel(const void* __restrict__ Wv, const float* __restrict__ xin, unsigned ne, int K,
                                                       const float* __restrict__ ln_g, const float* __restrict__ c2,
                                                       const float* __restrict__ c3, const int* __restrict__ cw,
                                                       const GemvArgs a) {
    // 14 preloaded dwords: Wv, xin, ne = N | epilogue << 24, K, ln_g, c2, c3, cw = the step control block (always a
    // readable address: its second word is the sequence length of the KV append).  The body (gemv_internal.h) is shared with
    // the fused ln_1 + c_attn + attention kernel (attn_qkv.hip).
    gemv_lnk_body<WT, LPR, CPL, NP, false>((int)blockIdx.x, Wv, xin, ne, K, ln_g, c2, c3, cw, a, 1u, nullptr, nullptr, 0u);
}

// c2[n] = sum_k W[n][k] g[k], c3[n] = sum_k W[n][k] b[k] + bias[n]: one wave per row, fp32 accumulation.
template <typename WT>
__global__ __launch_bounds__(256) void ln_fold_kernel(const void* __restrict__ Wv, const float* __restrict__ g,
                                                      const float* __restrict__ b, const float* __restrict__ bias, int N, int K,
                                                      float* __restrict__ c2, float* __restrict__ c3) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const WT* w = reinterpret_cast<const WT*>(Wv) + (size_t)row * K;
    float s2 = 0.0f, s3 = 0.0f;
    for (int k = lane; k < K; k += 64) {
        float wv;
        if constexpr (sizeof(WT) == 2) wv = __uint_as_float((uint32_t)w[k] << 16);
        else if constexpr (sizeof(WT) == 3) wv = b24_elem(Wv, (size_t)row, K, (size_t)k);  // c2 / c3 of the stored values
        else wv = w[k];
        s2 = fmaf(wv, g[k], s2);
        s3 = fmaf(wv, b[k], s3);
    }
    s2 = wave_allsum(s2);
    s3 = wave_allsum(s3);
    if (lane == 0) {
        c2[row] = s2;
        c3[row] = s3 + (bias ? bias[row] : 0.0f);
    }
}

template <typename WT>
int launch_lnk(const GemvArgs& a, const GemvPlan& pl, hipStream_t s) {
    // four passes of 64 / LPR rows per workgroup
#define ZG_LK(LPR_, CPL_)                                                                                              \
    if (pl.lpr == LPR_ && pl.cpl == CPL_) {                                                                            \
        note_kernel("gemv_lnk_kernel<%s, %d, %d, 4>", wt_name<WT>(), LPR_, CPL_);       \
        hipLaunchKernelGGL((gemv_lnk_kernel<WT, LPR_, CPL_, 4>), dim3(pl.grid), dim3(256), 0, s, a.W, a.x,             \
                           (unsigned)a.N | ((unsigned)a.epilogue << 24), a.K, a.ln_g, a.ln_c2, a.ln_c3,                 \
                           a.ctrl ? reinterpret_cast<const int*>(a.ctrl) : reinterpret_cast<const int*>(a.zero), a);   \
        ZG_HIP(hipGetLastError());                                                                                     \
        return ZG_OK;                                                                                                  \
    }
    ZG_LK(16, 2)
    ZG_LK(32, 2)
    ZG_LK(32, 3)
    ZG_LK(64, 2)
#undef ZG_LK
    zg::set_error("gemv (LayerNorm, K split): no instantiation for K=%d", a.K);
    return ZG_ERR_UNSUPPORTED;
}


// Slow generic fallback for K % 8 != 0 (op tier only): one wave per row, scalar loads.

}  // namespace

int gemv_launch_ksplit(const GemvArgs& a, const GemvPlan& p, int weight_type, hipStream_t s) {
    if (weight_type == WT_B24) return launch_ksplit<b24_t>(a, p, s);
    return weight_type == WT_BF16 ? launch_ksplit<bf16_t>(a, p, s) : launch_ksplit<float>(a, p, s);
}
int gemv_launch_lnk(const GemvArgs& a, const GemvPlan& p, int weight_type, hipStream_t s) {
    if (weight_type == WT_B24) return launch_lnk<b24_t>(a, p, s);
    return weight_type == WT_BF16 ? launch_lnk<bf16_t>(a, p, s) : launch_lnk<float>(a, p, s);
}

int launch_ln_fold(const void* W, int weight_type, const float* g, const float* b, const float* bias, int N, int K, float* c2,
                   float* c3, hipStream_t s) {
    if (weight_type == WT_BF16)
        hipLaunchKernelGGL((ln_fold_kernel<bf16_t>), dim3((N + 3) / 4), dim3(256), 0, s, W, g, b, bias, N, K, c2, c3);
    else if (weight_type == WT_B24)
        hipLaunchKernelGGL((ln_fold_kernel<b24_t>), dim3((N + 3) / 4), dim3(256), 0, s, W, g, b, bias, N, K, c2, c3);
    else
        hipLaunchKernelGGL((ln_fold_kernel<float>), dim3((N + 3) / 4), dim3(256), 0, s, W, g, b, bias, N, K, c2, c3);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

}  // namespace zg
