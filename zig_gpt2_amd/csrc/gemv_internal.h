// gemv_internal.h — what the GEMV translation units share (gemv.hip: the plan and its dispatch; gemv_valu.hip: the general VALU
// kernel; gemv_ksplit.hip: the two M = 1 K-split kernels; gemv_mfma16.hip: the 16-wave matrix-core kernel; gemv_pl4.hip: the
// four-wave plane-fed kernel and the wave-per-tile lm_head): device helpers and, at the end, the units' launchers.  No shape
// test lives here — a launch's route and layout are gemv_plan's (gemv.hip).  Device helpers live in an anonymous namespace:
// every unit gets its own copy.
#pragma once
#include <stdlib.h>

#include "zg_kernels.h"

// Diagnostic build (-DZG_STAMPS): wave 0 of the first and of the last workgroup record s_memtime at
// fixed points of the kernel and append them to GemvArgs::dbg.  Compiled out of the product build.
#ifdef ZG_STAMPS
#define ZG_STAMP_DECL() unsigned long long zg_ts[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define ZG_STAMP(i) zg_ts[i] = __builtin_amdgcn_s_memtime()
#define ZG_STAMP_FLUSH()                                                                              \
    if (a.dbg && threadIdx.x == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x - 1)) {             \
        const unsigned long long slot = atomicAdd(a.dbg, 1ull);                                       \
        unsigned long long* d = a.dbg + 16 + slot * 10;                                               \
        for (int i = 0; i < 8; ++i) d[i] = zg_ts[i];                                                  \
        d[8] = blockIdx.x;                                                                            \
        d[9] = __builtin_amdgcn_s_memtime();                                                          \
    }
#else
#define ZG_STAMP_DECL()
#define ZG_STAMP(i)
#define ZG_STAMP_FLUSH()
#endif

namespace zg {

namespace {


struct W8 {
    float v[8];
};

// Raw (still packed) 8-element weight chunk: kept packed in registers until the FMAs so that two
// passes of loads in flight cost 4 VGPRs per bf16 chunk, not 8.
template <typename WT>
struct Raw;
template <>
struct Raw<bf16_t> {
    u32x4 p;
};
template <>
struct Raw<float> {
    f32x4 a, b;
};

__device__ __forceinline__ Raw<bf16_t> load_raw(const bf16_t* row, int c) {
    Raw<bf16_t> r;
    r.p = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(row) + c);
    return r;
}
__device__ __forceinline__ Raw<float> load_raw(const float* row, int c) {
    Raw<float> r;
    r.a = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(row) + 2 * c);
    r.b = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(row) + 2 * c + 1);
    return r;
}
__device__ __forceinline__ void zero_raw(Raw<bf16_t>& r) { r.p = u32x4{0u, 0u, 0u, 0u}; }
__device__ __forceinline__ void zero_raw(Raw<float>& r) {
    r.a = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    r.b = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}
__device__ __forceinline__ W8 unpack(const Raw<bf16_t>& r) {
    W8 w;
    w.v[0] = bf16_lo(r.p.x); w.v[1] = bf16_hi(r.p.x);
    w.v[2] = bf16_lo(r.p.y); w.v[3] = bf16_hi(r.p.y);
    w.v[4] = bf16_lo(r.p.z); w.v[5] = bf16_hi(r.p.z);
    w.v[6] = bf16_lo(r.p.w); w.v[7] = bf16_hi(r.p.w);
    return w;
}
__device__ __forceinline__ W8 unpack(const Raw<float>& r) {
    W8 w;
    w.v[0] = r.a.x; w.v[1] = r.a.y; w.v[2] = r.a.z; w.v[3] = r.a.w;
    w.v[4] = r.b.x; w.v[5] = r.b.y; w.v[6] = r.b.z; w.v[7] = r.b.w;
    return w;
}

// B24 (zg_common.h b24_t): a chunk is 16 B of upper halves and the 8 low bytes of the same 8 elements
template <>
struct Raw<b24_t> {
    u32x4 h;
    u32x2 l;
};

// Weight matrices as the kernels address them: wmat = the matrix from column k0 on, wrow = one of its rows, the argument of
// load_raw.  bf16 / fp32: plain pointers, W + k0 and W + row K.  B24: a row is 3 K bytes of two parts, so both are kept.
template <typename WT>
struct WMat {
    typedef const WT* type;
};
struct B24Mat {
    const char* base;
    size_t k0;
};
struct B24Row {
    const u32x4* hi;
    const u32x2* lo;
};
template <>
struct WMat<b24_t> {
    typedef B24Mat type;
};
template <typename WT, typename I>
__device__ __forceinline__ typename WMat<WT>::type wmat(const void* W, I k0) {
    if constexpr (sizeof(WT) == 3) return B24Mat{reinterpret_cast<const char*>(W), (size_t)k0};
    else return reinterpret_cast<const WT*>(W) + k0;
}
template <typename WT>
__device__ __forceinline__ const WT* wrow(const WT* W, size_t row, int K) {
    return W + row * K;
}
__device__ __forceinline__ B24Row wrow(const B24Mat& m, size_t row, int K) {
    const char* r = m.base + row * (size_t)(3 * K);
    return B24Row{reinterpret_cast<const u32x4*>(r + 2 * (size_t)m.k0), reinterpret_cast<const u32x2*>(r + 2 * (size_t)K + m.k0)};
}

__device__ __forceinline__ Raw<b24_t> load_raw(const B24Row& row, int c) {
    Raw<b24_t> r;
    r.h = __builtin_nontemporal_load(row.hi + c);
    r.l = __builtin_nontemporal_load(row.lo + c);
    return r;
}
__device__ __forceinline__ void zero_raw(Raw<b24_t>& r) {
    r.h = u32x4{0u, 0u, 0u, 0u};
    r.l = u32x2{0u, 0u};
}
// element j = (upper half j) << 16 | (low byte j) << 8: from here on the fp32 kernels' arithmetic
__device__ __forceinline__ W8 unpack(const Raw<b24_t>& r) {
    W8 w;
    w.v[0] = __uint_as_float((r.h.x << 16) | ((r.l.x & 0xffu) << 8));
    w.v[1] = __uint_as_float((r.h.x & 0xffff0000u) | (r.l.x & 0xff00u));
    w.v[2] = __uint_as_float((r.h.y << 16) | ((r.l.x >> 8) & 0xff00u));
    w.v[3] = __uint_as_float((r.h.y & 0xffff0000u) | ((r.l.x >> 16) & 0xff00u));
    w.v[4] = __uint_as_float((r.h.z << 16) | ((r.l.y & 0xffu) << 8));
    w.v[5] = __uint_as_float((r.h.z & 0xffff0000u) | (r.l.y & 0xff00u));
    w.v[6] = __uint_as_float((r.h.w << 16) | ((r.l.y >> 8) & 0xff00u));
    w.v[7] = __uint_as_float((r.h.w & 0xffff0000u) | ((r.l.y >> 16) & 0xff00u));
    return w;
}

// Kernel-name spelling of the weight type (zg_debug_last_kernel)
template <typename WT>
inline const char* wt_name() {
    return sizeof(WT) == 2 ? "unsigned short" : sizeof(WT) == 3 ? "b24" : "float";
}

__device__ __forceinline__ W8 zero_w8() {
    W8 w;
#pragma unroll
    for (int j = 0; j < 8; ++j) w.v[j] = 0.0f;
    return w;
}

__device__ __forceinline__ W8 load_x8(const float* p) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p);
    const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
    W8 w;
    w.v[0] = a.x; w.v[1] = a.y; w.v[2] = a.z; w.v[3] = a.w;
    w.v[4] = b.x; w.v[5] = b.y; w.v[6] = b.z; w.v[7] = b.w;
    return w;
}

__device__ __forceinline__ float dot8(const W8& w, const W8& x, float acc) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = fmaf(w.v[j], x.v[j], acc);
    return acc;
}

// The order of the argmax partials, in the form the lm_head epilogues were compiled with (zg_common.h pick_before is its one
// definition for every reader of the partials; expressed through it, these kernels' register allocation changes)
struct Best {
    float val;
    int idx;
};
__device__ __forceinline__ Best better(Best a, Best b) {
    return (b.val > a.val || (b.val == a.val && b.idx < a.idx)) ? b : a;
}
__device__ __forceinline__ Best wave_best(Best b) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Best o;
        o.val = __shfl_xor(b.val, off, 64);
        o.idx = __shfl_xor(b.idx, off, 64);
        b = better(b, o);
    }
    return b;
}

template <typename KV>
__device__ __forceinline__ void kv_store(void* cache, size_t off, float v) {
    // fp16 cache: saturate instead of overflowing to inf (a masked position holding inf would turn p = 0 into NaN)
    if (sizeof(KV) == 2) v = fminf(fmaxf(v, -65504.0f), 65504.0f);
    reinterpret_cast<KV*>(cache)[off] = (KV)v;
}

// bias_n / resid_mn were fetched together with the row's weights (no dependent round trip here).
__device__ __forceinline__ float epilogue_row(const GemvArgs& a, int m, int n, float acc, float bias_n,
                                              float resid_mn, int pos, Best& best) {
    float v = acc + bias_n;
    switch (a.epilogue) {
        case EPI_STORE:
            a.y[(size_t)m * a.y_stride + n] = v;
            break;
        case EPI_RESIDUAL:
            v += resid_mn;
            a.y[(size_t)m * a.y_stride + n] = v;
            break;
        case EPI_GELU:
            v = gelu_ref(v);
            if (a.y) a.y[(size_t)m * a.y_stride + n] = v;  // null: the output leaves as planes only (GemvArgs.pl_out)
            break;
        case EPI_QKV: {
            const int E = a.N / 3;
            if (n < E) {
                a.q[(size_t)m * E + n] = v;
            } else {
                const int which = n >= 2 * E;
                const int e = n - (which ? 2 * E : E);
                int h, d;
                if (a.head_dim == 64) {  // the GPT-2 family: no integer division in the epilogue
                    h = e >> 6;
                    d = e & 63;
                } else {
                    h = e / a.head_dim;
                    d = e % a.head_dim;
                }
                const size_t off = (((size_t)m * a.n_heads + h) * a.ctx + pos) * a.head_dim + d;
                void* cache = which ? a.v_cache : a.k_cache;
                if (a.kv_mode == 1) kv_store<_Float16>(cache, off, v);
                else if (a.kv_mode == 2) b24_store(cache, a.kv_lo, off, v);
                else kv_store<float>(cache, off, v);
            }
            break;
        }
        case EPI_ARGMAX: {
            if (a.logits) a.logits[(size_t)m * a.logits_stride + n] = v;
            Best c;
            c.val = v;
            c.idx = n;
            best = better(best, c);
            break;
        }
    }
    return v;
}

// Merged attention output for elements [e0, e0+4) of sequence m: all loads issued before any math.
__device__ __forceinline__ f32x4 merge_attn4(const GemvArgs& a, int m, int e0, int nsplit) {
    const int h = e0 / a.head_dim, d0 = e0 % a.head_dim;
    const float* p = a.part + ((size_t)(m * a.n_heads + h) * a.max_splits) * kPartStride;
    constexpr int MAXS = 4;  // ctx 1024 / 256; more splits fall back to the loop below
    if (nsplit <= MAXS) {
        float ms[MAXS], ls[MAXS];
        float o[MAXS][4];
#pragma unroll
        for (int s = 0; s < MAXS; ++s) {  // branch-free: surplus splits re-read the last valid one ...
            const float* ps = p + min(s, nsplit - 1) * kPartStride;
            ms[s] = ps[64];
            ls[s] = ps[65];
            const float2 lo = *reinterpret_cast<const float2*>(ps + d0);      // 8-B aligned: kPartStride
            const float2 hi = *reinterpret_cast<const float2*>(ps + d0 + 2);  // and d0 are even
            o[s][0] = lo.x; o[s][1] = lo.y; o[s][2] = hi.x; o[s][3] = hi.y;
        }
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s >= nsplit) ms[s] = -1e30f;  // ... and get weight exp(-1e30 - max) == 0
        const float mx = fmaxf(fmaxf(ms[0], ms[1]), fmaxf(ms[2], ms[3]));
        float l = 0.0f;
        float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < MAXS; ++s) {
            const float w = __expf(ms[s] - mx);
            l = fmaf(w, ls[s], l);
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = fmaf(w, o[s][j], r[j]);
        }
        const float inv = 1.0f / l;
        return f32x4{r[0] * inv, r[1] * inv, r[2] * inv, r[3] * inv};
    }
    float mx = -1e30f;
    for (int s = 0; s < nsplit; ++s) mx = fmaxf(mx, p[s * kPartStride + 64]);
    float l = 0.0f;
    float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = 0; s < nsplit; ++s) {
        const float w = __expf(p[s * kPartStride + 64] - mx);
        l = fmaf(w, p[s * kPartStride + 65], l);
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = fmaf(w, p[s * kPartStride + d0 + j], r[j]);
    }
    const float inv = 1.0f / l;
    return f32x4{r[0] * inv, r[1] * inv, r[2] * inv, r[3] * inv};
}

// Branch-free: out-of-range rows / chunks are clamped to a valid address instead of predicated, so the
// loads stay in straight-line code and the compiler can wait for them with counted vmcnt (predicated
// loads sit in exec-masked branches, after which it falls back to vmcnt(0) and the pass pipeline
// collapses).  A clamped chunk multiplies an input that is zero; a clamped row's result is discarded.
template <typename WT, int LPR, int CPL>
__device__ __forceinline__ void load_pass(Raw<WT> (&w)[CPL], const typename WMat<WT>::type& W, int K, int nch, int row, int n_rows,
                                          int lr) {
    const auto wp = wrow(W, (size_t)max(min(row, n_rows - 1), 0), K);  // n_rows = this wave's row_end: surplus slots re-read its own last row
#pragma unroll
    for (int i = 0; i < CPL; ++i) w[i] = load_raw(wp, min(lr + LPR * i, nch - 1));
}

// Per-row epilogue operands, requested together with the row's weights.
template <int MT>
struct RowExtra {
    float bias;
    float resid[MT];
};
template <int MT>
__device__ __forceinline__ RowExtra<MT> load_extra(const GemvArgs& a, int epilogue, int M, int N, int r) {
    RowExtra<MT> e;
    const int rr = min(r, N - 1);
    e.bias = *(a.bias ? a.bias + rr : a.zero);
#pragma unroll
    for (int m = 0; m < MT; ++m)
        e.resid[m] = *((epilogue == EPI_RESIDUAL && m < M) ? a.resid + (size_t)m * a.resid_stride + rr : a.zero);
    return e;
}

// LayerNorm of one input row by ONE wave into its private LDS strip (NJ float4 per lane cover the row).
// Single pass sum / sum of squares; std = sqrt(E[x^2] - mean^2 + eps): reference src/ops.zig:88-101.
// Loads are branch-free (index clamped, surplus zeroed afterwards) so they all fly together.
template <int NJ>
__device__ __forceinline__ void ln_strip(const float* __restrict__ xin, const float* __restrict__ ln_g,
                                         const float* __restrict__ ln_b, f32x4* xw4, int nq, int K, float eps,
                                         int lane) {
    f32x4 v[NJ], g4[NJ], b4[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int ic = min(lane + 64 * j, nq - 1);
        v[j] = reinterpret_cast<const f32x4*>(xin)[ic];
        g4[j] = reinterpret_cast<const f32x4*>(ln_g)[ic];
        b4[j] = reinterpret_cast<const f32x4*>(ln_b)[ic];
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (lane + 64 * j >= nq) v[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float t1 = 0.0f, t2 = 0.0f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        t1 += (v[j].x + v[j].y) + (v[j].z + v[j].w);
        t2 = fmaf(v[j].x, v[j].x, fmaf(v[j].y, v[j].y, fmaf(v[j].z, v[j].z, fmaf(v[j].w, v[j].w, t2))));
    }
    t1 = wave_allsum(t1);
    t2 = wave_allsum(t2);
    const float inv_k = 1.0f / (float)K;
    const float mean = t1 * inv_k;
    const float rstd = __builtin_amdgcn_rsqf(t2 * inv_k - mean * mean + eps);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = lane + 64 * j;
        if (i < nq) {
            f32x4 o;
            o.x = fmaf((v[j].x - mean) * rstd, g4[j].x, b4[j].x);
            o.y = fmaf((v[j].y - mean) * rstd, g4[j].y, b4[j].y);
            o.z = fmaf((v[j].z - mean) * rstd, g4[j].z, b4[j].z);
            o.w = fmaf((v[j].w - mean) * rstd, g4[j].w, b4[j].w);
            xw4[i] = o;
        }
    }
}

// One workgroup = 1..4 waves (M == 1: gemv_plan picks one wave for narrow matrices so that the dispatcher spreads
// them over all CUs, two / four where the waves share one input strip; M > 1: four); each wave owns rows
// [gw * rows_per_wave, +rows_per_wave).
// LPR lanes share one row (RPP = 64 / LPR rows per pass); CPL 16-B chunks per lane per row.
//
// Every kernel of a decode step except lm_head is bound by its chain of dependent memory round
// trips, not by bandwidth, so the structure minimises that chain:
//   * the hot scalars (W, x, N, K, ...) are separate leading kernel arguments so that they are
//     pre-loaded into SGPRs with the wave (kernarg preload) instead of fetched by s_load;
//   * the first pass of weights is requested before anything else;
//   * M == 1: each WAVE builds the transformed input row (LayerNorm / head merge) for itself in a
//     private LDS strip with wave-level reductions only — no workgroup barrier, and the input is
//     fetched 4x per workgroup instead of once per 16-lane group (which made hundreds of waves
//     hammer the same few cache lines).  M > 1: one cooperative build per workgroup;
//   * bias / residual operands of a row travel with the row's weights;
//   * passes are software-pipelined one deep (next pass in flight while this one is reduced).
typedef __attribute__((ext_vector_type(8))) __bf16 mf_bf16x8;
typedef __attribute__((ext_vector_type(4))) float mf_f32x4;

constexpr int kMfmaRows = 8;  // batch rows held in LDS (rows 8..15 of the MFMA tile alias rows 0..7)

// planes: [3][kMfmaRows][S] bytes, S = 2 K + 16 (the 16-B pad spreads the rows over the LDS banks)
__device__ __forceinline__ void store_split4(char* planes, int S, int m, int k, f32x4 v) {
    uint32_t h0, m0, l0, h1, m1, l1;
    split3_pk(v.x, v.y, h0, m0, l0);
    split3_pk(v.z, v.w, h1, m1, l1);
    const u32x2 h = {h0, h1}, md = {m0, m1}, l = {l0, l1};
    const size_t off = (size_t)m * S + (size_t)k * 2;
    const size_t plane = (size_t)kMfmaRows * S;
    *reinterpret_cast<u32x2*>(planes + off) = h;
    *reinterpret_cast<u32x2*>(planes + plane + off) = md;
    *reinterpret_cast<u32x2*>(planes + 2 * plane + off) = l;
}

// Body of gemv_lnk_kernel (gemv_ksplit.hip; the LayerNorm fold is described there), shared with the c_attn role of the fused
// ln_1 + c_attn + attention kernel (attn_qkv.hip).  blk = the workgroup's row block; pf_inc = what block 0 adds to the
// prefetcher's launch counter.  TAGGED (EPI_QKV, one sequence): every output row is also stored as a (value, tag) word at
// tagw[n], tag = *ew << 8 | launch_id, with an agent-scope relaxed store — the hand-over to the attention workgroups of the
// same launch.  The value is the one the epilogue stores to q / the caches; tag_first: the word is stored in front of them
// (AttnArgs.tail_off kAttnTailStoreLast clear).
template <typename WT, int LPR, int CPL, int NP, bool TAGGED>
__device__ __forceinline__ void gemv_lnk_body(int blk, const void* __restrict__ Wv, const float* __restrict__ xin, unsigned ne, int K,
                                              const float* __restrict__ ln_g, const float* __restrict__ c2, const float* __restrict__ c3,
                                              const int* __restrict__ cw, const GemvArgs& a, unsigned pf_inc,
                                              unsigned long long* __restrict__ tagw, const unsigned* __restrict__ ew, unsigned launch_id,
                                              bool tag_first = false) {
    const int N = (int)(ne & 0xffffffu), epilogue = (int)(ne >> 24);
    ZG_STAMP_DECL();
    ZG_STAMP(0);
    constexpr int RPP = 64 / LPR, ROWS = NP * RPP;
    __shared__ float part[4][ROWS];
    __shared__ float stat[4][2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane % LPR, rsub = lane / LPR;
    // The wave's share of K.  bf16 rows of whole 128-byte lines (K % 64 == 0): whole lines per wave — 7, 6, 6, 6 of
    // the 25 at K = 1600 instead of four times 6.25, whose quarters begin mid-line and make every wave touch the
    // boundary lines of its neighbours as well (31 line touches per row instead of 25).
    int kbeg, nchq;
    if (sizeof(WT) == 2 && (K & 63) == 0 && ((K >> 6) & 3) != 0 && (((K >> 6) >> 2) + 1) * 8 <= LPR * CPL) {
        const int lines = K >> 6, base = lines >> 2, rem = lines & 3;
        kbeg = (wave * base + min(wave, rem)) * 64;
        nchq = (base + (wave < rem ? 1 : 0)) * 8;
    } else {
        kbeg = wave * (K >> 2);
        nchq = K >> 5;
    }
    const auto W = wmat<WT>(Wv, kbeg);
    const int row0 = blk * ROWS;
    Raw<WT> wq[NP][CPL];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const auto pr = wrow(W, (size_t)min(row0 + p * RPP + rsub, N - 1), K);
#pragma unroll
        for (int i = 0; i < CPL; ++i) wq[p][i] = load_raw(pr, min(lr + LPR * i, nchq - 1));
    }
    ZG_STAMP(6);  // (6 and 7 split the issue phase: the weight loads issued, then those of x and ln_g)
    W8 xr[CPL], gr[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const size_t off = (size_t)kbeg + (size_t)min(lr + LPR * i, nchq - 1) * 8;
        xr[i] = load_x8(xin + off);
        gr[i] = load_x8(ln_g + off);
    }
    ZG_STAMP(7);
    float c2n = 0.0f, c3n = 0.0f;
    if (tid < ROWS) {
        const int n = min(row0 + tid, N - 1);
        c2n = c2[n];
        c3n = c3[n];
    }
    const int T = max(cw[1], 1);  // KV append position (EPI_QKV)
    const unsigned epoch = TAGGED ? ew[0] : 0u;
    ZG_STAMP(1);
    {   // the argument-block fields of the tail, fetched under the vector loads (zg_common.h ZG_PIN)
        ZG_PIN(a.progress); ZG_PIN(a.y); ZG_PIN(a.y_stride); ZG_PIN(a.epilogue); ZG_PIN(__float_as_uint(a.eps));
        if (epilogue == EPI_QKV) {
            ZG_PIN(a.q); ZG_PIN(a.k_cache); ZG_PIN(a.v_cache); ZG_PIN(a.N); ZG_PIN(a.head_dim); ZG_PIN(a.n_heads); ZG_PIN(a.ctx); ZG_PIN(a.kv_mode); ZG_PIN(a.kv_lo);
        }
    }
    if (TAGGED) { ZG_PIN(tagw); ZG_PIN(launch_id); ZG_PIN((unsigned)tag_first); }
    pf_count(a.progress, pf_inc);
    ZG_STAMP(2);
    // statistics of this wave's quarter (every LPR-lane group holds the whole quarter) and z = g x
    float sx = 0.0f, sxx = 0.0f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        if (lr + LPR * i >= nchq) xr[i] = zero_w8();  // clamped surplus chunks contribute nothing
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sx += xr[i].v[j];
            sxx = fmaf(xr[i].v[j], xr[i].v[j], sxx);
            xr[i].v[j] *= gr[i].v[j];
        }
    }
    sx = group_allsum<LPR>(sx);
    sxx = group_allsum<LPR>(sxx);
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
    if (lane == 0) {
        stat[wave][0] = sx;
        stat[wave][1] = sxx;
    }
    __syncthreads();
    ZG_STAMP(4);
    if (tid < ROWS && row0 + tid < N) {
        const int n = row0 + tid;
        const float inv_k = 1.0f / (float)K;
        const float mean = ((stat[0][0] + stat[1][0]) + (stat[2][0] + stat[3][0])) * inv_k;
        // E[x^2] - mean^2 spelled out as ONE contraction (fmaf(inv_k, sum x^2, -mean^2)): left to the compiler, the contraction
        // it picks depends on the surrounding kernel, and the fused c_attn role (attn_qkv.hip) must round as this kernel does
        const float msq = mean * mean;
        const float var = fmaf(((stat[0][1] + stat[1][1]) + (stat[2][1] + stat[3][1])), inv_k, -msq);
        const float rstd = __builtin_amdgcn_rsqf(var + a.eps);
        const float S1 = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
        const float y = fmaf(rstd, fmaf(-mean, c2n, S1), c3n);
        Best nobest;
        // TAGGED: the word the attention workgroups of this launch wait for leaves FIRST (tag_first), in front of the epilogue's
        // address arithmetic and its q / cache store: it carries the epilogue's own value, acc + bias with the bias in c3
        const float bias_n = 0.0f;
        const unsigned long long tagged_hi = (unsigned long long)((epoch << 8) | launch_id) << 32;
        if (TAGGED && tag_first)
            __hip_atomic_store(tagw + n, tagged_hi | __float_as_uint(y + bias_n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float v = epilogue_row(a, 0, n, y, bias_n, 0.0f, T - 1, nobest);
        if (TAGGED && !tag_first)
            __hip_atomic_store(tagw + n, tagged_hi | __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    ZG_STAMP(5);
    ZG_STAMP_FLUSH();
}

}  // namespace

// ---- launchers of the units: a = the arguments with the plan's layout written in (launch_gemv), p = the plan.  They map the
// plan's template choice to an instantiation and launch dim3(p.grid, p.kslices) x p.block with p.lds bytes; no shape is judged here.
constexpr size_t kGemvLdsMax = 160 * 1024;  // the LDS of a CU
int gemv_launch_ksplit(const GemvArgs& a, const GemvPlan& p, int weight_type, hipStream_t s);
int gemv_launch_lnk(const GemvArgs& a, const GemvPlan& p, int weight_type, hipStream_t s);
int gemv_launch_valu(const GemvArgs& a, const GemvPlan& p, int weight_type, hipStream_t s);  // GR_VALU, GR_GENERIC
int gemv_launch_mfma16(const GemvArgs& a, const GemvPlan& p, hipStream_t s);  // 16-wave kernel (4 waves for lm_head), K slices
int gemv_launch_pl4(const GemvArgs& a, const GemvPlan& p, hipStream_t s);
int gemv_launch_lm_wpt(const GemvArgs& a, const GemvPlan& p, hipStream_t s);

}  // namespace zg
