// attn_decode.h — the fp32-cache decode attention (attn.hip: what it computes and how) as a device function, shared by
// attn_decode_kernel and the attention role of the fused ln_1 + c_attn + attention kernel (attn_qkv.hip), so that both run
// the same arithmetic.  Helpers live in an anonymous namespace: every unit gets its own copy.
#pragma once
#include "zg_kernels.h"

namespace zg {

namespace {

constexpr float kNegBig = -1e30f;

template <typename KV>
__device__ __forceinline__ f32x4 load_kv4(const KV* p);
template <>
__device__ __forceinline__ f32x4 load_kv4<float>(const float* p) {
    return *reinterpret_cast<const f32x4*>(p);
}
template <>
__device__ __forceinline__ f32x4 load_kv4<_Float16>(const _Float16* p) {
    typedef __attribute__((ext_vector_type(4))) _Float16 h4;
    const h4 v = *reinterpret_cast<const h4*>(p);
    f32x4 r;
    r.x = (float)v.x; r.y = (float)v.y; r.z = (float)v.z; r.w = (float)v.w;
    return r;
}

// Butterfly reduce-scatter of 16 values over the 16 lanes of a DPP row: on return lane j of each
// row holds sum over the row's lanes of s[j].
__device__ __forceinline__ float row16_reduce_scatter(float (&s)[16], int lr) {
    // step 1: exchange across lane bit 3 (rotate by 8 == xor 8 inside a 16-lane row)
    float a8[8];
    {
        const bool hi = lr & 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float keep = hi ? s[j + 8] : s[j];
            const float send = hi ? s[j] : s[j + 8];
            a8[j] = keep + dpp_row_ror<8>(send);
        }
    }
    // step 2: across lane bit 2 — xor 4 is not one rotation: take both rotations and select
    float a4[4];
    {
        const bool hi = lr & 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float keep = hi ? a8[j + 4] : a8[j];
            const float send = hi ? a8[j] : a8[j + 4];
            // partner = lr ^ 4.  row_ror:n delivers lane (i - n) mod 16 to lane i, so lanes with
            // bit 2 set take ror 4 (from lr - 4) and the others ror 12 (from lr + 4).
            const float from_lo = dpp_row_ror<4>(send);
            const float from_hi = dpp_row_ror<12>(send);
            a4[j] = keep + (hi ? from_lo : from_hi);
        }
    }
    float a2[2];
    {
        const bool hi = lr & 2;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float keep = hi ? a4[j + 2] : a4[j];
            const float send = hi ? a4[j] : a4[j + 2];
            const float from_lo = dpp_row_ror<2>(send);
            const float from_hi = dpp_row_ror<14>(send);
            a2[j] = keep + (hi ? from_lo : from_hi);
        }
    }
    {
        const bool hi = lr & 1;
        const float keep = hi ? a2[1] : a2[0];
        const float send = hi ? a2[0] : a2[1];
        const float from_lo = dpp_row_ror<1>(send);
        const float from_hi = dpp_row_ror<15>(send);
        return keep + (hi ? from_lo : from_hi);
    }
}

// Diagnostic build (-DZG_STAMPS; tools/kernel_stamps.py): lane 0 of every wave of the attention workgroups of head 0 records
// s_memtime at t0 entry, t1 K / V loads issued, t2 first poll round back, t3 tags matched, t4 arithmetic done, t5 published (wave
// 0; the others: behind the barrier); word 6 = the rounds consumed | held row T - 1 << 32, word 7 = the new row in place (behind
// the row switch, in front of the arithmetic; the compiler may move arithmetic across it); word 8 = 0x10000 | split << 4 | wave.
#ifdef ZG_STAMPS
#define ZG_ASTAMP_DECL() unsigned long long zg_at[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define ZG_ASTAMP(i) zg_at[i] = __builtin_amdgcn_s_memtime()
#define ZG_ASTAMP_SET(i, v) zg_at[i] = (v)
// (behind the round's verdict, so behind the wait for its loads; bit 0: that round did not match)
#define ZG_ASTAMP_FIRST_ROUND(i, spins, ok) \
    if ((spins) == 0) zg_at[i] = (ok) ? __builtin_amdgcn_s_memtime() & ~1ull : __builtin_amdgcn_s_memtime() | 1ull
#define ZG_ASTAMP_FLUSH()                                                                  \
    if (FUSED && a.dbg && h == 0 && lane == 0) {                                           \
        const unsigned long long slot = atomicAdd(a.dbg, 1ull);                            \
        if (slot < 4096) {                                                                 \
            unsigned long long* d = a.dbg + 16 + slot * 10;                                \
            for (int i = 0; i < 8; ++i) d[i] = zg_at[i];                                   \
            d[8] = 0x10000ull | ((unsigned long long)split << 4) | (unsigned long long)wave; \
            d[9] = __builtin_amdgcn_s_memtime();                                           \
        }                                                                                  \
    }
#else
#define ZG_ASTAMP_DECL()
#define ZG_ASTAMP(i)
#define ZG_ASTAMP_SET(i, v)
#define ZG_ASTAMP_FIRST_ROUND(i, spins, ok)
#define ZG_ASTAMP_FLUSH()
#endif

// The argument-block fields the end of an attention workgroup needs (publish_partial), fetched under the K / V loads
#define ZG_PIN_ATTN_TAIL(a) \
    ZG_PIN(a.progress); ZG_PIN(a.part); ZG_PIN(a.max_splits); ZG_PIN(a.pl_out); ZG_PIN(a.part_tag); ZG_PIN(a.launch_id); ZG_PIN(a.merge_cnt); ZG_PIN(a.fault); ZG_PIN(a.spin_limit)
// A (value, tag) word of a tagged hand-over, as the pollers read it: one agent-scope relaxed load; the value is the lower half
__device__ __forceinline__ unsigned long long tagged_load(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float tag_value(unsigned long long w) { return __uint_as_float((unsigned)w); }

// Wave 0 of a split hands over its partial (o[lane], M, l).  Op tier / one sequence: plain stores, the consumer merges
// (attn_merge_kernel, or the c_proj prologue).  Lock-step batch with activation planes (AttnArgs.pl_out): one split of (b, h)
// merges all of them — same arithmetic as merge_attn4 in gemv_internal.h: weights exp(m_s - max m), sums in split order, one
// reciprocal — and writes the head's 64 outputs as the three bf16 planes the c_proj Linear loads as MFMA A fragments
// (zg_common.h plane_elem): the last split by tagged words, or the last to arrive by ticket.
__device__ __forceinline__ void publish_partial(const AttnArgs& a, int n_heads, int nsplit, int b, int h, int split, int lane, float o,
                                                float M, float l, unsigned tag) {
    float* part = a.part + (((size_t)b * n_heads + h) * a.max_splits + split) * kPartStride;
    if (a.pl_out == nullptr) {
        part[lane] = o;
        if (lane == 0) {
            part[64] = M;
            part[65] = l;
        }
        return;
    }
    // nsplit = the launched splits: every one of them publishes
    constexpr int MAXS = 4;  // ctx 1024 / 256; more splits take the loops
    float r = o, lsum = l;
    if (nsplit > 1 && a.part_tag) {
        // Tagged hand-over: every split but the LAST stores (value, tag) words and is done; the last split polls them — one
        // memory-side round trip behind the slowest split instead of the three of the ticket below (drain, ticket, read back).
        // The poller is the last split because a launch's workgroups are dispatched in block order (x, then y = split): the
        // workgroups it waits for are placed BEFORE it, so it can never hold a slot that one of them needs — whatever the
        // occupancy (CU masks, partitions, other resident kernels).  Arithmetic in split order, as the consumer-side merge.
        typedef unsigned long long u64;
        auto pack = [&](float v) { return ((u64)tag << 32) | (u64)__float_as_uint(v); };
        u64* pt0 = a.part_tag + ((size_t)b * n_heads + h) * a.max_splits * kPartStride;  // split 0 of this (sequence, head)
        const int last = nsplit - 1;
        if (split != last) {
            u64* pt = pt0 + split * kPartStride;
            __hip_atomic_store(pt + lane, pack(o), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (lane == 0) {
                __hip_atomic_store(pt + 64, pack(M), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(pt + 65, pack(l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            return;
        }
        r = 0.0f;
        lsum = 0.0f;
        if (nsplit <= MAXS) {
            u64 vo[MAXS - 1], vm[MAXS - 1], vl[MAXS - 1];
            for (int spins = 0;; ++spins) {
                bool ok = true;
#pragma unroll
                for (int s = 0; s < MAXS - 1; ++s) {  // splits 0 .. last - 1; surplus slots re-read the last of them (unused below)
                    const u64* ps = pt0 + min(s, last - 1) * kPartStride;
                    vo[s] = tagged_load(ps + lane);
                    vm[s] = tagged_load(ps + 64);
                    vl[s] = tagged_load(ps + 65);
                    ok = ok && (unsigned)(vo[s] >> 32) == tag && (unsigned)(vm[s] >> 32) == tag && (unsigned)(vl[s] >> 32) == tag;
                }
                if (__builtin_amdgcn_ballot_w64(!ok) == 0) break;
                if ((unsigned)spins >= a.spin_limit) {  // bounded: never hang the queue — and never pass silently
                    if (lane == 0 && a.fault) __hip_atomic_store(a.fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            float ms[MAXS], ls[MAXS], os[MAXS];
#pragma unroll
            for (int s = 0; s < MAXS; ++s) {  // slot s = split s: polled below `last`, this workgroup's own at `last`, weight 0 above
                const bool polled = s < last && s < MAXS - 1;
                ms[s] = polled ? tag_value(vm[s < MAXS - 1 ? s : 0]) : s == last ? M : -1e30f;
                ls[s] = polled ? tag_value(vl[s < MAXS - 1 ? s : 0]) : l;
                os[s] = polled ? tag_value(vo[s < MAXS - 1 ? s : 0]) : o;
            }
            const float mx = fmaxf(fmaxf(ms[0], ms[1]), fmaxf(ms[2], ms[3]));
#pragma unroll
            for (int s = 0; s < MAXS; ++s) {
                const float w = __expf(ms[s] - mx);
                lsum = fmaf(w, ls[s], lsum);
                r = fmaf(w, os[s], r);
            }
        } else {
            // Long contexts: one split is polled at a time, so the maximum is a RUNNING one and this workgroup's own partial comes last:
            // another summation order than the two-pass form, bitwise different by design (test_long_context_merges_more_than_four_splits)
            float mrun = -1e30f;
            for (int s = 0; s <= last; ++s) {
                float m_s = M, o_s = o, l_s = l;
                if (s < last) {
                    const u64* ps = pt0 + s * kPartStride;
                    u64 vo, vm, vl;
                    for (int spins = 0;; ++spins) {
                        vo = tagged_load(ps + lane);
                        vm = tagged_load(ps + 64);
                        vl = tagged_load(ps + 65);
                        const bool ok = (unsigned)(vo >> 32) == tag && (unsigned)(vm >> 32) == tag && (unsigned)(vl >> 32) == tag;
                        if (__builtin_amdgcn_ballot_w64(!ok) == 0) break;
                        if ((unsigned)spins >= a.spin_limit) {
                            if (lane == 0 && a.fault) __hip_atomic_store(a.fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                    }
                    m_s = tag_value(vm);
                    o_s = tag_value(vo);
                    l_s = tag_value(vl);
                }
                const float mnew = fmaxf(mrun, m_s);
                const float w0 = __expf(mrun - mnew), w1 = __expf(m_s - mnew);
                r = fmaf(w1, o_s, r * w0);
                lsum = fmaf(w1, l_s, lsum * w0);
                mrun = mnew;
            }
        }
    } else if (nsplit > 1) {
        typedef __attribute__((address_space(1))) unsigned gu32;
        gu32* gp = (gu32*)part;
        __hip_atomic_store(gp + lane, __float_as_uint(o), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0) {
            __hip_atomic_store(gp + 64, __float_as_uint(M), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(gp + 65, __float_as_uint(l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int* cnt = a.merge_cnt + b * n_heads + h;
        int ticket = 0;
        if (lane == 0) ticket = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ticket = __builtin_amdgcn_readfirstlane(ticket);
        if (ticket != nsplit - 1) return;
        if (lane == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch
        const gu32* p0 = (const gu32*)(a.part + ((size_t)b * n_heads + h) * a.max_splits * kPartStride);
        r = 0.0f;
        lsum = 0.0f;
        auto word = [&](int s, int i) { return __uint_as_float(__hip_atomic_load(p0 + s * kPartStride + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); };
        if (nsplit <= MAXS) {
            float ms[MAXS], ls[MAXS], os[MAXS];
#pragma unroll
            for (int s = 0; s < MAXS; ++s) {  // branch-free: surplus splits re-read the last valid one ...
                ms[s] = word(min(s, nsplit - 1), 64);
                ls[s] = word(min(s, nsplit - 1), 65);
                os[s] = word(min(s, nsplit - 1), lane);
            }
#pragma unroll
            for (int s = 0; s < MAXS; ++s)
                if (s >= nsplit) ms[s] = -1e30f;  // ... and get weight exp(-1e30 - max) == 0
            const float mx = fmaxf(fmaxf(ms[0], ms[1]), fmaxf(ms[2], ms[3]));
#pragma unroll
            for (int s = 0; s < MAXS; ++s) {
                const float w = __expf(ms[s] - mx);
                lsum = fmaf(w, ls[s], lsum);
                r = fmaf(w, os[s], r);
            }
        } else {
            float mx = -1e30f;
            for (int s = 0; s < nsplit; ++s) mx = fmaxf(mx, word(s, 64));
            for (int s = 0; s < nsplit; ++s) {
                const float w = __expf(word(s, 64) - mx);
                lsum = fmaf(w, word(s, 65), lsum);
                r = fmaf(w, word(s, lane), r);
            }
        }
    }
    const float v = r * (1.0f / lsum);
    uint32_t hi, mid, lo;  // (store_planes, spelled out: the element index is formed behind the split here)
    split3_pk(v, 0.0f, hi, mid, lo);
    const int k = h * 64 + lane;
    a.pl_out[plane_elem(0, b, k)] = (bf16_t)hi;
    a.pl_out[plane_elem(1, b, k)] = (bf16_t)mid;
    a.pl_out[plane_elem(2, b, k)] = (bf16_t)lo;
}

// One workgroup (head h, split, sequence b) of the decode attention: launched as grid (H, max_splits, B), block 256; requires
// head_dim == 64.  FUSED (one sequence, model tier): q and the new row T - 1 come from the tagged words qkv_tag [3][H * 64]
// of this step instead of q / the caches — see the fused kernel in attn_qkv.hip.
// Arguments (zg_common.h ZG_PIN): the 14 preloaded dwords carry everything a K/V address depends on — q, k, v, the three
// strides (32-bit element counts; bit 31 of st = "sequence length from the control block"), th = t_hi | heads << 20 — plus the two words
// read through a pointer, cw = step control block and ew = epoch of the tags (always readable addresses).  The first
// version took the AttnArgs block alone: its K/V loads were issued behind two dependent scalar round trips (kernarg
// block, then the sequence length behind the control-block pointer in it).
template <typename KV, bool FUSED>
__device__ __forceinline__ void attn_decode_body(int h, int split, int b, const float* __restrict__ qp, const void* __restrict__ kp,
                                                 const void* __restrict__ vp, unsigned sb, unsigned sh, unsigned st, unsigned th,
                                                 const int* __restrict__ cw, const unsigned* __restrict__ ew, const AttnArgs& a,
                                                 const unsigned long long* __restrict__ qkv_tag) {
    __shared__ __attribute__((aligned(16))) float s_o[4][64];
    __shared__ float s_m[4], s_l[4];
    const int t_hi = (int)(th & 0xfffffu), n_heads = (int)(th >> 20);  // (grid sizes are scalar loads from the kernarg segment)
    // t_hi: launch-time upper bound of the sequence length (seq_len itself in the op tier, the
    // 64-position bucket of the captured graph in the model tier).  Every K/V load below depends
    // only on t_hi, so it is in flight while the exact seq_len is still being fetched from the
    // device control block; seq_len is needed for masking alone.
    const int Tc = cw[1];
    const unsigned epoch = ew[0];
    const int T = (st >> 31) ? Tc : t_hi;
    const size_t stride_t = st & 0x7fffffffu;
    const int chunk0 = split * kAttnChunk;
    if (chunk0 >= t_hi) return;  // nothing to attend to in this split (consumer skips it too)

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, g = lane >> 4;
    const int base = chunk0 + wave * 64;

    const KV* K = reinterpret_cast<const KV*>(kp) + (size_t)b * sb + (size_t)h * sh;
    const KV* V = reinterpret_cast<const KV*>(vp) + (size_t)b * sb + (size_t)h * sh;
    f32x4 q4 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!FUSED) q4 = *reinterpret_cast<const f32x4*>(qp + ((size_t)b * n_heads + h) * 64 + lr * 4);
    const float alpha = 0.125f;  // 1 / sqrt(64), applied to the dot product like sgemm alpha (ops.zig:275)

    float m_w = kNegBig, l_w = 0.0f;
    f32x4 o4 = {0.0f, 0.0f, 0.0f, 0.0f};
    ZG_ASTAMP_DECL();
    ZG_ASTAMP(0);
    if (base < t_hi) {
        // ---- all K and V loads up front: position t = base + 4*i + g, dims 4*lr .. 4*lr+3
        // Branch-free: positions at or beyond t_hi re-read the last valid row (their probability is exactly 0 below: t >= t_hi
        // >= T).  With `if (t < t_hi) load else 0` the compiler merged one loaded component with its zero in a fresh
        // register right behind the second pair of loads — a vmcnt wait, i.e. a whole memory round trip, in the middle of
        // the load sequence, with 14 of the 16 pairs not yet issued.
        f32x4 k4[16], v4[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int t = min(base + 4 * i + g, t_hi - 1);
            k4[i] = load_kv4<KV>(K + (size_t)t * stride_t + lr * 4);
            v4[i] = load_kv4<KV>(V + (size_t)t * stride_t + lr * 4);
        }
        ZG_PIN_ATTN_TAIL(a); ZG_PIN(a.tail_off);
        pf_count(a.progress);
        ZG_ASTAMP(1);
        if (FUSED) {
            // ---- this step's q of head h and, in the wave that holds position T - 1, the new k / v row: (value, tag) words the
            // c_attn workgroups of this launch store (gemv_lnk_body TAGGED), polled with a bound behind the K / V loads above.
            // The loads above use the standalone kernel's addresses, so row T - 1 was also read from the cache, racing with its
            // append: those registers are overwritten below.  Every other position reads the row the two-launch path reads, with
            // one exception — when T == t_hi and t_hi is not a multiple of 64 (a context size that is not), the lanes clamped to
            // t_hi - 1 = T - 1 re-read the row being appended.  Their probability is exactly 0, so the result is still bitwise the
            // same as long as the old row is finite (the state arena is zeroed at create; caches are cleared behind a prompt).
            typedef unsigned long long u64;
            const int E = n_heads * 64;
            const unsigned tag = (epoch << 8) | a.launch_id;
            const int rel = __builtin_amdgcn_readfirstlane(T - 1 - base);  // position T - 1 within this wave's 64
            const bool holder = (unsigned)rel < 64u;
            const u64* wq = qkv_tag + h * 64 + lr * 4;
            // A lane's four words of q (of k, of v) are 32 contiguous, 32-byte-aligned bytes: two 16-byte sc1 loads instead of four
            // 8-byte ones — a round of 2 (holder: 6) vector-memory instructions instead of 4 (12), so the holder samples the
            // producers' words at twice the rate (AttnArgs.tail_off kAttnPollNarrow set: the 8-byte loads).  Every 8-byte half is
            // still validated by its own tag.  What this relies on: an aligned 8-byte (value, tag) word stored by ONE store is never
            // seen torn inside a 16-byte sc1 load — observed on gfx950, as for the 8-byte load, not an architectural guarantee; the
            // two words of one load may be of different steps, which the per-word tags catch.  The loads go through a buffer
            // descriptor over the 3 E words (sc1 = aux bit 4: served by the L2 like the agent-scope loads).
            const bool wide = (a.tail_off & kAttnPollNarrow) == 0;
            const __amdgpu_buffer_rsrc_t rt =
                __builtin_amdgcn_make_buffer_rsrc(const_cast<u64*>(qkv_tag), 0, (unsigned)(3 * E) * 8u, 0x00020000);
            const unsigned oq = (unsigned)(h * 64 + lr * 4) * 8u, oe = (unsigned)E * 8u;
            u64 wv[12];
            unsigned spins = 0;
            for (;; ++spins) {
                bool ok = true;
                if (wide) {
                    asm volatile("" ::: "memory");  // (a poll: every round loads again)
                    u32x4 w[6];
                    w[0] = __builtin_amdgcn_raw_buffer_load_b128(rt, oq, 0, 16);
                    w[1] = __builtin_amdgcn_raw_buffer_load_b128(rt, oq + 16u, 0, 16);
                    if (holder) {
                        w[2] = __builtin_amdgcn_raw_buffer_load_b128(rt, oq + oe, 0, 16);
                        w[3] = __builtin_amdgcn_raw_buffer_load_b128(rt, oq + oe + 16u, 0, 16);
                        w[4] = __builtin_amdgcn_raw_buffer_load_b128(rt, oq + 2u * oe, 0, 16);
                        w[5] = __builtin_amdgcn_raw_buffer_load_b128(rt, oq + 2u * oe + 16u, 0, 16);
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        wv[2 * j] = ((u64)w[j].y << 32) | w[j].x;
                        wv[2 * j + 1] = ((u64)w[j].w << 32) | w[j].z;
                        ok = ok && w[j].y == tag && w[j].w == tag;
                    }
                    if (holder) {
#pragma unroll
                        for (int j = 2; j < 6; ++j) {
                            wv[2 * j] = ((u64)w[j].y << 32) | w[j].x;
                            wv[2 * j + 1] = ((u64)w[j].w << 32) | w[j].z;
                            ok = ok && w[j].y == tag && w[j].w == tag;
                        }
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        wv[j] = tagged_load(wq + j);
                        ok = ok && (unsigned)(wv[j] >> 32) == tag;
                    }
                    if (holder) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            wv[4 + j] = tagged_load(wq + E + j);
                            wv[8 + j] = tagged_load(wq + 2 * E + j);
                            ok = ok && (unsigned)(wv[4 + j] >> 32) == tag && (unsigned)(wv[8 + j] >> 32) == tag;
                        }
                    }
                }
                const bool all = __builtin_amdgcn_ballot_w64(!ok) == 0;
                ZG_ASTAMP_FIRST_ROUND(2, spins, all);
                if (all) break;
                if (spins >= a.spin_limit) {  // bounded: never hang the queue — and never pass silently (check_fault)
                    if (lane == 0 && a.fault) __hip_atomic_store(a.fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            ZG_ASTAMP(3);
            ZG_ASTAMP_SET(6, (unsigned long long)(spins + 1) | ((unsigned long long)holder << 32));
            q4 = f32x4{tag_value(wv[0]), tag_value(wv[1]), tag_value(wv[2]), tag_value(wv[3])};
            if (holder && g == (rel & 3)) {
                const f32x4 kn = {tag_value(wv[4]), tag_value(wv[5]), tag_value(wv[6]), tag_value(wv[7])};
                const f32x4 vn = {tag_value(wv[8]), tag_value(wv[9]), tag_value(wv[10]), tag_value(wv[11])};
                // (this branch — code only the holder wave runs, once per launch — costs it 770 ticks of s_memtime; two ways round
                // it were built and measured, and neither gained anything in the step that clears the noise: profiles/NOTEBOOK.md §22)
                switch (rel >> 2) {  // (uniform: a scalar branch to one register pair)
#define ZG_NEW_ROW(i) case i: k4[i] = kn; v4[i] = vn; break;
                    ZG_NEW_ROW(0) ZG_NEW_ROW(1) ZG_NEW_ROW(2) ZG_NEW_ROW(3) ZG_NEW_ROW(4) ZG_NEW_ROW(5) ZG_NEW_ROW(6) ZG_NEW_ROW(7)
                    ZG_NEW_ROW(8) ZG_NEW_ROW(9) ZG_NEW_ROW(10) ZG_NEW_ROW(11) ZG_NEW_ROW(12) ZG_NEW_ROW(13) ZG_NEW_ROW(14) ZG_NEW_ROW(15)
#undef ZG_NEW_ROW
                }
            }
            ZG_ASTAMP(7);
        }
        // ---- partial dots, then reduce-scatter: lane (g, j) ends with the score of t = base + 4*j + g
        float s[16];
#pragma unroll
        for (int i = 0; i < 16; ++i)
            s[i] = fmaf(q4.x, k4[i].x, fmaf(q4.y, k4[i].y, fmaf(q4.z, k4[i].z, q4.w * k4[i].w)));
        float sc = row16_reduce_scatter(s, lr) * alpha;
        const int t_mine = base + 4 * lr + g;
        if (t_mine >= T) sc = kNegBig;
        // ---- wave softmax statistics
        m_w = wave_allmax(sc);
        const float p = (t_mine < T) ? __expf(sc - m_w) : 0.0f;
        l_w = wave_allsum(p);
        // ---- o += p_t * V_t ; p of position (i, g) lives in lane g*16 + i
        // lane i of each 16-lane row to the whole row: DPP row_newbcast, no LDS crossbar
#define ZG_PV(i)                                                                                                         \
    {                                                                                                                    \
        const float pi = __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(p), 0x150 + (i), 0xF, 0xF, false)); \
        o4.x = fmaf(pi, v4[i].x, o4.x);                                                                                  \
        o4.y = fmaf(pi, v4[i].y, o4.y);                                                                                  \
        o4.z = fmaf(pi, v4[i].z, o4.z);                                                                                  \
        o4.w = fmaf(pi, v4[i].w, o4.w);                                                                                  \
    }
        ZG_PV(0) ZG_PV(1) ZG_PV(2) ZG_PV(3) ZG_PV(4) ZG_PV(5) ZG_PV(6) ZG_PV(7)
        ZG_PV(8) ZG_PV(9) ZG_PV(10) ZG_PV(11) ZG_PV(12) ZG_PV(13) ZG_PV(14) ZG_PV(15)
#undef ZG_PV
        // sum the four position groups (lanes 16 apart)
        o4.x += __shfl_xor(o4.x, 16, 64); o4.y += __shfl_xor(o4.y, 16, 64);
        o4.z += __shfl_xor(o4.z, 16, 64); o4.w += __shfl_xor(o4.w, 16, 64);
        o4.x += __shfl_xor(o4.x, 32, 64); o4.y += __shfl_xor(o4.y, 32, 64);
        o4.z += __shfl_xor(o4.z, 32, 64); o4.w += __shfl_xor(o4.w, 32, 64);
        ZG_ASTAMP(4);
    }
    if (lane < 16) *reinterpret_cast<f32x4*>(&s_o[wave][lane * 4]) = o4;
    if (lane == 0) {
        s_m[wave] = m_w;
        s_l[wave] = l_w;
    }
    __syncthreads();
    if (wave == 0) {
        const float M = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
        float o = 0.0f, l = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float sc = __expf(s_m[w] - M);
            o = fmaf(sc, s_o[w][lane], o);
            l = fmaf(sc, s_l[w], l);
        }
        publish_partial(a, n_heads, (t_hi + kAttnChunk - 1) / kAttnChunk, b, h, split, lane, o, M, l, (epoch << 8) | a.launch_id);
    }
    ZG_ASTAMP(5);
    ZG_ASTAMP_FLUSH();
}

}  // namespace

}  // namespace zg
