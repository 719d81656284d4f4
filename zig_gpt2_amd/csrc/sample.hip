// sample.hip — the head of a decode step and the stages of the device sampler behind lm_head (model tier): embed_step_kernel,
// the plain sampler's three kernels, and — as included headers, one per stage — truncation (sample_filter.h), penalties
// (sample_penalty.h), history-dependent bans (sample_ban.h), logit edits (sample_edit.h), guided decoding (sample_guide.h), log-probabilities (sample_logprob.h), scoring (sample_score.h), the stop
// conditions (sample_stop.h) and beam search (sample_beam.h), with every stage's launcher and workspace carver.  What the stages share — the pick from lm_head's
// argmax partials, the row maximum, the rebuild of a slice's partial — is in sample_common.h; the order of picks itself
// (pick_before), clamp_token and counter_uniform are in zg_common.h.
#include <algorithm>

#include "zg_kernels.h"

namespace zg {

namespace {

#include "sample_common.h"

// Head of one decode step (single workgroup).  Follows generate/sample of src/main.zig:322-342
// with greedy argmax: picks the token fed at position s, records outputs, writes
// x = wte[token] + wpe[s] (GPT.forward, src/main.zig:179-183), publishes seq_len = s + 1 and
// advances the step counter so that the same captured graph serves every position.
// Latency-bound: the argmax partials of the previous step are fetched speculatively together with
// the control words (one memory round trip), one wave per sequence; only the wte row depends on
// the chosen token (second round trip).
__global__ __launch_bounds__(512) void embed_step_kernel(StepCtrl* ctrl, const float* part_val, const int* part_idx, int part_stride, int n_partials,
                                                         const int* prompt, const int* prompt_len, int batch, int prompt_stride, const EmbedArgs a) {
    // 14 preloaded dwords (zg_common.h ZG_PIN, rule 1): what the loads at entry are addressed by — the control block, the argmax
    // partials with their count and stride, the prompt rows — so the control words and the partials leave in one round trip.  `a`
    // is the whole block as the host fills it (launch_embed_step passes those nine again as its leading parameters); the kernel
    // reads only its other fields from it, pinned under the partial loads.
    __shared__ int s_tok[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = ctrl->step;
    const int mode = ctrl->mode;
    const int npart = n_partials;
    const int n_waves = batch > 4 ? 8 : 4;  // as launched (blockDim is a scalar load from the kernarg segment)
    for (int b = wave; b < batch; b += n_waves) {
        // speculative fetch of this sequence's partial maxima (valid memory whether or not needed).  This is partials_first
        // (sample_common.h: the rounds, the order pick_before, wave_first) WRITTEN OUT: the argument block is pinned between the loads
        // and the first compare, and through the helpers the compares become selects that cost this kernel six more SGPRs (103: seven
        // waves a SIMD for eight).  tests/test_pick_rows_gpu.py holds this text and the shared one to the same rule.
        float bv = kPickStartVal;
        int bi = kPickStartIdx;
        // eight partials per lane per round, loads first and branch-free (clamped): a load-compare loop is one dependent memory
        // round trip per 64 partials — seven of them for the 393 partials of 124M, most of this kernel's time
        for (int base = 0; base < npart; base += 512) {
            float pv[8];
            int pi[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int p = min(base + lane + 64 * j, npart - 1);
                pv[j] = part_val[(size_t)b * part_stride + p];
                pi[j] = part_idx[(size_t)b * part_stride + p];
            }
            {   // the argument-block fields used further down, fetched under the partial-maxima loads (zg_common.h ZG_PIN, rule 2)
                ZG_PIN(a.forced); ZG_PIN(a.wte); ZG_PIN(a.wpe); ZG_PIN(a.weight_type); ZG_PIN(a.n_embed); ZG_PIN(a.cur_token); ZG_PIN(a.out_tokens);
                ZG_PIN(a.out_stride); ZG_PIN(a.x); ZG_PIN(a.pl_out); ZG_PIN(a.pl_g); ZG_PIN(a.epoch); ZG_PIN(a.finish_only); ZG_PIN(a.st_out); ZG_PIN(a.vocab);
                ZG_PIN(a.progress); ZG_PIN(a.sampled);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {  // (a clamped duplicate of the last partial changes nothing)
                if (pv[j] > bv || (pv[j] == bv && pi[j] < bi)) { bv = pv[j]; bi = pi[j]; }
            }
        }
        if (b == 0 && a.progress != nullptr && a.finish_only == 0 && lane == 0) {
            // a step at sequence length s + 1 starts; block 0 of every launch of this queue lands on the XCD this block is on
            const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u;  // HW_REG_XCC_ID
            const unsigned long long word = ((unsigned long long)(0x100u | xcc) << 32) | (((unsigned)(s + 1) << 8) | 1u);
            __hip_atomic_store(static_cast<unsigned long long*>(__builtin_assume_aligned(a.progress, 8)), word, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
#ifdef ZG_STAMPS
            reinterpret_cast<PfCtl*>(a.progress)->xcd_log[0] = 0x100u | xcc;
#endif
        }
        const int np = prompt_len ? prompt_len[b] : 0;
        const int p_cur = prompt[(size_t)b * prompt_stride + min(s, prompt_stride - 1)];
        const int p_last = prompt[(size_t)b * prompt_stride + max(min(np, prompt_stride) - 1, 0)];
        const int forced = a.forced[b];
        const int drawn = a.sampled[b];  // (mode 2; always a readable address)
        // argmax over the wave (wave_first, written out): DPP row rotations inside the 16-lane rows, then every lane folds in the
        // four row winners through v_readlane — all lanes end with the wave's pick
#define ZG_AM_STEP(N)                                                                                                   \
    {                                                                                                                   \
        const float ov = dpp_row_ror<N>(bv);                                                                            \
        const int oi = __builtin_amdgcn_update_dpp(0, bi, 0x120 | N, 0xF, 0xF, true);                                   \
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }                                                     \
    }
        ZG_AM_STEP(8) ZG_AM_STEP(4) ZG_AM_STEP(2) ZG_AM_STEP(1)
#undef ZG_AM_STEP
        {
            const float rv = bv;
            const int ri = bi;
#pragma unroll
            for (int r = 0; r < 64; r += 16) {
                const float ov = lane_value(rv, r);
                const int oi = __builtin_amdgcn_readlane(ri, r);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
        }
        // logits that are all NaN compare false everywhere and leave the start value standing: index 0 then, as a loop that starts at
        // logits[0] and keeps what compares greater (the oracle, and the reference's order of comparison) — never an index past
        // the vocabulary, which the gather below would follow out of the table (a NaN in a checkpoint must not fault the GPU)
        int g = clamp_token(bi, a.vocab);
        if (mode == 2 && a.finish_only != 2) g = clamp_token(drawn, a.vocab);  // the sampler's draw takes the pick's place
        // the pick of step s-1 exists iff that step ran lm_head (main.zig:337)
        const bool have_pick = a.finish_only == 2 || ((mode != 1) && (s >= 1) && (s - 1 >= np));
        if (lane == 0) {
            if (have_pick) {
                if (a.finish_only == 2) a.cur_token[b] = g;  // zg_gpt_argmax, zg_debug_pick_rows
                else a.out_tokens[(size_t)b * a.out_stride + (s - 1)] = g;
            }
            if (a.finish_only == 0 || a.finish_only == 3) {
                int tok;
                if (mode == 1) tok = forced;
                else if (s < np) tok = p_cur;      // main.zig:331-334: prompt token s
                else if (s == np) tok = p_last;    // main.zig:337: the previous token is fed again
                else tok = g;
                if (mode != 1 && s < np) a.out_tokens[(size_t)b * a.out_stride + s] = tok;
                a.cur_token[b] = tok;
                s_tok[b] = tok;
            }
        }
    }
    if (a.finish_only == 1 || a.finish_only == 2) return;
    __syncthreads();
    const int total4 = batch * (a.n_embed >> 2);
    for (int i = threadIdx.x; i < total4; i += 64 * n_waves) {
        const int b = i / (a.n_embed >> 2), e = (i % (a.n_embed >> 2)) * 4;
        const int tok = s_tok[b];
        f32x4 o;
        if (a.weight_type == WT_BF16) {
            const u32x2 t = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(a.wte) + (size_t)tok * a.n_embed + e);
            const u32x2 p = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(a.wpe) + (size_t)s * a.n_embed + e);
            o.x = bf16_lo(t.x) + bf16_lo(p.x);
            o.y = bf16_hi(t.x) + bf16_hi(p.x);
            o.z = bf16_lo(t.y) + bf16_lo(p.y);
            o.w = bf16_hi(t.y) + bf16_hi(p.y);
        } else if (a.weight_type == WT_B24) {
            o = load_b24x4(a.wte, (size_t)tok, a.n_embed, e) + load_b24x4(a.wpe, (size_t)s, a.n_embed, e);
        } else {
            const f32x4 t = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(a.wte) + (size_t)tok * a.n_embed + e);
            const f32x4 p = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(a.wpe) + (size_t)s * a.n_embed + e);
            o = t + p;
        }
        *reinterpret_cast<f32x4*>(a.x + (size_t)b * a.n_embed + e) = o;
        // the first Linear of the lock-step batch reads its input as planes of g * x (the planes of one 32-k step are 8 x 32 apart)
        if (a.pl_out) store_split3x4(a.pl_out + plane_elem(0, b, e), 8 * 32, o * *reinterpret_cast<const f32x4*>(a.pl_g + e));
        if (a.st_out) {  // LayerNorm statistics by 16-column tile: four consecutive threads hold one tile of one row
            float s1 = (o.x + o.y) + (o.z + o.w);
            float s2 = fmaf(o.x, o.x, fmaf(o.y, o.y, fmaf(o.z, o.z, o.w * o.w)));
            s1 += __shfl_xor(s1, 1, 64); s2 += __shfl_xor(s2, 1, 64);
            s1 += __shfl_xor(s1, 2, 64); s2 += __shfl_xor(s2, 2, 64);
            if ((threadIdx.x & 3) == 0) *reinterpret_cast<float2*>(a.st_out + ((size_t)b * (a.n_embed >> 4) + (e >> 4)) * 2) = float2{s1, s2};
        }
    }
    if (threadIdx.x == 0 && a.epoch) *a.epoch += 1u;  // a step starts: new tags for its hand-overs
    if (threadIdx.x == 0 && a.finish_only == 0) {
        ctrl->seq_len = s + 1;
        ctrl->step = s + 1;
    }
}

// softmax(x / temp) and the weighted draw of GPT.sample (src/main.zig:200-206; std.rand weightedIndex: the first index whose
// running sum exceeds u x total), in three small kernels behind lm_head.  History: one workgroup per row with a contiguous chunk of
// 50 logits per lane and a 1024-step serial scan (~100 us per row at V = 50257); then one workgroup with coalesced passes and
// segment sums (28 us: a single CU has ~100 cache lines in flight against ~2 us of memory-side latency for 1600 lines of logits
// that another XCD's lm_head just wrote).  Now:
//   sample_seg_kernel   many workgroups: the row maximum comes from lm_head's argmax partials (no pass over the logits), every
//                       wave sums e = exp(x / temp - max) over SEGMENTS of 64 consecutive elements (786 at V = 50257)
//   sample_pick_kernel  one wave per row walks the segment sums IN INDEX ORDER (64 lanes x consecutive runs of segments, a scan
//                       over the lanes, the owning lane walks its run), then scans the 64 elements of the segment that holds
//                       u x total lane by lane.  Sums inside a segment and over lanes are tree-shaped: the draw can differ from a
//                       strictly left-to-right sum only where u x total lies within rounding (~1e-7) of a boundary.
//   sample_probs_kernel (only when the caller wants them) leaves the probabilities in the logits row, as the reference does.
// NaN probabilities (no interval holds the point) give the last index.  vocab <= 64 x 4096.
constexpr int kSegMax = 4096;  // segment sums per row; [kSegMax] = the row maximum / temp, [kSegMax + 1] = the total

// The parameters are one entry per row (params[b]; a uniform call stages equal entries), and a row's FORM is its own: PLAIN when
// its entry switches on neither filter nor min-p.  A plain row keeps the plain kernels' arithmetic — plain_weight below, the row
// maximum scaled by 1 / temp in [kSegMax], no threshold — also inside a chain launched for a neighbour's filters: the branch is
// uniform over the workgroup, which serves one row.
__device__ __forceinline__ bool row_is_plain(const SampleParams& p) { return p.top_k == 0u && !(p.top_p < 1.0f) && !(p.min_p_off > -INFINITY); }
__device__ __forceinline__ float plain_weight(float x, float inv_temp, float mx) { return __expf(x * inv_temp - mx); }

__global__ __launch_bounds__(256) void sample_seg_kernel(const float* __restrict__ logits, int vocab, const SampleParams* params, float inv_temp_arg,
                                                         const float* __restrict__ part_val, int n_part, int part_stride, float* __restrict__ seg_out) {
    __shared__ float s_red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const float inv_temp = params ? params[b].inv_temp : inv_temp_arg;
    const float* x = logits + (size_t)b * vocab;
    float* so = seg_out + (size_t)b * (kSegMax + 2);
    const float mx = row_max_from_partials(part_val + (size_t)b * part_stride, n_part, s_red) * inv_temp;
    const int nseg = (vocab + 63) >> 6;
    for (int sg = blockIdx.x * 4 + wave; sg < nseg; sg += gridDim.x * 4) {
        const int i = sg * 64 + lane;
        const float e = i < vocab ? plain_weight(x[i], inv_temp, mx) : 0.0f;
        const float t = wave_allsum(e);
        if (lane == 0) so[sg] = t;
    }
    if (blockIdx.x == 0 && tid == 0) so[kSegMax] = mx;
}

// FILT (top-k / top-p, sample_filter.h): elements under the row's threshold tau[b] weigh nothing, and where rounding leaves
// the point past every interval the pick falls on the last KEPT element (never on a dropped one).  A plain row of a FILT launch
// (row_is_plain) runs the text of the plain instance: `filt` is FILT narrowed by the row's own form.
template <bool FILT>
__global__ __launch_bounds__(64) void sample_pick_kernel(const float* __restrict__ logits, int vocab, const SampleParams* params, float inv_temp_arg,
                                                         const float* __restrict__ u_arr, const StepCtrl* ctrl, float* __restrict__ seg_io,
                                                         int* __restrict__ token_out, const float* __restrict__ tau_arr) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const bool filt = FILT && !row_is_plain(params[b]);
    const float tau = filt ? tau_arr[b] : 0.0f;
    const float inv_temp = params ? params[b].inv_temp : inv_temp_arg;
    const float* x = logits + (size_t)b * vocab;
    float* so = seg_io + (size_t)b * (kSegMax + 2);
    // no uniforms given: the counter PRNG of (seed, sequence length of the step whose logits these are, sequence)
    const float u = u_arr ? u_arr[b] : counter_uniform(params[b].seed, (unsigned long long)ctrl->seq_len, (unsigned long long)b);
    const int nseg = (vocab + 63) >> 6;
    const int run = (nseg + 63) >> 6, s0 = lane * run, s1 = min(s0 + run, nseg);
    const float mx = so[kSegMax];
    float local = 0.0f;
    for (int k = s0; k < s1; ++k) local += so[k];
    float incl = local;  // inclusive scan over the lanes, in lane order
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    const float total = __shfl(incl, 63, 64);
    const float point = u * total;
    int pick = vocab - 1;
    unsigned long long hit = __builtin_amdgcn_ballot_w64(s0 < s1 && point < incl);
    if (hit != 0ull) {
        const int owner = __builtin_ctzll(hit);
        int sg = 0;
        float before = 0.0f;
        if (lane == owner) {  // the owning lane walks its run of segments
            before = incl - local;
            sg = s1 - 1;
            for (int k = s0; k < s1; ++k) {
                const float v = so[k];
                if (point < before + v) {
                    sg = k;
                    break;
                }
                before += v;
            }
        }
        sg = __shfl(sg, owner, 64);
        before = __shfl(before, owner, 64);
        const int i = sg * 64 + lane;
        const float xi = i < vocab ? x[i] : 0.0f;
        const bool kept = i < vocab && (!filt || xi >= tau);
        float c = kept ? (filt ? __expf((xi - mx) * inv_temp) : plain_weight(xi, inv_temp, mx)) : 0.0f;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float up = __shfl_up(c, off, 64);
            if (lane >= off) c += up;
        }
        const unsigned long long in = __builtin_amdgcn_ballot_w64(kept && point < before + c);
        // (rounding between the segment sum and its lane-by-lane scan can leave the point just past the last lane: that lane then)
        pick = sg * 64 + (in != 0ull ? __builtin_ctzll(in) : min(63, vocab - 1 - sg * 64));
        if (filt && in == 0ull) {
            const unsigned long long kb = __builtin_amdgcn_ballot_w64(kept);
            if (kb != 0ull) pick = sg * 64 + 63 - __builtin_clzll(kb);
            else hit = 0ull;  // (the walk ended on a segment that keeps nothing: as below)
        }
    }
    if (filt && hit == 0ull) {  // the point at or past the total (u x total rounded up): the last kept element of the last segment that weighs anything
        int ls = -1;
        for (int k = s0; k < s1; ++k)
            if (so[k] > 0.0f) ls = k;
        const unsigned long long lb = __builtin_amdgcn_ballot_w64(ls >= 0);
        if (lb != 0ull) {
            const int sg = __shfl(ls, 63 - __builtin_clzll(lb), 64);
            const int i = sg * 64 + lane;
            const unsigned long long kb = __builtin_amdgcn_ballot_w64(i < vocab && x[i] >= tau);
            if (kb != 0ull) pick = sg * 64 + 63 - __builtin_clzll(kb);
        }
    }
    if (lane == 0) {
        token_out[b] = pick;
        so[kSegMax + 1] = total;
    }
}

__global__ __launch_bounds__(256) void sample_probs_kernel(float* logits, int vocab, const SampleParams* params, float inv_temp_arg,
                                                           const float* __restrict__ seg_io) {
    const int b = blockIdx.y;
    const float inv_temp = params ? params[b].inv_temp : inv_temp_arg;
    float* x = logits + (size_t)b * vocab;
    const float* so = seg_io + (size_t)b * (kSegMax + 2);
    const float mx = so[kSegMax], inv = 1.0f / so[kSegMax + 1];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < vocab; i += gridDim.x * 256) x[i] = plain_weight(x[i], inv_temp, mx) * inv;
}

#include "sample_filter.h"
#include "sample_penalty.h"
#include "sample_ban.h"
#include "sample_edit.h"
#include "sample_guide.h"
#include "sample_logprob.h"
#include "sample_score.h"
#include "sample_stop.h"
#include "sample_beam.h"

// What every sampler chain checks of the vocabulary, and the grid of its segment kernel: four segments of 64 per workgroup
int seg_grid(int vocab, int* nb) {
    ZG_REQUIRE(vocab >= 1 && vocab <= 64 * kSegMax, ZG_ERR_UNSUPPORTED, "sampler: vocabulary of %d beyond %d", vocab, 64 * kSegMax);
    const int nseg = (vocab + 63) / 64;
    *nb = std::min(128, (nseg + 3) / 4);
    return ZG_OK;
}

int sample_launches(float* logits, int batch, int vocab, const SampleParams* params, float inv_temp, const float* u, const StepCtrl* ctrl,
                    const float* part_val, int n_part, int part_stride, float* seg_ws, int* token_out, bool write_probs, hipStream_t s) {
    int nb;
    ZG_TRY(seg_grid(vocab, &nb));
    ZG_REQUIRE(part_val && n_part >= 1 && seg_ws && token_out, ZG_ERR_ARG, "sampler: missing argmax partials / workspace");
    hipLaunchKernelGGL(sample_seg_kernel, dim3(nb, batch), dim3(256), 0, s, logits, vocab, params, inv_temp, part_val, n_part, part_stride, seg_ws);
    ZG_HIP(hipGetLastError());
    hipLaunchKernelGGL(sample_pick_kernel<false>, dim3(batch), dim3(64), 0, s, logits, vocab, params, inv_temp, u, ctrl, seg_ws, token_out,
                       (const float*)nullptr);
    ZG_HIP(hipGetLastError());
    if (write_probs) {
        hipLaunchKernelGGL(sample_probs_kernel, dim3(std::min(256, (vocab + 255) / 256), batch), dim3(256), 0, s, logits, vocab, params, inv_temp, seg_ws);
        ZG_HIP(hipGetLastError());
    }
    return ZG_OK;
}

inline int logprob_chunks(int vocab) { return (vocab + kLpChunk - 1) / kLpChunk; }

}  // namespace

int launch_embed_step(const EmbedArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(embed_step_kernel, dim3(1), dim3(a.batch > 4 ? 512 : 256), 0, s, a.ctrl, a.part_val, a.part_idx, a.part_stride, a.n_partials,
                       a.prompt, a.prompt_len, a.batch, a.prompt_stride, a);  // one wave per sequence
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_sample(float* logits, int batch, int vocab, const SampleParams* params, float temp, const float* u, const float* part_val, int n_part,
                  int part_stride, float* seg_ws, int* token_out, bool write_probs, hipStream_t s) {
    ZG_REQUIRE(u != nullptr, ZG_ERR_ARG, "sampler: a per-call launch without its uniforms");
    return sample_launches(logits, batch, vocab, params, params ? 0.0f : 1.0f / temp, u, nullptr, part_val, n_part, part_stride, seg_ws, token_out, write_probs, s);
}

int launch_sample_step(float* logits, int batch, int vocab, const SampleParams* params, const StepCtrl* ctrl, const float* part_val, int n_part,
                       int part_stride, float* seg_ws, int* token_out, hipStream_t s) {
    return sample_launches(logits, batch, vocab, params, 0.0f, nullptr, ctrl, part_val, n_part, part_stride, seg_ws, token_out, false, s);
}

size_t sample_workspace_floats(int batch) { return (size_t)batch * (kSegMax + 2); }

size_t filter_workspace_bytes(int batch) { return (size_t)batch * (3 * kFiltBins * 12 + 2 * sizeof(FilterState) + 8); }

FilterWs filter_workspace(void* base, int batch) {
    FilterWs w;
    char* p = static_cast<char*>(base);
    w.mass = reinterpret_cast<unsigned long long*>(p);
    p += (size_t)batch * 3 * kFiltBins * 8;
    w.cnt = reinterpret_cast<unsigned*>(p);
    p += (size_t)batch * 3 * kFiltBins * 4;
    w.st = p;
    p += (size_t)batch * 2 * sizeof(FilterState);
    w.tau = reinterpret_cast<float*>(p);
    return w;
}

int launch_sample_filtered(float* logits, int batch, int vocab, const SampleParams* params, int n_levels, const float* u, const StepCtrl* ctrl,
                           const float* part_val, int n_part, int part_stride, float* seg_ws, const FilterWs& fws, int* token_out, bool write_probs,
                           hipStream_t s) {
    int nb;
    ZG_TRY(seg_grid(vocab, &nb));
    ZG_REQUIRE(params && part_val && n_part >= 1 && seg_ws && token_out && fws.mass && (n_levels == 0 || n_levels == 3 || n_levels == 6) && (u || ctrl), ZG_ERR_ARG,
               "truncated sampler: missing argument");
    const int nlb = std::min(64, (vocab + 1023) / 1024);  // ~4 elements per thread: the level kernels pay per workgroup (bin scan, histogram flush)
    for (int pos = 1; pos <= n_levels; ++pos) {
        hipLaunchKernelGGL(filter_level_kernel, dim3(nlb, batch), dim3(256), 0, s, logits, vocab, params, part_val, n_part, part_stride, fws, pos, n_levels);
        ZG_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(sample_seg_filt_kernel, dim3(nb, batch), dim3(256), 0, s, logits, vocab, params, part_val, n_part, part_stride, seg_ws, fws, n_levels);
    ZG_HIP(hipGetLastError());
    hipLaunchKernelGGL(sample_pick_kernel<true>, dim3(batch), dim3(64), 0, s, logits, vocab, params, 0.0f, u, ctrl, seg_ws, token_out, fws.tau);
    ZG_HIP(hipGetLastError());
    if (write_probs) {
        hipLaunchKernelGGL(sample_probs_filt_kernel, dim3(std::min(256, (vocab + 255) / 256), batch), dim3(256), 0, s, logits, vocab, params, seg_ws, fws.tau);
        ZG_HIP(hipGetLastError());
    }
    return ZG_OK;
}

int launch_row_max_partials(const float* logits, int batch, int vocab, float* part_val, int n_part, hipStream_t s) {
    ZG_REQUIRE(logits && part_val && batch >= 1 && vocab >= 1 && n_part >= 1 && n_part <= 4096, ZG_ERR_ARG, "row_max_partials: bad argument");
    hipLaunchKernelGGL(row_max_partials_kernel, dim3(n_part, batch), dim3(256), 0, s, logits, vocab, part_val);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_penalize(float* logits, int batch, int vocab, const PenParams* params, const PenHistory& h, float* part_val, int* part_idx, int n_part,
                    unsigned* counts_out, hipStream_t s, bool rebuild) {
    ZG_REQUIRE(logits && params && part_val && part_idx && batch >= 1 && vocab >= 1 && n_part >= 1 && n_part <= 4096, ZG_ERR_ARG,
               "penalties: missing argument");
    ZG_REQUIRE(h.max_hist >= 0 && h.max_hist <= kPenMaxHistory, ZG_ERR_UNSUPPORTED, "penalties: a history of %d tokens exceeds the %d the LDS table holds",
               h.max_hist, kPenMaxHistory);
    int slots = 64;
    while (slots < 2 * h.max_hist) slots *= 2;
    const size_t lds = (size_t)slots * 2 * sizeof(unsigned);
    if (lds > 64 * 1024) {  // opt in once, like every other launcher here
        static bool raised = false;
        if (!raised) {
            ZG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&penalty_apply_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       2 * kPenMaxHistory * 2 * (int)sizeof(unsigned)));
            raised = true;
        }
    }
    hipLaunchKernelGGL(penalty_apply_kernel, dim3(batch), dim3(256), lds, s, logits, vocab, params, h, slots, counts_out);
    ZG_HIP(hipGetLastError());
    if (!rebuild) return ZG_OK;
    hipLaunchKernelGGL(row_argmax_partials_kernel, dim3(n_part, batch), dim3(256), 0, s, logits, vocab, part_val, part_idx);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_ban(float* logits, int batch, int vocab, const BanArgs& a, const PenHistory& h, hipStream_t s) {
    ZG_REQUIRE(logits && a.rules && (h.ctrl ? a.prompt_len != nullptr : a.picked != nullptr) && batch >= 1 && batch <= kBanMaxRows && vocab >= 1, ZG_ERR_ARG,
               "bans: missing argument");
    ZG_REQUIRE(h.max_hist >= 0 && h.max_hist <= kPenMaxHistory, ZG_ERR_UNSUPPORTED, "bans: a history of %d tokens exceeds the %d the LDS holds", h.max_hist,
               kPenMaxHistory);
    hipLaunchKernelGGL(ban_apply_kernel, dim3(batch), dim3(256), (size_t)h.max_hist * sizeof(int), s, logits, vocab, a, h);  // (at most 32 KB: no opt-in)
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_row_argmax_partials(const float* logits, int batch, int vocab, float* part_val, int* part_idx, int n_part, hipStream_t s) {
    ZG_REQUIRE(logits && part_val && part_idx && batch >= 1 && vocab >= 1 && n_part >= 1 && n_part <= 4096, ZG_ERR_ARG, "row_argmax_partials: bad argument");
    hipLaunchKernelGGL(row_argmax_partials_kernel, dim3(n_part, batch), dim3(256), 0, s, logits, vocab, part_val, part_idx);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_logit_edit(float* logits, int batch, int vocab, const EditTable* tab, const unsigned* keep, float* part_val, int* part_idx, int n_part,
                      hipStream_t s) {
    ZG_REQUIRE(logits && tab && keep && part_val && part_idx && batch >= 1 && vocab >= 1 && n_part >= 1 && n_part <= 4096, ZG_ERR_ARG,
               "logit edits: missing argument");
    hipLaunchKernelGGL(logit_edit_kernel, dim3(n_part, batch), dim3(256), 0, s, logits, vocab, tab, keep, part_val, part_idx);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_guide_mask(float* logits, int batch, int vocab, const EditTable* tab, const unsigned* keep, const GuideArgs& g, float* part_val, int* part_idx,
                      int n_part, hipStream_t s) {
    ZG_REQUIRE(logits && g.keep && g.n_states && g.state && (g.ctrl == nullptr || g.prompt_len) && (tab == nullptr) == (keep == nullptr) && part_val && part_idx &&
                   batch >= 1 && vocab >= 1 && n_part >= 1 && n_part <= 4096,
               ZG_ERR_ARG, "guide mask: missing argument");
    hipLaunchKernelGGL(guide_mask_kernel, dim3(n_part, batch), dim3(256), 0, s, logits, vocab, tab, keep, g, part_val, part_idx);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_guide_advance(const GuideArgs& g, const int* picks, int batch, int vocab, hipStream_t s) {
    ZG_REQUIRE(g.next && g.n_states && g.state && (g.ctrl == nullptr || g.prompt_len) && (g.rec == nullptr || g.rec_stride >= 1) && picks && batch >= 1 &&
                   batch <= 64 && vocab >= 1,
               ZG_ERR_ARG, "guide advance: missing argument");
    hipLaunchKernelGGL(guide_advance_kernel, dim3(1), dim3(64), 0, s, g, picks, batch, vocab);  // one lane per row
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

size_t logprob_workspace_bytes(int batch, int vocab) { return (size_t)batch * logprob_chunks(vocab) * (1 + 2 * kLpTopMax) * 4; }

LogprobWs logprob_workspace(void* base, int batch, int vocab) {
    const size_t slots = (size_t)batch * logprob_chunks(vocab);
    LogprobWs w;
    w.sum = static_cast<float*>(base);
    w.val = w.sum + slots;
    w.idx = reinterpret_cast<int*>(w.val + slots * kLpTopMax);
    return w;
}

int launch_logprob(const float* logits, int batch, int vocab, const float* part_val, const int* part_idx, int n_part, int part_stride, const int* top_n,
                   const LogprobWs& ws, const int* tokens, const StepCtrl* ctrl, const int* prompt_len, const LogprobRec& rec, hipStream_t s) {
    ZG_REQUIRE(vocab >= 1 && vocab <= kLpChunk * kLpMaxChunks, ZG_ERR_UNSUPPORTED, "log-probabilities: vocabulary of %d beyond %d", vocab,
               kLpChunk * kLpMaxChunks);
    ZG_REQUIRE(logits && part_val && (tokens || part_idx) && n_part >= 1 && top_n && ws.sum && rec.logprob && rec.top_ids && rec.top_logprobs &&
                   rec.stride >= 1 && batch >= 1,
               ZG_ERR_ARG, "log-probabilities: missing argument");
    const int nc = logprob_chunks(vocab);
    hipLaunchKernelGGL(logprob_part_kernel, dim3(nc, batch), dim3(256), 0, s, logits, vocab, part_val, n_part, part_stride, top_n, ws, nc);
    ZG_HIP(hipGetLastError());
    hipLaunchKernelGGL(logprob_finish_kernel, dim3(batch), dim3(256), 0, s, logits, vocab, part_val, part_idx, n_part, part_stride, top_n, ws, nc, tokens,
                       ctrl, prompt_len, rec);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

size_t score_workspace_bytes(int rows, int vocab) { return (size_t)rows * logprob_chunks(vocab) * (2 + 2 * kLpTopMax) * 4; }

ScoreWs score_workspace(void* base, int rows, int vocab) {
    const size_t slots = (size_t)rows * logprob_chunks(vocab);
    ScoreWs w;
    w.lp.sum = static_cast<float*>(base);
    w.max = w.lp.sum + slots;
    w.lp.val = w.max + slots;
    w.lp.idx = reinterpret_cast<int*>(w.lp.val + slots * kLpTopMax);
    return w;
}

int launch_score(const float* logits, int rows, int vocab, int row_stride, const int* top_n, const ScoreWs& ws, const ScoreTargets& tg, const LogprobRec& rec,
                 hipStream_t s) {
    ZG_REQUIRE(vocab >= 1 && vocab <= kLpChunk * kLpMaxChunks, ZG_ERR_UNSUPPORTED, "score: vocabulary of %d beyond %d", vocab, kLpChunk * kLpMaxChunks);
    ZG_REQUIRE(logits && top_n && ws.lp.sum && tg.tokens && tg.token_stride >= 1 && tg.n >= 1 && tg.past >= 0 && tg.row0 >= 0 && rec.logprob && rec.top_ids &&
                   rec.top_logprobs && rec.stride >= 1 && rows >= 1 && rows <= 65535 && row_stride >= vocab,
               ZG_ERR_ARG, "score: missing argument");
    const int nc = logprob_chunks(vocab);
    hipLaunchKernelGGL(score_part_kernel, dim3(nc, rows), dim3(256), 0, s, logits, vocab, row_stride, top_n, ws, nc);
    ZG_HIP(hipGetLastError());
    hipLaunchKernelGGL(score_finish_kernel, dim3(rows), dim3(256), 0, s, logits, vocab, row_stride, top_n, ws, nc, tg, rec);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_stop(const StopArgs& a, hipStream_t s) {
    ZG_REQUIRE(a.conds && a.tokens && a.prompt_len && a.finish_col && a.reason && a.stride >= 1 && a.batch >= 1 && a.batch <= kStopMaxRows && a.vocab >= 1 &&
                   (a.col >= 0 ? a.col < a.stride : a.ctrl != nullptr) && (a.picks || a.pick_from_record || (a.part_val && a.part_idx && a.n_part >= 1)),
               ZG_ERR_ARG, "stop stage: missing argument");
    hipLaunchKernelGGL(stop_step_kernel, dim3(1), dim3(a.batch > 4 ? 512 : 256), 0, s, a);  // one wave per row
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_beam(const BeamArgs& a, hipStream_t s) {
    ZG_REQUIRE(a.st && a.lenpow && a.n_lenpow >= 2 && a.top_ids && a.top_logprobs && a.sampled && a.parent && a.score && a.logprob && a.stride >= 1 &&
                   a.batch >= 1 && a.batch <= kBeamRows && a.vocab >= 1 && (a.col >= 0 ? a.col < a.stride : a.ctrl != nullptr),
               ZG_ERR_ARG, "beam stage: missing argument");
    hipLaunchKernelGGL(beam_step_kernel, dim3(1), dim3(64 * kBeamRows), 0, s, a);  // one wave per group
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

}  // namespace zg
