// sample_filter.h — top-k / nucleus (top-p) truncation in front of the sampler: the kernels (included by sample.hip
// behind sample_seg / sample_pick / sample_probs, inside its unnamed namespace).
//
// For one row x[0..V): tau_k = the k-th largest value (duplicates counted), K = { x >= tau_k }; e = exp(x / temp - max / temp) over
// K, tau_p = the largest value v of K with sum{ e : x >= v } >= top_p * sum{ e : K }; kept = { x >= max(tau_k, tau_p) } — ties at
// a threshold stay together, -0.0 and +0.0 are one value, the top token is always kept.  The sampler then runs with weight 0
// under the threshold.
//
// The threshold is found EXACTLY by a radix select over order-preserving 32-bit keys, 11 / 11 / 10 bits per level, many
// workgroups per row and one launch per level:
//   filter_level_kernel (position i of the chain)   searches the histogram its predecessor built (every workgroup re-scans the
//                         <= 2048 bins: the bin where the running count reaches the rank still wanted / the running mass reaches
//                         top_p x total) and so fixes 11 more key bits; then builds the histogram of the next level over the elements
//                         that match the key bits fixed so far: LDS atomics per workgroup, non-empty bins added to the row's histogram.
//   sample_seg_filt_kernel   searches the last histogram (the key is complete: tau), then sums the segments as sample_seg_kernel
//                         does, elements under tau weighing nothing.
// One filter = 3 level launches + the segment kernel in sample_seg_kernel's place (3 added launches); top-k AND top-p = 6 levels
// (the nucleus descent runs over K, which is known only when tau_k is: 6 added launches).
// Masses are 64-bit fixed point (e x 2^32, integer atomics): the thresholds do not depend on the order in which workgroups
// arrive.  Counts and masses of a row live in three histograms used in turn: the launch at position i reads [(i-1) % 3], adds to
// [i % 3] and zeroes [(i+1) % 3] (which its predecessor has read and its successor will fill); [1] is zero when a chain starts
// (the arena is zeroed at create, launch 3 and 6 leave it zero).  The state of the descent (key prefix, rank left, mass above, target,
// tau_k's key) goes from launch to launch through two slots per row used in turn, written by workgroup 0.
// NaN logits: keys above +inf, weight 0; whatever threshold comes out, every index stays below the vocabulary.
// min-p (include/zgpt2.h zg_logit_edits): tau_m = row maximum + SampleParams.min_p_off joins the threshold where sample_seg_filt_kernel
// completes it — kept = { x >= max(tau_k, tau_p, tau_m) } —, and alone (both filters off) it is a chain of zero levels: no selection
// launch, sample_seg_filt_kernel with tau = tau_m and the threshold-aware pick / probability kernels behind it.
// Per-row parameters: n_levels is the chain's, the descents are the row's own (filt_kind: K then nothing, nothing
// then P, K then P, or none).  Where a row has no descent it still zeroes its share of the histogram in turn — so the rotation
// above holds for every row whatever its neighbours run — and hands its state on unchanged; a top-k-only row of a six-level chain
// keeps tau_k's key as its prefix (no nucleus descent at top_p 1, which could cut elements whose fixed-point mass rounds to 0), a
// row with neither filter ends with tau = -inf before min-p, and a plain row takes the plain kernels' arithmetic (sample.hip).

constexpr int kFiltBins = 2048;
constexpr float kFiltScale = 4294967296.0f;  // fixed-point masses: e in [0, 1] x 2^32; a row of 2^18 elements sums below 2^51 (exact in a double)

struct FilterState {
    unsigned prefix;   // the key bits fixed so far
    unsigned k_rem;    // top-k: the rank still wanted among the keys that match the prefix
    unsigned lo_key;   // (top-k and top-p) tau_k's key: the nucleus descent sees nothing below it
    unsigned pad;
    unsigned long long mass_above;  // top-p: mass of the keys above the prefix's range
    unsigned long long target;      // top-p: top_p x the mass of K
};

// the row's part of a FilterWs
struct FilterRow {
    unsigned* cnt;             // [3][kFiltBins]
    unsigned long long* mass;  // [3][kFiltBins]
    FilterState* st;           // [2]
};
__device__ __forceinline__ FilterRow filter_row(const FilterWs& ws, int b) {
    return FilterRow{ws.cnt + (size_t)b * 3 * kFiltBins, ws.mass + (size_t)b * 3 * kFiltBins, static_cast<FilterState*>(ws.st) + (size_t)b * 2};
}

// order-preserving key of a float (larger value = larger key), -0.0 taken as +0.0
__device__ __forceinline__ unsigned filter_key(float x) {
    unsigned u = __float_as_uint(x);
    if ((u & 0x7fffffffu) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float filter_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__device__ __forceinline__ int filt_shift(int lv) { return lv == 0 ? 21 : lv == 1 ? 10 : 0; }
__device__ __forceinline__ int filt_bins(int lv) { return lv == 2 ? 1024 : 2048; }
// kind of descent d (0 / 1) of ONE ROW in a chain of n_levels launches: three launches hold the row's one filter (top-k if it is
// on, else the nucleus), six hold top-k in the first three and the nucleus in the last three — each only where the row has it
enum { FILT_SKIP = 0, FILT_K = 1, FILT_P = 2 };
__device__ __forceinline__ int filt_kind(int n_levels, int d, bool k_on, bool p_on) {
    if (n_levels == 3) return k_on ? FILT_K : p_on ? FILT_P : FILT_SKIP;
    return d == 0 ? (k_on ? FILT_K : FILT_SKIP) : (p_on ? FILT_P : FILT_SKIP);
}

__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int off) {
    const unsigned lo = __shfl_up((unsigned)v, off, 64), hi = __shfl_up((unsigned)(v >> 32), off, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// One level's search, by the whole workgroup (256 threads, all of them call): the bins of a histogram are walked from the top; the
// hit is the first bin at which the running count reaches st.k_rem (by_mass false) or st.mass_above + the running mass reaches
// st.target (by_mass; set_target: the target is top_p x this histogram's total first).  The bin's bits join the prefix, what lay
// above it leaves the rank / joins the mass.  Nothing reached (NaN games): the lowest bin.
__device__ void filter_search(const unsigned* __restrict__ cnt, const unsigned long long* __restrict__ mass, int lv, bool by_mass, bool set_target,
                              float top_p, FilterState& st) {
    __shared__ unsigned s_wc[4];
    __shared__ unsigned long long s_wm[4];
    __shared__ unsigned s_hit[2];
    __shared__ unsigned long long s_hitm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = filt_bins(lv), per = nb >> 8;  // 8 or 4 bins per thread, thread 0 the topmost
    unsigned c[8];
    unsigned long long m[8];
    unsigned cs = 0;
    unsigned long long ms = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int bin = nb - 1 - (tid * per + i);
        c[i] = i < per ? cnt[bin] : 0u;
        m[i] = (i < per && by_mass) ? mass[bin] : 0ull;
        cs += c[i];
        ms += m[i];
    }
    unsigned ci = cs;  // inclusive scan over the threads, topmost bins first
    unsigned long long mi = ms;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned uc = __shfl_up(ci, off, 64);
        const unsigned long long um = shfl_up_u64(mi, off);
        if (lane >= off) {
            ci += uc;
            mi += um;
        }
    }
    __syncthreads();  // (the shared words of an earlier search of this launch are no longer read)
    if (lane == 63) {
        s_wc[wave] = ci;
        s_wm[wave] = mi;
    }
    __syncthreads();
    unsigned long long total_m = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) {
            ci += s_wc[w];
            mi += s_wm[w];
        }
        total_m += s_wm[w];
    }
    unsigned long long target = st.target;
    if (set_target) {
        target = (unsigned long long)((double)top_p * (double)total_m);
        if (target < 1ull) target = 1ull;
        if (target > total_m) target = total_m;
    }
    const unsigned k_rem = st.k_rem;
    const unsigned long long above = st.mass_above;
    auto reached = [&](unsigned cc, unsigned long long mm) { return by_mass ? above + mm >= target : cc >= k_rem; };
    unsigned ce = ci - cs;
    unsigned long long me = mi - ms;
    const bool last_resort = tid == 255 && !reached(ci, mi);
    if ((!reached(ce, me) && reached(ci, mi)) || last_resort) {
        int hit = 0;
        unsigned hc = 0;
        unsigned long long hm = 0;
        bool found = false;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < per && !found) {
                hit = nb - 1 - (tid * per + i);
                hc = ce;
                hm = me;
                ce += c[i];
                me += m[i];
                found = reached(ce, me);
            }
        }
        s_hit[0] = (unsigned)hit;
        s_hit[1] = hc;
        s_hitm = hm;
    }
    __syncthreads();
    st.prefix |= s_hit[0] << filt_shift(lv);
    st.k_rem = k_rem - s_hit[1];
    st.mass_above = above + s_hitm;
    st.target = target;
}

// e x 2^32 of one element (NaN and anything outside [0, 1]: clamped).  The truncated kernels take the maximum off BEFORE the
// division by the temperature — (x - max) / temp, exact at the top token whatever the magnitude — where the plain sampler computes
// x / temp - max / temp (contracted to an fma, which a row of 1e30s turns into exp(+rounding error of max / temp)).
__device__ __forceinline__ unsigned long long filter_mass(float x, float inv_temp, float mx) {
    const float e = fminf(fmaxf(__expf((x - mx) * inv_temp), 0.0f), 1.0f);
    return (unsigned long long)(e * kFiltScale);
}

__device__ __forceinline__ void filter_zero(const FilterRow& r, int which) {
    for (int bin = blockIdx.x * 256 + threadIdx.x; bin < kFiltBins; bin += gridDim.x * 256) {
        r.cnt[which * kFiltBins + bin] = 0u;
        r.mass[which * kFiltBins + bin] = 0ull;
    }
}

// the search a launch at position pos (> 1) owes its predecessor; leaves the state as the build of position pos wants it
__device__ void filter_advance(const FilterRow& r, int pos, int n_levels, bool k_on, bool p_on, float top_p, FilterState& st) {
    st = r.st[(pos - 1) & 1];
    const int dp = (pos - 2) / 3, lp = (pos - 2) % 3, kind = filt_kind(n_levels, dp, k_on, p_on);
    const int h = (pos - 1) % 3;
    if (kind != FILT_SKIP) filter_search(r.cnt + h * kFiltBins, r.mass + h * kFiltBins, lp, kind == FILT_P, kind == FILT_P && lp == 0, top_p, st);
    if (lp == 2 && dp == 0 && n_levels == 6 && p_on) {  // tau_k is known: the nucleus descent starts over, above it (a row without one keeps tau_k's key)
        st.lo_key = kind == FILT_SKIP ? 0u : st.prefix;
        st.prefix = 0u;
        st.mass_above = 0ull;
    }
}

__global__ __launch_bounds__(256) void filter_level_kernel(const float* __restrict__ logits, int vocab, const SampleParams* __restrict__ params,
                                                           const float* __restrict__ part_val, int n_part, int part_stride, FilterWs ws, int pos,
                                                           int n_levels) {
    __shared__ unsigned s_cnt[kFiltBins];
    __shared__ unsigned long long s_mass[kFiltBins];
    __shared__ float s_red[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const FilterRow r = filter_row(ws, b);
    const float inv_temp = params[b].inv_temp, top_p = params[b].top_p;
    const unsigned top_k = params[b].top_k;
    const bool k_on = top_k != 0u && top_k < (unsigned)vocab, p_on = top_p < 1.0f;
    filter_zero(r, (pos + 1) % 3);
    FilterState st{0u, top_k, 0u, 0u, 0ull, 0ull};
    if (pos > 1) filter_advance(r, pos, n_levels, k_on, p_on, top_p, st);
    if (blockIdx.x == 0 && tid == 0) r.st[pos & 1] = st;
    const int d = (pos - 1) / 3, lv = (pos - 1) % 3, kind = filt_kind(n_levels, d, k_on, p_on);
    if (kind == FILT_SKIP) return;
    const int nb = filt_bins(lv), sh = filt_shift(lv);
    for (int i = tid; i < nb; i += 256) {
        s_cnt[i] = 0u;
        s_mass[i] = 0ull;
    }
    const float mx = row_max_from_partials(part_val + (size_t)b * part_stride, n_part, s_red);  // (its barrier also covers the zeroing above)
    const float* x = logits + (size_t)b * vocab;
    const int msh = lv == 1 ? 21 : 10;  // the prefix bits a key must match at levels 1 and 2
    for (int i = blockIdx.x * 256 + tid; i < vocab; i += gridDim.x * 256) {
        const float v = x[i];
        const unsigned key = filter_key(v);
        if (key < st.lo_key || (lv != 0 && (key >> msh) != (st.prefix >> msh))) continue;
        const unsigned bin = (key >> sh) & (unsigned)(nb - 1);
        atomicAdd(&s_cnt[bin], 1u);
        if (kind == FILT_P) atomicAdd(&s_mass[bin], filter_mass(v, inv_temp, mx));
    }
    __syncthreads();
    const int h = pos % 3;
    for (int i = tid; i < nb; i += 256) {
        const unsigned cc = s_cnt[i];
        if (cc != 0u) {
            atomicAdd(&r.cnt[h * kFiltBins + i], cc);
            const unsigned long long mm = s_mass[i];
            if (mm != 0ull) atomicAdd(&r.mass[h * kFiltBins + i], mm);
        }
    }
}

// sample_seg_kernel behind a chain of n_levels filter launches: the last search completes the key of tau (n_levels 0: no chain,
// tau is min-p's alone)
__global__ __launch_bounds__(256) void sample_seg_filt_kernel(const float* __restrict__ logits, int vocab, const SampleParams* __restrict__ params,
                                                              const float* __restrict__ part_val, int n_part, int part_stride, float* __restrict__ seg_out,
                                                              FilterWs ws, int n_levels) {
    __shared__ float s_red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
    const FilterRow r = filter_row(ws, b);
    const float inv_temp = params[b].inv_temp, top_p = params[b].top_p;
    const unsigned top_k = params[b].top_k;
    const bool k_on = top_k != 0u && top_k < (unsigned)vocab, p_on = top_p < 1.0f;
    const bool plain = row_is_plain(params[b]);
    const int pos = n_levels + 1;
    float tau = -INFINITY;
    if (n_levels != 0) {  // (0: min-p alone — no chain ran, the workspace is not touched)
        filter_zero(r, (pos + 1) % 3);
        FilterState st;
        filter_advance(r, pos, n_levels, k_on, p_on, top_p, st);
        if (k_on || p_on) tau = filter_unkey(st.prefix);  // (a row without a filter: the chain was its neighbours')
    }
    const float* x = logits + (size_t)b * vocab;
    float* so = seg_out + (size_t)b * (kSegMax + 2);
    const float mx = row_max_from_partials(part_val + (size_t)b * part_stride, n_part, s_red);  // [kSegMax] holds the row maximum itself here
    const int nseg = (vocab + 63) >> 6;
    if (plain) {  // sample_seg_kernel's text: the maximum scaled by 1 / temp, nothing cut
        const float mxs = mx * inv_temp;
        if (blockIdx.x == 0 && tid == 0) ws.tau[b] = -INFINITY;
        for (int sg = blockIdx.x * 4 + wave; sg < nseg; sg += gridDim.x * 4) {
            const int i = sg * 64 + lane;
            const float e = i < vocab ? plain_weight(x[i], inv_temp, mxs) : 0.0f;
            const float t = wave_allsum(e);
            if (lane == 0) so[sg] = t;
        }
        if (blockIdx.x == 0 && tid == 0) so[kSegMax] = mxs;
        return;
    }
    // min-p (applied last, as HF does): tau_m = max + temp x log(min_p), one fp32 add; off (-inf): tau keeps its own bits, a NaN's too
    const float d = params[b].min_p_off;
    if (d > -INFINITY) tau = fmaxf(tau, mx + d);
    if (blockIdx.x == 0 && tid == 0) ws.tau[b] = tau;
    for (int sg = blockIdx.x * 4 + wave; sg < nseg; sg += gridDim.x * 4) {
        const int i = sg * 64 + lane;
        const float v = i < vocab ? x[i] : 0.0f;
        const float e = (i < vocab && v >= tau) ? __expf((v - mx) * inv_temp) : 0.0f;
        const float t = wave_allsum(e);
        if (lane == 0) so[sg] = t;
    }
    if (blockIdx.x == 0 && tid == 0) so[kSegMax] = mx;
}

// sample_probs_kernel with exact 0 under the threshold
__global__ __launch_bounds__(256) void sample_probs_filt_kernel(float* logits, int vocab, const SampleParams* __restrict__ params,
                                                                const float* __restrict__ seg_io, const float* __restrict__ tau_arr) {
    const int b = blockIdx.y;
    float* x = logits + (size_t)b * vocab;
    const float* so = seg_io + (size_t)b * (kSegMax + 2);
    const float mx = so[kSegMax], inv = 1.0f / so[kSegMax + 1], inv_temp = params[b].inv_temp, tau = tau_arr[b];
    if (row_is_plain(params[b])) {  // sample_probs_kernel's text ([kSegMax] holds the scaled maximum for such a row)
        for (int i = blockIdx.x * 256 + threadIdx.x; i < vocab; i += gridDim.x * 256) x[i] = plain_weight(x[i], inv_temp, mx) * inv;
        return;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < vocab; i += gridDim.x * 256) {
        const float v = x[i];
        x[i] = v >= tau ? __expf((v - mx) * inv_temp) * inv : 0.0f;
    }
}

// the row maxima by slice, as lm_head's argmax epilogue leaves them (zg_debug_sample_rows: logits without an lm_head)
__global__ __launch_bounds__(256) void row_max_partials_kernel(const float* __restrict__ logits, int vocab, float* __restrict__ part_val) {
    __shared__ float s_red[4];
    const float* x = logits + (size_t)blockIdx.y * vocab;
    slice_partial_store(x, vocab, slice_thread_max(x, vocab), s_red, nullptr, part_val, nullptr);  // (the index is not wanted)
}
