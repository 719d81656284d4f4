// sample_common.h — the row primitives every stage of the device sampler shares (sample.hip includes it in front of the stage
// headers, inside its unnamed namespace): the pick from lm_head's argmax partials under zg_common.h pick_before, the row maximum
// from those partials, and the rebuild of one slice's partial behind a stage that rewrote the row.  All of them are for
// workgroups of four waves (256 threads) unless they say "wave".

// Where a pick starts: below every finite logit, and an index that loses every tie and that clamp_token turns into token 0.  A
// row of NaNs, or of -inf, leaves it standing.
constexpr float kPickStartVal = -3.0e38f;
constexpr int kPickStartIdx = 0x7fffffff;

// One wave's first (value, index) under pick_before; every lane ends with it.  DPP row rotations inside the 16-lane rows, then
// every lane folds in the four row winners (its own among them) through v_readlane (six rounds of ds_bpermute pairs were ~0.3 us
// of dependent LDS-crossbar hops).  The order is total over what can win, so the winner does not depend on the tree's shape.
template <int N>
__device__ __forceinline__ void wave_first_step(float& bv, int& bi) {
    const float ov = dpp_row_ror<N>(bv);
    const int oi = __builtin_amdgcn_update_dpp(0, bi, 0x120 | N, 0xF, 0xF, true);
    if (pick_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
}
__device__ __forceinline__ void wave_first(float& bv, int& bi) {
    wave_first_step<8>(bv, bi);
    wave_first_step<4>(bv, bi);
    wave_first_step<2>(bv, bi);
    wave_first_step<1>(bv, bi);
    const float rv = bv;
    const int ri = bi;
#pragma unroll
    for (int r = 0; r < 64; r += 16) {
        const float ov = lane_value(rv, r);
        const int oi = __builtin_amdgcn_readlane(ri, r);
        if (pick_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
}

// One wave's pick from a row's argmax partials part_val / part_idx [n_part]: rounds of eight partials per lane, loads first and
// branch-free (clamped: a duplicate of the last partial changes nothing) — a load-compare loop is one dependent memory round trip
// per 64 partials, seven of them for the 393 partials of 124M.  A load half and a fold half, then whole.  (embed_step_kernel, which
// pins its argument block between the halves, has this text written out: sample.hip says why.)  The index is returned as stored:
// clamp_token makes it a token.
__device__ __forceinline__ void partials_load(const float* part_val, const int* part_idx, int n_part, int base, float (&pv)[8], int (&pi)[8]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int p = min(base + lane + 64 * j, n_part - 1);
        pv[j] = part_val[p];
        pi[j] = part_idx[p];
    }
}
__device__ __forceinline__ void partials_fold(const float (&pv)[8], const int (&pi)[8], float& bv, int& bi) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (pick_before(pv[j], pi[j], bv, bi)) { bv = pv[j]; bi = pi[j]; }
}
__device__ __forceinline__ int partials_first(const float* part_val, const int* part_idx, int n_part) {
    float bv = kPickStartVal;
    int bi = kPickStartIdx;
    for (int base = 0; base < n_part; base += 512) {
        float pv[8];
        int pi[8];
        partials_load(part_val, part_idx, n_part, base, pv, pi);
        partials_fold(pv, pi, bv, bi);
    }
    wave_first(bv, bi);
    return bi;
}

// The maximum over a workgroup of four waves through the LDS (s_red[4], not read by anyone still); every lane receives it
__device__ __forceinline__ float block4_allmax(float v, float* s_red) {
    v = wave_allmax(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
}

// The row maximum = the maximum of the per-workgroup maxima lm_head's argmax epilogue (or a stage behind it that rebuilt them)
// left in part_row [n_part]: no pass over the logits.  Never below -3e38.
__device__ __forceinline__ float row_max_from_partials(const float* __restrict__ part_row, int n_part, float* s_red) {
    float mxr = -3.0e38f;
    for (int p = threadIdx.x; p < n_part; p += 256) mxr = fmaxf(mxr, part_row[p]);
    return block4_allmax(mxr, s_red);
}

// The rebuild of one slice's partial.  Workgroup j of a row of gridDim.x owns slice j = the indices j * 256 + t (mod
// gridDim.x * 256); `m` is the maximum of the calling thread's elements of it (-3e38 where it has none that compare).  The slice
// maximum, then — part_idx given, with the LDS word s_idx — the lowest index that holds it through atomicMin on that word, then
// the stores to slot [blockIdx.y][blockIdx.x].  A slice that holds nothing comparable: the start value and an index the readers clamp.
__device__ __forceinline__ void slice_partial_store(const float* x, int vocab, float m, float* s_red, int* s_idx, float* __restrict__ part_val,
                                                    int* __restrict__ part_idx) {
    const int tid = threadIdx.x;
    if (part_idx != nullptr && tid == 0) *s_idx = kPickStartIdx;
    const float mx = block4_allmax(m, s_red);  // (its barrier also covers the word above)
    const size_t slot = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (part_idx == nullptr) {
        if (tid == 0) part_val[slot] = mx;
        return;
    }
    int first = kPickStartIdx;
    for (int i = blockIdx.x * 256 + tid; i < vocab; i += gridDim.x * 256)
        if (x[i] == mx) {
            first = i;
            break;
        }
    if (first != kPickStartIdx) atomicMin(s_idx, first);
    __syncthreads();
    if (tid == 0) {
        part_val[slot] = mx;
        part_idx[slot] = *s_idx;
    }
}
// the maximum of the calling thread's elements of its workgroup's slice of the row x
__device__ __forceinline__ float slice_thread_max(const float* __restrict__ x, int vocab) {
    float m = -3.0e38f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < vocab; i += gridDim.x * 256) m = fmaxf(m, x[i]);
    return m;
}
