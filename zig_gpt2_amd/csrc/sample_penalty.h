// sample_penalty.h — repetition / presence / frequency penalties on the raw logits, in front of the sampler: the kernels (included
// by sample.hip behind sample_filter.h, inside its unnamed namespace).  include/zgpt2.h zg_logit_penalties is the contract.
//
// For one row x[0..V) and its history (token ids, any order, duplicates allowed): c[i] = occurrences of i in the history;
// c == 0 leaves x[i] alone, c >= 1 gives ((x > 0 ? x / r : x * r) - (presence + frequency * c)), every operation rounded on its
// own — once per DISTINCT token however often it occurs (HF's gather / scatter).
//   penalty_apply_kernel     one workgroup per row.  The distinct tokens and their counts are found in an open-addressed LDS table
//                            of 2 x max_hist slots (a power of two): atomicCAS claims a key, atomicAdd counts, linear probing
//                            bounded by the table size.  Counts are integers: nothing depends on the order of arrival.  Behind a
//                            barrier one thread per occupied slot reads its logit and rewrites it: one writer per index.
//   row_argmax_partials_kernel   lm_head's argmax epilogue left the maxima of the UNPENALISED row in part_val / part_idx, and both
//                            samplers take the row maximum from there without a pass over the logits: they are rebuilt from the
//                            penalised row, n_part slices per row (slice j = the indices j * 256 + t (mod n_part * 256)).
// A token >= vocab is skipped (a corrupted record never becomes an address); lengths read from device memory are clamped to the
// strides and to max_hist, so the table always has a free slot.  The filter workspace is not touched.
// The values are the row's own (params[b]): a row whose penalties are off is counted like any other and never written
// back — it keeps its bits, a NaN's payload and a -0.0 included, beside neighbours that are penalised.

constexpr unsigned kPenEmpty = 0xffffffffu;

__device__ __forceinline__ float penalized_logit(float x, float r, float presence, float frequency, unsigned count) {
#pragma clang fp contract(off)
    const float y = x > 0.0f ? x / r : x * r;  // -0.0, +0.0, negative values and NaN take the product
    const float fc = frequency * (float)count;
    const float off = presence + fc;
    return y - off;
}

__global__ __launch_bounds__(256) void penalty_apply_kernel(float* __restrict__ logits, int vocab, const PenParams* __restrict__ params, PenHistory h,
                                                            int slots, unsigned* __restrict__ counts_out) {
    extern __shared__ unsigned pen_lds[];  // keys[slots] | counts[slots]
    unsigned* keys = pen_lds;
    unsigned* cnt = pen_lds + slots;
    const int tid = threadIdx.x, b = blockIdx.x;
    for (int i = tid; i < slots; i += 256) {
        keys[i] = kPenEmpty;
        cnt[i] = 0u;
    }
    const int cap = min(h.max_hist, slots >> 1);
    const int n_prior = h.prior ? min(max(h.prior_len[b], 0), min(h.prior_stride, cap)) : 0;
    int past = 0, n_rec = 0;
    if (h.ctrl && h.rec) {  // the loop's record of this row: positions past .. step - 2 (the step in flight is step - 1)
        past = min(max(params[b].past_len, 0), h.rec_stride);
        n_rec = min(max(h.ctrl->step - 1 - past, 0), min(h.rec_stride - past, cap - n_prior));
    }
    __syncthreads();
    const unsigned mask = (unsigned)slots - 1u;
    for (int i = tid; i < n_prior + n_rec; i += 256) {
        const int tok = i < n_prior ? h.prior[(size_t)b * h.prior_stride + i] : h.rec[(size_t)b * h.rec_stride + past + (i - n_prior)];
        if ((unsigned)tok >= (unsigned)vocab) continue;
        unsigned s = (((unsigned)tok * 2654435761u) >> 16) & mask;
        for (int probe = 0; probe < slots; ++probe) {
            const unsigned old = atomicCAS(&keys[s], kPenEmpty, (unsigned)tok);
            if (old == kPenEmpty || old == (unsigned)tok) {
                atomicAdd(&cnt[s], 1u);
                break;
            }
            s = (s + 1u) & mask;
        }
    }
    __syncthreads();
    const float r = params[b].repetition, presence = params[b].presence, frequency = params[b].frequency;
    const bool off = r == 1.0f && presence == 0.0f && frequency == 0.0f;  // (uniform over the workgroup)
    float* x = logits + (size_t)b * vocab;
    for (int i = tid; i < slots; i += 256) {
        const unsigned tok = keys[i];
        if (tok >= (unsigned)vocab) continue;  // empty
        const unsigned c = cnt[i];
        if (!off) x[tok] = penalized_logit(x[tok], r, presence, frequency, c);
        if (counts_out) counts_out[(size_t)b * vocab + tok] = c;
    }
}

// row_max_partials_kernel with the index beside the maximum (sample_common.h slice_partial_store: the lowest one on ties)
__global__ __launch_bounds__(256) void row_argmax_partials_kernel(const float* __restrict__ logits, int vocab, float* __restrict__ part_val,
                                                                  int* __restrict__ part_idx) {
    __shared__ float s_red[4];
    __shared__ int s_idx;
    const float* x = logits + (size_t)blockIdx.y * vocab;
    slice_partial_store(x, vocab, slice_thread_max(x, vocab), s_red, &s_idx, part_val, part_idx);
}
