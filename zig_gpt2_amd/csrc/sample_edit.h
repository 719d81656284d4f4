// sample_edit.h — logit bias and token allow / ban lists on the logit row, between the penalty stage and the sampler: the kernel
// (included by sample.hip behind sample_penalty.h, inside its unnamed namespace).  include/zgpt2.h zg_logit_edits is the contract.
//
// For one row x[0..V): keep[i] = bit i of the keep set the host built from the two lists (bit set: allowed and not banned);
// y[i] = keep[i] ? (i biased ? x[i] + v : x[i]) : -inf.  The sum is one rounded fp32 add; a kept, unbiased index is not written.
//   logit_edit_kernel   grid (n_part, batch): workgroup j of a row owns slice j = the indices j * 256 + t (mod n_part * 256) — the
//                       slices of row_argmax_partials_kernel — edits exactly that slice and reports its maximum (lowest index on
//                       ties) into part_val / part_idx, so the partials the samplers, zg_gpt_argmax and the log-probability stage
//                       start from are those of the edited row without a second launch.
// Bias: the workgroup walks the (id, value) table (<= kEditMaxBias pairs, distinct ids) and the thread that meets a pair of its own
// slice whose id is kept rewrites that logit; behind a barrier the slice loop writes -inf where the keep bit is clear.  An index is
// therefore written by at most one thread: a kept biased one by the table walk, a dropped one by the slice loop.  Ids and the count
// are read from device memory (one captured launch serves every set) and bounds-checked before they become an address.
// The keep set costs one word per 32 elements; the 32 lanes that share a word read the same address.
// A slice left without a comparable value (all -inf): the start value and an index the readers clamp, as row_argmax_partials_kernel.

__global__ __launch_bounds__(256) void logit_edit_kernel(float* __restrict__ logits, int vocab, const EditTable* __restrict__ tab,
                                                         const unsigned* __restrict__ keep, float* __restrict__ part_val, int* __restrict__ part_idx) {
    __shared__ float s_red[4];
    __shared__ int s_idx;
    const int tid = threadIdx.x, b = blockIdx.y;
    const int stride = gridDim.x * 256;
    float* x = logits + (size_t)b * vocab;
    const int n_bias = min(max(tab->n_bias, 0), kEditMaxBias);
    for (int p = tid; p < n_bias; p += 256) {
        const unsigned id = (unsigned)tab->ids[p];
        if (id >= (unsigned)vocab) continue;
        if ((int)((id >> 8) % gridDim.x) != (int)blockIdx.x) continue;  // another workgroup's slice
        if (!((keep[id >> 5] >> (id & 31u)) & 1u)) continue;            // a bias on a dropped token: the slice loop writes -inf
        x[id] = x[id] + tab->vals[p];
    }
    __syncthreads();  // (workgroup scope: the rewritten logits are visible to the slice loop's loads)
    float m = -3.0e38f;
    for (int i = blockIdx.x * 256 + tid; i < vocab; i += stride) {
        if ((keep[i >> 5] >> (i & 31)) & 1u) m = fmaxf(m, x[i]);
        else x[i] = -INFINITY;
    }
    // (the index search reads the slice again: a dropped index holds -inf, which this thread wrote itself; the slice maximum is
    // never below the start value)
    slice_partial_store(x, vocab, m, s_red, &s_idx, part_val, part_idx);
}
