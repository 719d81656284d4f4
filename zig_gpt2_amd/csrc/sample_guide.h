// sample_guide.h — guided decoding: a token-level automaton per row, as the last of the stages that rewrite the logit row and one
// small stage behind the sampler: the kernels (included by sample.hip behind sample_edit.h, inside its unnamed namespace).
// include/zgpt2.h zg_guide is the contract.
//
// A row b stands in state[b] of the table next [n_states][vocab] (uint16; kGuideDead: not allowed).  For a picked column
//   y[i] = next[state[b]][i] != dead ? x[i] : -inf,   and behind the pick   state[b] = next[state[b]][pick].
// The mask does not read `next`: the host built one keep bitmap per state from it (keep [n_states][words]), and the state only
// chooses which one the row's workgroups read — a word per 32 elements, shared by the 32 lanes that need it.
//   guide_mask_kernel     logit_edit_kernel's twin, grid (n_part, batch), the same slices and the same single-writer rule: the
//                         keep word of an index is the state's, ANDed with the call's own keep set when the call has edits (tab
//                         and keep given); a row without a guide takes all-ones in the state's place.  The bias walk tests the
//                         combined bit.  The slice maximum (lowest index on ties) goes to part_val / part_idx, so a tail with
//                         edits and a guide has ONE launch for both, and the partials are rebuilt once.  A row that has neither
//                         a guide nor edits is read, never written: it keeps its bits (NaN payloads, -0.0) beside guided rows.
//   guide_advance_kernel  one workgroup, one lane per row: writes the state record of the column in flight, then follows the
//                         transition of the sampler's pick.  2-byte loads (rows of `next` are vocab uint16 apart and a vocabulary
//                         may be odd: nothing wider is aligned), plain stores, no atomics, nothing waited for.  The position is
//                         read from device memory, so inside a multi-step graph the kernel simply repeats.
// A row is guided at the column in flight iff its state is in [0, *n_states) and the column is a picked one (ctrl->seq_len - 1 >=
// prompt_len[b]; without ctrl: always).  A prompt column is neither masked nor advanced.  State, token and *n_states come from
// device memory and are clamped (state < n_states <= kGuideMaxStates, token < vocab) before they address anything; a transition
// that is dead or out of range — possible only for a pick from a row holding NaN — leaves the state where it is.

// the state row b is masked by and advanced from at the column in flight, or -1
__device__ __forceinline__ int guide_row_state(const GuideArgs& g, int b) {
    const int n = min(max(*g.n_states, 0), kGuideMaxStates);
    const int st = g.state[b];
    const bool picked = g.ctrl == nullptr || g.ctrl->seq_len - 1 >= g.prompt_len[b];
    return (picked && (unsigned)st < (unsigned)n) ? st : -1;
}

__global__ __launch_bounds__(256) void guide_mask_kernel(float* __restrict__ logits, int vocab, const EditTable* __restrict__ tab,
                                                         const unsigned* __restrict__ keep, const GuideArgs g, float* __restrict__ part_val,
                                                         int* __restrict__ part_idx) {
    __shared__ float s_red[4];
    __shared__ int s_idx;
    const int tid = threadIdx.x, b = blockIdx.y;
    const int stride = gridDim.x * 256;
    float* x = logits + (size_t)b * vocab;
    const int st = guide_row_state(g, b);  // (uniform over the workgroup, which serves one row)
    const unsigned* gk = st >= 0 ? g.keep + (size_t)st * ((vocab + 31) >> 5) : nullptr;
    auto kept = [&](unsigned i) {
        unsigned w = gk ? gk[i >> 5] : ~0u;
        if (keep) w &= keep[i >> 5];
        return ((w >> (i & 31u)) & 1u) != 0u;
    };
    if (tab) {  // logit_edit_kernel's table walk, on the combined bit
        const int n_bias = min(max(tab->n_bias, 0), kEditMaxBias);
        for (int p = tid; p < n_bias; p += 256) {
            const unsigned id = (unsigned)tab->ids[p];
            if (id >= (unsigned)vocab) continue;
            if ((int)((id >> 8) % gridDim.x) != (int)blockIdx.x) continue;  // another workgroup's slice
            if (!kept(id)) continue;                                        // a bias on a dropped token: the slice loop writes -inf
            x[id] = x[id] + tab->vals[p];
        }
    }
    __syncthreads();  // (workgroup scope: the rewritten logits are visible to the slice loop's loads)
    float m = -3.0e38f;
    if (gk == nullptr && keep == nullptr) m = slice_thread_max(x, vocab);  // no guide, no edits: the row is only read
    else
        for (int i = blockIdx.x * 256 + tid; i < vocab; i += stride) {
            if (kept((unsigned)i)) m = fmaxf(m, x[i]);
            else x[i] = -INFINITY;
        }
    slice_partial_store(x, vocab, m, s_red, &s_idx, part_val, part_idx);
}

__global__ __launch_bounds__(64) void guide_advance_kernel(const GuideArgs g, const int* __restrict__ picks, int batch, int vocab) {
    const int b = threadIdx.x;
    if (b >= batch) return;
    const int st = guide_row_state(g, b);
    if (st < 0) return;  // a prompt column, or a row without a guide: its record keeps the "none" the host put there
    const int n = min(max(*g.n_states, 0), kGuideMaxStates);
    const int col = g.ctrl ? g.ctrl->seq_len - 1 : 0;
    if (g.rec != nullptr && (unsigned)col < (unsigned)g.rec_stride) g.rec[(size_t)b * g.rec_stride + col] = st;
    const unsigned tok = (unsigned)picks[b];
    if (tok >= (unsigned)vocab) return;
    const unsigned nx = g.next[(size_t)st * vocab + tok];
    if (nx < (unsigned)n) g.state[b] = (int)nx;
}
