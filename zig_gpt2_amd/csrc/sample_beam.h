// sample_beam.h — beam search in the device loop, as the stage behind the log-probability stage of a greedy step: the kernel
// (included by sample.hip behind sample_stop.h, inside its unnamed namespace).  include/zgpt2.h zg_beam_options is the contract;
// tests/beam_ref.py restates this text in numpy float32.
//
// The rows of a handle are G = batch / W groups of W slots; group g owns slots g W .. g W + W - 1 and one wave of the one workgroup.
// The step in flight picks column col = ctrl->seq_len - 1.  Its lists — the top 2 W (token, log-probability) pairs the
// log-probability stage has just recorded in column col — are indexed by the slot as it stood BEFORE the step, which is the
// parent's slot; the token, parent and score this kernel records in column col are indexed by the slot AFTER it.
//
// A group that is not done:
//   1. candidates (score[s] + list[s][j], s, j) over its live slots and j < 2 W: one rounded fp32 add.  At column c0 only the group's
//      first slot is live; from then on all are.  Order: value descending, slot ascending, j ascending; NaN below every number
//      (beam_key), -0.0 equal to +0.0.  The first 2 W are kept: 2 W rounds of a wave maximum over one 64-bit key per candidate.
//   2. lane 0 walks them in rank order r.  A candidate whose token is eos is offered to the group's pool of finished hypotheses
//      if r < W and dropped otherwise; its normalised score is value / lenpow[col - c0 + 1], one correctly rounded division.  Any
//      other candidate is the next beam until W are taken.
//   3. the pool holds at most W entries (sum, norm, parent slot, column).  A full pool takes an offer only if its norm is strictly
//      greater (by beam_key) than the WORST entry's, in that entry's place.  THE TIE RULE: the worst entry is the one of lowest
//      norm and, among equal norms, the one at the highest index of the pool.
//   4. slots, in rank order: a beam keeps its parent's slot unless an earlier beam took it; the beams left over then take the free
//      slots in ascending order.  So the parent of a beam that moves is always a slot that keeps its own beam: the table `src`
//      this kernel leaves for the cache fork behind it has src[src[s]] == src[s].
//   5. the group is done — after the walk — when its pool is full and (early stopping, or worst norm >= best new beam's value /
//      lenpow[col - c0 + 1]).  The beams of that step are still recorded.
// A slot no beam was found for (fewer than W candidates that are not eos: lists with repeated tokens only) keeps itself: parent
// itself, its list's first token, score -inf.  The slots of a done group do the same with their score unchanged, every step:
// nothing of theirs is read afterwards.  Last, thread 0 tells the host what the stop stage tells it: done_col = the highest done
// column + 1 once every group is done, then progress = col + 1.  Every index read from memory is clamped before it becomes an address.

__device__ __forceinline__ unsigned beam_key(float v) {
    if (v != v) return 0u;
    if (v == 0.0f) return 0x80000000u;
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// index of the worst of n >= 1 pool entries (THE TIE RULE above)
__device__ __forceinline__ int beam_pool_worst(const float* norm, int n) {
    int w = 0;
    for (int k = 1; k < n; ++k)
        if (beam_key(norm[k]) <= beam_key(norm[w])) w = k;
    return w;
}

__global__ __launch_bounds__(64 * kBeamRows) void beam_step_kernel(const BeamArgs a) {
    __shared__ int s_ck[kBeamRows][2 * kBeamMax];  // the kept candidates of a group, in rank order (-1: none)
    __shared__ float s_bv[kBeamRows][kBeamMax];    // the new beams of a group, in rank order: value, parent's local slot, list entry, token
    __shared__ int s_bs[kBeamRows][kBeamMax], s_bj[kBeamRows][kBeamMax], s_bt[kBeamRows][kBeamMax];
    __shared__ int s_done[kBeamRows];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    BeamState* const st = a.st;
    const int W = min(max(st->W, 1), min(kBeamMax, a.batch));
    const int G = a.batch / W;
    const int col = min(max(a.col >= 0 ? a.col : a.ctrl->seq_len - 1, 0), a.stride - 1);
    const int c0 = st->c0, eos = st->eos;
    const float lp = a.lenpow[min(max(col - c0 + 1, 0), a.n_lenpow - 1)];
    auto at = [&](int s, int j) { return ((size_t)s * a.stride + col) * kLpTopMax + j; };
    if (g < G) {
        const int s0 = g * W;
        int done = st->done_col[g];
        if (done >= 0) {  // (uniform over the wave)
            if (lane < W) {
                const int s = s0 + lane;
                a.sampled[s] = clamp_token(a.top_ids[at(s, 0)], a.vocab);
                a.parent[(size_t)s * a.stride + col] = s;
                a.score[(size_t)s * a.stride + col] = st->score[s];
                a.logprob[(size_t)s * a.stride + col] = a.top_logprobs[at(s, 0)];
                st->src[s] = s;
            }
        } else {
            // 1. one key per candidate: the value's order in the upper word, the complement of k = slot * 2 W + j in the lower
            unsigned long long key[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int k = lane + 64 * i, sl = k / (2 * W), j = k - sl * 2 * W;
                key[i] = 0ull;
                if (sl < W && (col > c0 || sl == 0)) {
                    const float v = st->score[s0 + sl] + a.top_logprobs[at(s0 + sl, j)];
                    key[i] = ((unsigned long long)beam_key(v) << 32) | (unsigned long long)(0xffffffffu - (unsigned)k);
                }
            }
            for (int r = 0; r < 2 * W; ++r) {
                unsigned long long best = key[0] > key[1] ? key[0] : key[1];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    const unsigned long long o = __shfl_xor(best, off, 64);
                    best = o > best ? o : best;
                }
                if (best != 0ull && key[0] == best) key[0] = 0ull;
                if (best != 0ull && key[1] == best) key[1] = 0ull;
                if (lane == 0) s_ck[g][r] = best != 0ull ? (int)(0xffffffffu - (unsigned)best) : -1;
            }
            if (lane == 0) {
                // 2. the walk
                int nb = 0;
                for (int r = 0; r < 2 * W; ++r) {
                    const int k = s_ck[g][r];
                    if (k < 0) continue;
                    const int sl = k / (2 * W), j = k - sl * 2 * W;
                    const float v = st->score[s0 + sl] + a.top_logprobs[at(s0 + sl, j)];
                    const int tok = clamp_token(a.top_ids[at(s0 + sl, j)], a.vocab);
                    if (eos >= 0 && tok == eos) {
                        if (r < W) {  // 3. the offer
                            const float norm = __fdiv_rn(v, lp);
                            int n = min(max(st->pool_n[g], 0), W), idx = -1;
                            if (n < W) {
                                idx = n;
                                st->pool_n[g] = n + 1;
                            } else {
                                const int w = beam_pool_worst(st->pool_norm + s0, n);
                                if (beam_key(norm) > beam_key(st->pool_norm[s0 + w])) idx = w;
                            }
                            if (idx >= 0) {
                                st->pool_sum[s0 + idx] = v;
                                st->pool_norm[s0 + idx] = norm;
                                st->pool_parent[s0 + idx] = s0 + sl;
                                st->pool_col[s0 + idx] = col;
                            }
                        }
                        continue;
                    }
                    if (nb < W) {
                        s_bv[g][nb] = v;
                        s_bs[g][nb] = sl;
                        s_bj[g][nb] = j;
                        s_bt[g][nb] = tok;
                        ++nb;
                    }
                }
                // 5. the done test (on the pool as the walk left it and the best new beam), before the scores are overwritten
                const int n = min(max(st->pool_n[g], 0), W);
                if (n >= W) {
                    const float worst = st->pool_norm[s0 + beam_pool_worst(st->pool_norm + s0, n)];
                    if (st->early != 0 || worst >= __fdiv_rn(nb > 0 ? s_bv[g][0] : -INFINITY, lp)) done = col;
                }
                // 4. slots
                unsigned taken = 0u;
                int slot[kBeamMax];
#pragma unroll
                for (int i = 0; i < kBeamMax; ++i) {
                    slot[i] = -1;
                    if (i < nb && !((taken >> s_bs[g][i]) & 1u)) {
                        slot[i] = s_bs[g][i];
                        taken |= 1u << slot[i];
                    }
                }
#pragma unroll
                for (int i = 0; i < kBeamMax; ++i)
                    if (i < nb && slot[i] < 0) {
                        slot[i] = __ffs((int)~taken) - 1;  // (nb <= W: a slot below W is free)
                        taken |= 1u << slot[i];
                    }
#pragma unroll
                for (int i = 0; i < kBeamMax; ++i)
                    if (i < nb) {
                        const int t = s0 + slot[i], p = s0 + s_bs[g][i];
                        a.sampled[t] = s_bt[g][i];
                        a.parent[(size_t)t * a.stride + col] = p;
                        a.score[(size_t)t * a.stride + col] = s_bv[g][i];
                        a.logprob[(size_t)t * a.stride + col] = a.top_logprobs[at(p, s_bj[g][i])];
                        st->src[t] = p;
                        st->score[t] = s_bv[g][i];  // (every candidate's sum was formed above: the old scores are dead)
                    }
                for (int t = 0; t < W; ++t)
                    if (!((taken >> t) & 1u)) {  // no beam was found for this slot: it keeps itself
                        const int s = s0 + t;
                        a.sampled[s] = clamp_token(a.top_ids[at(s, 0)], a.vocab);
                        a.parent[(size_t)s * a.stride + col] = s;
                        a.score[(size_t)s * a.stride + col] = -INFINITY;
                        a.logprob[(size_t)s * a.stride + col] = a.top_logprobs[at(s, 0)];
                        st->src[s] = s;
                        st->score[s] = -INFINITY;
                    }
                if (done >= 0) st->done_col[g] = done;
            }
        }
        if (lane == 0) s_done[g] = done;
    }
    __syncthreads();
    if (threadIdx.x == 0 && a.host) {
        int hi = 0;
        bool all = true;
        for (int k = 0; k < G; ++k) {
            all = all && s_done[k] >= 0;
            hi = max(hi, s_done[k]);
        }
        if (all) __hip_atomic_store(&a.host->done_col, (unsigned)(hi + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&a.host->progress, (unsigned)(col + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
