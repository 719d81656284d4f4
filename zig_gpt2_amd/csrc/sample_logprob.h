// sample_logprob.h — the log-probability of the token a decode step picks and the top-N alternatives of its row, as one more
// optional stage behind the sampler: the kernels (included by sample.hip behind sample_edit.h, inside its unnamed
// namespace).  include/zgpt2.h zg_gpt_generate_logprobs_enqueue is the contract.
//
// For one row x[0..V) as the sampler stage receives it (raw, or as the penalties leave it; temperature 1, nothing truncated),
// m = max x and S = sum exp(x - m):  logprob(i) = (x[i] - m) - log S;  the top-N are the N largest x, value descending, index
// ascending on ties (-0.0 == +0.0, -inf an ordinary value), found by comparisons only.
//   logprob_part_kernel     grid (chunks, batch): a workgroup owns kLpChunk consecutive elements, four per lane.  m comes from
//                           lm_head's argmax partials (no pass over the row).  The chunk's sum: four terms per lane in index order,
//                           the wave's DPP tree, the four waves in order.  Its best min(top_n, chunk) (value, index) pairs: top_n
//                           rounds of a workgroup argmax over what is not yet taken (DPP inside the wave, LDS across the waves).
//   logprob_finish_kernel   one workgroup per row: the chunk sums added in index order, the chunks' candidate lists — each already
//                           in order — merged by top_n more argmax rounds over the lists' heads (LDS), the token the step records
//                           (the sampler's draw, or the lowest-index argmax of the partials as embed_step_kernel takes it one step
//                           later), and one column of the record buffers written behind the last round.
// sample_score.h's two kernels are these two with another source of m: what all four share — the chunk a workgroup loads, its sum,
// the selection rounds, the merge of the lists and the store of the record column — is written once, below (lp_chunk_*, lp_lists_*).
// Nothing is accumulated atomically and no order depends on arrival: the same inputs give the same bits on every run.  A NaN never
// wins a comparison, so a row holding one may list fewer than top_n real candidates: every index is clamped below the vocabulary
// before it is stored or followed.  Every index read from memory (column, token, top_n) is clamped before it becomes an address.

constexpr int kLpChunk = 1024;      // elements of a row per workgroup of logprob_part_kernel
constexpr int kLpMaxChunks = 256;   // vocab <= 262144, as the samplers
constexpr int kLpTopMax = 20;       // ZG_LOGPROBS_TOP_MAX: the candidate lists and the record buffers have this many slots
constexpr int kLpNone = 0x7fffffff; // the index of "nothing left": loses every tie, also against a real -inf

// (value, index) first under pick_before over a workgroup of four waves; every lane receives it: wave_first, then the four waves
// through the LDS.
__device__ __forceinline__ void lp_block_first(float& bv, int& bi, float* s_v, int* s_i) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wave_first(bv, bi);
    __syncthreads();  // (the previous round's readers are done)
    if (lane == 0) {
        s_v[wave] = bv;
        s_i[wave] = bi;
    }
    __syncthreads();
    bv = s_v[0];
    bi = s_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (pick_before(s_v[w], s_i[w], bv, bi)) { bv = s_v[w]; bi = s_i[w]; }
}

__device__ __forceinline__ int lp_top_n(const int* top_n) { return min(max(*top_n, 0), kLpTopMax); }

// The chunk of workgroup c of a row x: kLpChunk consecutive columns, four per lane (column c * kLpChunk + j * 256 + tid in v[j]).
// Returns the mask of the lane's columns at or beyond vocab: never read (-inf), out of the sum and taken before the first round.
__device__ __forceinline__ unsigned lp_chunk_load(const float* __restrict__ x, int vocab, int c, float (&v)[4]) {
    unsigned taken = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = c * kLpChunk + j * 256 + threadIdx.x;
        v[j] = i < vocab ? x[i] : -INFINITY;
        if (i >= vocab) taken |= 1u << j;
    }
    return taken;
}

// sum of expf(v - m) over the chunk: four terms per lane in index order, the wave's DPP tree, the four waves in order
__device__ __forceinline__ float lp_chunk_sum(const float (&v)[4], unsigned taken, float m, float* s_sum) {
    float e = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) e += (taken >> j) & 1u ? 0.0f : expf(v[j] - m);
    e = wave_allsum(e);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = e;
    __syncthreads();
    return (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
}

// The chunk's best min(top_n, chunk) (value, index) pairs into val / idx [kLpTopMax], in order: top_n rounds of a workgroup argmax
// over what is not yet taken.  The rounds keep their winners in the LDS; the list is stored behind the last one, a lane per entry.
__device__ __forceinline__ void lp_chunk_rounds(const float (&v)[4], unsigned taken, int c, int top_n, float* s_v, int* s_i, float* s_ov, int* s_oi,
                                                float* __restrict__ val, int* __restrict__ idx) {
    const int tid = threadIdx.x;
    for (int r = 0; r < top_n; ++r) {
        float bv = -INFINITY;
        int bi = kLpNone;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = c * kLpChunk + j * 256 + tid;
            if (!((taken >> j) & 1u) && pick_before(v[j], i, bv, bi)) { bv = v[j]; bi = i; }
        }
        lp_block_first(bv, bi, s_v, s_i);
        if (tid == 0) {
            s_ov[r] = bv;
            s_oi[r] = bi;
        }
        const int loc = bi - c * kLpChunk;  // (kLpNone: no lane's)
        if (bi != kLpNone && (loc & 255) == tid) taken |= 1u << ((loc >> 8) & 3);
    }
    __syncthreads();
    if (tid < top_n) {
        val[tid] = s_ov[tid];
        idx[tid] = s_oi[tid];
    }
}

// The chunk sums and candidate lists of row `row` of the workspace into the LDS (the caller's barrier follows)
__device__ __forceinline__ void lp_lists_load(const LogprobWs& ws, size_t row, int n_chunks, int top_n, float* s_sum, float* s_cv, int* s_ci) {
    const int tid = threadIdx.x;
    if (tid < n_chunks) s_sum[tid] = ws.sum[row * n_chunks + tid];
    for (int k = tid; k < n_chunks * top_n; k += 256) {
        const int c = k / top_n, j = k - c * top_n;
        s_cv[c * kLpTopMax + j] = ws.val[(row * n_chunks + c) * kLpTopMax + j];
        s_ci[c * kLpTopMax + j] = ws.idx[(row * n_chunks + c) * kLpTopMax + j];
    }
}

// The merge of the lists and column `out` of the record: the lists are in order and the chunks are index ranges, so the next of
// the row is always the first of the lists' heads — top_n more argmax rounds, a lane per list.  m, log_s and lp_tok are lane 0's.
__device__ __forceinline__ void lp_lists_merge_store(int n_chunks, int top_n, int vocab, float m, float log_s, float lp_tok, const float* s_cv, const int* s_ci,
                                                     float* s_v, int* s_i, float* s_ov, int* s_oi, const LogprobRec& rec, size_t out) {
    const int tid = threadIdx.x;
    int pos = 0;
    const bool mine = tid < n_chunks && top_n > 0;
    float hv = mine ? s_cv[tid * kLpTopMax] : -INFINITY;
    int hi = mine ? s_ci[tid * kLpTopMax] : kLpNone;
    for (int r = 0; r < top_n; ++r) {
        float bv = hv;
        int bi = hi;
        lp_block_first(bv, bi, s_v, s_i);
        if (tid == 0) {  // (kept in the LDS until the rounds are over, as in the part kernels)
            s_oi[r] = clamp_token(bi, vocab);
            s_ov[r] = (bv - m) - log_s;
        }
        if (mine && bi != kLpNone && hi == bi) {  // the winner's list moves on
            ++pos;
            hv = pos < top_n ? s_cv[tid * kLpTopMax + pos] : -INFINITY;
            hi = pos < top_n ? s_ci[tid * kLpTopMax + pos] : kLpNone;
        }
    }
    __syncthreads();
    if (tid == 0) rec.logprob[out] = lp_tok;
    if (tid < top_n) {
        rec.top_ids[out * kLpTopMax + tid] = s_oi[tid];
        rec.top_logprobs[out * kLpTopMax + tid] = s_ov[tid];
    }
}

__global__ __launch_bounds__(256) void logprob_part_kernel(const float* __restrict__ logits, int vocab, const float* __restrict__ part_val, int n_part,
                                                           int part_stride, const int* __restrict__ top_n_ptr, LogprobWs ws, int n_chunks) {
    __shared__ float s_mx[4], s_sum[4], s_v[4], s_ov[kLpTopMax];
    __shared__ int s_i[4], s_oi[kLpTopMax];
    const int c = blockIdx.x, b = blockIdx.y;
    const int top_n = lp_top_n(top_n_ptr);
    const float m = row_max_from_partials(part_val + (size_t)b * part_stride, n_part, s_mx);
    float v[4];
    const unsigned taken = lp_chunk_load(logits + (size_t)b * vocab, vocab, c, v);
    const size_t slot = (size_t)b * n_chunks + c;
    const float chunk_sum = lp_chunk_sum(v, taken, m, s_sum);
    lp_chunk_rounds(v, taken, c, top_n, s_v, s_i, s_ov, s_oi, ws.val + slot * kLpTopMax, ws.idx + slot * kLpTopMax);
    if (threadIdx.x == 0) ws.sum[slot] = chunk_sum;
}

__global__ __launch_bounds__(256) void logprob_finish_kernel(const float* __restrict__ logits, int vocab, const float* __restrict__ part_val,
                                                             const int* __restrict__ part_idx, int n_part, int part_stride,
                                                             const int* __restrict__ top_n_ptr, LogprobWs ws, int n_chunks,
                                                             const int* __restrict__ tokens, const StepCtrl* ctrl,
                                                             const int* __restrict__ prompt_len, LogprobRec rec) {
    __shared__ float s_mx[4], s_v[4], s_sum[kLpMaxChunks], s_ov[kLpTopMax];
    __shared__ int s_i[4], s_oi[kLpTopMax];
    __shared__ float s_cv[kLpMaxChunks * kLpTopMax];
    __shared__ int s_ci[kLpMaxChunks * kLpTopMax];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int top_n = lp_top_n(top_n_ptr);
    n_chunks = min(n_chunks, kLpMaxChunks);
    // the column this step's pick is recorded in: the position it was computed at
    const int col = ctrl ? min(max(ctrl->seq_len - 1, 0), rec.stride - 1) : 0;
    const size_t out = (size_t)b * rec.stride + col;
    if (prompt_len && col < prompt_len[b]) {  // the column records a prompt token: nothing was picked
        if (tid == 0) rec.logprob[out] = __uint_as_float(0x7fc00000u);
        return;
    }
    const float* x = logits + (size_t)b * vocab;
    const float m = row_max_from_partials(part_val + (size_t)b * part_stride, n_part, s_mx);
    // the token the step records — thread 0 alone follows it, so wave 0 alone finds it.  Greedy: partials_first, the very pick
    // embed_step_kernel makes of these partials one step later
    int tok = 0;
    if (tid < 64)
        tok = clamp_token(tokens ? tokens[b] : partials_first(part_val + (size_t)b * part_stride, part_idx + (size_t)b * part_stride, n_part), vocab);
    lp_lists_load(ws, (size_t)b, n_chunks, top_n, s_sum, s_cv, s_ci);
    __syncthreads();
    float log_s = 0.0f, lp_tok = 0.0f;
    if (tid == 0) {  // the chunk sums in index order
        float total = 0.0f;
        for (int c = 0; c < n_chunks; ++c) total += s_sum[c];
        log_s = logf(total);
        lp_tok = (x[tok] - m) - log_s;
    }
    lp_lists_merge_store(n_chunks, top_n, vocab, m, log_s, lp_tok, s_cv, s_ci, s_v, s_i, s_ov, s_oi, rec, out);
}
