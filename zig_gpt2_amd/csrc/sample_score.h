// sample_score.h — the log-probability of a GIVEN token at every position of a whole-prompt pass and the top-N alternatives there
// (zg_gpt_score): the statistics kernels over a block of logits rows [rows][row_stride] the lm_head GEMM just wrote
// (included by elementwise.hip behind sample_logprob.h, whose order, rounds and record buffers they share).  include/zgpt2.h
// zg_gpt_score is the contract; the definitions of logprob, top_ids and top_logprobs are §3.7's to the letter.
//
// No lm_head partials exist behind a GEMM, and a pass for the row maximum would read the block twice, so the maximum comes from
// the chunks themselves (an online softmax over chunks):
//   score_part_kernel     grid (chunks, rows): a workgroup owns kLpChunk consecutive columns of one row, four per lane, read once
//                         (lp_chunk_load).  Its own maximum m_c (never below -3e38, as lp_row_max), the sum of expf(x - m_c)
//                         (lp_chunk_sum), its best min(top_n, chunk) candidates (lp_chunk_rounds).  Only columns
//                         < vocab are read: the pad columns of the GEMM's 64-column grid never are.
//   score_finish_kernel   one workgroup per row: m = max m_c; S = sum over c in index order of s_c * expf(m_c - m), by one lane,
//                         logf once; the candidate lists merged and the column stored by lp_lists_merge_store.  Row t of sequence b predicts
//                         position past + t + 1: the target is prompt[b][past + t + 1], the column written is past + t + 1; the
//                         last row of a sequence has no target and writes nothing.
// Plain vector stores, no atomics, no fences (everything crosses a launch boundary): the same inputs give the same bits on every
// run.  Every index read from memory (target, top_n) or derived from an argument (column) is clamped before it addresses anything,
// every id is clamped below the vocabulary before it is stored.

__global__ __launch_bounds__(256) void score_part_kernel(const float* __restrict__ logits, int vocab, int row_stride, const int* __restrict__ top_n_ptr,
                                                         ScoreWs ws, int n_chunks) {
    __shared__ float s_mx[4], s_sum[4], s_v[4], s_ov[kLpTopMax];
    __shared__ int s_i[4], s_oi[kLpTopMax];
    const int tid = threadIdx.x, c = blockIdx.x, r = blockIdx.y;
    const int top_n = lp_top_n(top_n_ptr);
    float v[4];
    const unsigned taken = lp_chunk_load(logits + (size_t)r * row_stride, vocab, c, v);
    float mx = -3.0e38f;
#pragma unroll
    for (int j = 0; j < 4; ++j) mx = fmaxf(mx, v[j]);
    mx = wave_allmax(mx);
    if ((tid & 63) == 0) s_mx[tid >> 6] = mx;
    __syncthreads();
    const float m_c = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
    const size_t slot = (size_t)r * n_chunks + c;
    const float chunk_sum = lp_chunk_sum(v, taken, m_c, s_sum);
    lp_chunk_rounds(v, taken, c, top_n, s_v, s_i, s_ov, s_oi, ws.lp.val + slot * kLpTopMax, ws.lp.idx + slot * kLpTopMax);
    if (tid == 0) {
        ws.lp.sum[slot] = chunk_sum;
        ws.max[slot] = m_c;
    }
}

__global__ __launch_bounds__(256) void score_finish_kernel(const float* __restrict__ logits, int vocab, int row_stride, const int* __restrict__ top_n_ptr,
                                                           ScoreWs ws, int n_chunks, ScoreTargets tg, LogprobRec rec) {
    __shared__ float s_mx[4], s_v[4], s_sum[kLpMaxChunks], s_max[kLpMaxChunks], s_ov[kLpTopMax];
    __shared__ int s_i[4], s_oi[kLpTopMax];
    __shared__ float s_cv[kLpMaxChunks * kLpTopMax];
    __shared__ int s_ci[kLpMaxChunks * kLpTopMax];
    const int tid = threadIdx.x, r = blockIdx.x;
    const int top_n = lp_top_n(top_n_ptr);
    n_chunks = min(n_chunks, kLpMaxChunks);
    // row r of the block is row tg.row0 + r of the pass: sequence b, its t-th new position, predicting position past + t + 1
    const int n = max(tg.n, 1), row = tg.row0 + r, b = row / n, t = row - b * n;
    if (t >= n - 1) return;  // the last position of a sequence: nothing in the pass follows it
    const int pos = max(tg.past + t + 1, 0);
    const size_t out = (size_t)b * rec.stride + min(pos, rec.stride - 1);
    int tok = tg.tokens[(size_t)b * tg.token_stride + min(pos, tg.token_stride - 1)];
    tok = (unsigned)tok < (unsigned)vocab ? tok : 0;
    const float* x = logits + (size_t)r * row_stride;
    lp_lists_load(ws.lp, (size_t)r, n_chunks, top_n, s_sum, s_cv, s_ci);
    if (tid < n_chunks) s_max[tid] = ws.max[(size_t)r * n_chunks + tid];
    __syncthreads();
    float m = wave_allmax(tid < n_chunks ? s_max[tid] : -3.0e38f);
    if ((tid & 63) == 0) s_mx[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
    float log_s = 0.0f, lp_tok = 0.0f;
    if (tid == 0) {  // the chunk sums brought to the row maximum, in index order
        float total = 0.0f;
        for (int c = 0; c < n_chunks; ++c) total += s_sum[c] * expf(s_max[c] - m);
        log_s = logf(total);
        lp_tok = (x[tok] - m) - log_s;
    }
    lp_lists_merge_store(n_chunks, top_n, vocab, m, log_s, lp_tok, s_cv, s_ci, s_v, s_i, s_ov, s_oi, rec, out);
}

// The B operand of the scoring lm_head on fp32 / B24 handles: the stored values of wte [V][K] split exactly into bf16 planes,
// plane-major [3][V64][K] as the whole-prompt GEMMs read weight planes, rows V .. V64 - 1 zero.
__global__ __launch_bounds__(256) void wte_planes_kernel(const void* __restrict__ wte, int weight_type, size_t V, size_t V64, int K, bf16_t* __restrict__ out) {
    const size_t per_row = (size_t)(K / 4), n = V64 * per_row, plane = V64 * (size_t)K;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / per_row, k = (i % per_row) * 4;
        f32x4 v{0.0f, 0.0f, 0.0f, 0.0f};
        if (r < V) v = weight_type == WT_B24 ? load_b24x4(wte, r, K, (int)k) : *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(wte) + r * K + k);
        uint32_t h0, m0, l0, h1, m1, l1;
        split3_pk(v.x, v.y, h0, m0, l0);
        split3_pk(v.z, v.w, h1, m1, l1);
        bf16_t* o = out + r * K + k;
        *reinterpret_cast<u32x2*>(o) = u32x2{h0, h1};
        *reinterpret_cast<u32x2*>(o + plane) = u32x2{m0, m1};
        *reinterpret_cast<u32x2*>(o + 2 * plane) = u32x2{l0, l1};
    }
}
