// sample_score.h — the log-probability of a GIVEN token at every position of a whole-prompt pass and the top-N alternatives there
// (zg_gpt_score): the statistics kernels over a block of logits rows [rows][row_stride] the lm_head GEMM just wrote
// (included by sample.hip behind sample_logprob.h, whose order, rounds and record buffers they share).  include/zgpt2.h
// zg_gpt_score is the contract; the definitions of logprob, top_ids and top_logprobs are §3.7's to the letter.
//
// No lm_head partials exist behind a GEMM, and a pass for the row maximum would read the block twice, so the maximum comes from
// the chunks themselves (an online softmax over chunks):
//   score_part_kernel     grid (chunks, rows): a workgroup owns kLpChunk consecutive columns of one row, four per lane, read once
//                         (lp_chunk_load).  Its own maximum m_c (never below -3e38, as row_max_from_partials), the sum of expf(x - m_c)
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
    const float m_c = block4_allmax(mx, s_mx);
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
    tok = clamp_token(tok, vocab);
    const float* x = logits + (size_t)r * row_stride;
    lp_lists_load(ws.lp, (size_t)r, n_chunks, top_n, s_sum, s_cv, s_ci);
    if (tid < n_chunks) s_max[tid] = ws.max[(size_t)r * n_chunks + tid];
    __syncthreads();
    const float m = block4_allmax(tid < n_chunks ? s_max[tid] : -3.0e38f, s_mx);
    float log_s = 0.0f, lp_tok = 0.0f;
    if (tid == 0) {  // the chunk sums brought to the row maximum, in index order
        float total = 0.0f;
        for (int c = 0; c < n_chunks; ++c) total += s_sum[c] * expf(s_max[c] - m);
        log_s = logf(total);
        lp_tok = (x[tok] - m) - log_s;
    }
    lp_lists_merge_store(n_chunks, top_n, vocab, m, log_s, lp_tok, s_cv, s_ci, s_v, s_i, s_ov, s_oi, rec, out);
}
