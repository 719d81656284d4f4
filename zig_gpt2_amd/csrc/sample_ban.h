// sample_ban.h — history-dependent token bans, between the penalties and the edits: the kernel (included by sample.hip behind
// sample_penalty.h, inside its unnamed namespace).  include/zgpt2.h zg_ban_rules is the contract.
//
// For one row x[0..V), its history h[0..L) (token ids IN ORDER: the prior, then the loop's record from rules->past_len on) and
// picked = (column in flight) - prompt_len[b]:
//   n-gram, n = rules->ngram[b]   every window h[i .. i+n-1), i in 0 .. L-n, that equals the suffix h[L-n+1 .. L) bans h[i+n-1];
//                                 n == 1 compares nothing and bans every token of the history
//   words                         word w of m tokens bans w[m-1] when L >= m-1 and the suffix h[L-m+1 .. L) equals w[0 .. m-1)
//   suppress                      while 0 <= picked < rules->min_tokens[b], every id of rules->suppress
// A ban is a store of -inf to x[tok]: many threads may store the same value to one index, no thread reads the row, nothing is
// waited for.
//   ban_apply_kernel   one workgroup of 256 threads per row.  The history goes into the LDS (one int per token, at most max_hist
//                      <= kPenMaxHistory: 32 KB); behind a barrier the windows are strided over the threads — consecutive lanes
//                      read consecutive LDS words, and the suffix word they compare against is one address for all lanes (a
//                      broadcast) —, then one thread per word walks its word, then one thread per suppress id.
// Everything read from device memory is clamped before it sizes a loop or becomes an address: n to 0 .. kBanMaxNgram, the counts to
// their tables, a word length to 1 .. kBanMaxWordLen (0: the word is skipped), the history lengths to the strides and to max_hist
// exactly as penalty_apply_kernel clamps them; a token >= vocab in the history equals nothing and is never stored to, and a word or
// suppress id >= vocab is skipped.  A row whose rules are all off at this column returns before the first load of its history and
// is never written: it keeps its bits, a NaN's payload and a -0.0 included, beside active neighbours.

__global__ __launch_bounds__(256) void ban_apply_kernel(float* __restrict__ logits, int vocab, BanArgs a, PenHistory h) {
    extern __shared__ int ban_hist[];  // [max_hist]
    const int tid = threadIdx.x, b = blockIdx.x;
    const BanRules* __restrict__ r = a.rules;
    const int n = b < kBanMaxRows ? min(max(r->ngram[b], 0), kBanMaxNgram) : 0;
    const int min_tok = b < kBanMaxRows ? max(r->min_tokens[b], 0) : 0;
    const int n_words = min(max(r->n_words, 0), kBanMaxWords);
    const int n_supp = min(max(r->n_suppress, 0), kBanMaxSuppress);
    const int picked = h.ctrl ? h.ctrl->seq_len - 1 - a.prompt_len[b] : a.picked[b];
    const bool supp = n_supp > 0 && picked >= 0 && picked < min_tok;
    if (n == 0 && n_words == 0 && !supp) return;  // (uniform over the workgroup, which serves one row)
    const int cap = h.max_hist;
    const int n_prior = h.prior ? min(max(h.prior_len[b], 0), min(h.prior_stride, cap)) : 0;
    int past = 0, n_rec = 0;
    if (h.ctrl && h.rec) {  // the loop's record of this row: positions past .. step - 2 (the step in flight is step - 1)
        past = min(max(r->past_len, 0), h.rec_stride);
        n_rec = min(max(h.ctrl->step - 1 - past, 0), min(h.rec_stride - past, cap - n_prior));
    }
    const int L = n_prior + n_rec;
    for (int i = tid; i < L; i += 256)
        ban_hist[i] = i < n_prior ? h.prior[(size_t)b * h.prior_stride + i] : h.rec[(size_t)b * h.rec_stride + past + (i - n_prior)];
    __syncthreads();
    float* x = logits + (size_t)b * vocab;
    if (n >= 1) {  // windows 0 .. L - n (none while L < n); the suffix starts at L - n + 1
        const int suf = L - n + 1;
        for (int i = tid; i <= L - n; i += 256) {
            bool eq = true;
            for (int j = 0; j < n - 1; ++j) {
                const int t = ban_hist[i + j];
                eq = eq && t == ban_hist[suf + j] && (unsigned)t < (unsigned)vocab;
            }
            const int tok = ban_hist[i + n - 1];
            if (eq && (unsigned)tok < (unsigned)vocab) x[tok] = -INFINITY;
        }
    }
    if (tid < n_words) {
        const int m = min(r->word_len[tid], kBanMaxWordLen);
        if (m >= 1 && L >= m - 1) {
            bool eq = true;
            for (int j = 0; j < m - 1; ++j) eq = eq && ban_hist[L - m + 1 + j] == r->words[tid][j];
            const int tok = r->words[tid][m - 1];
            if (eq && (unsigned)tok < (unsigned)vocab) x[tok] = -INFINITY;
        }
    }
    if (supp && tid < n_supp) {
        const int tok = r->suppress[tid];
        if ((unsigned)tok < (unsigned)vocab) x[tok] = -INFINITY;
    }
}
