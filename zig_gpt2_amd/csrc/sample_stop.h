// sample_stop.h — stop tokens and stop sequences of the device loop, as the last optional stage of a decode step: the kernel
// (included by sample.hip behind sample_score.h, inside its unnamed namespace).  include/zgpt2.h zg_stop_conditions is the
// contract.
//
// One launch per step, one workgroup, one wave per row.  The step in flight records column col = ctrl->seq_len - 1; row b picked a
// token there iff col >= prompt_len[b] (embed_step_kernel's have_pick, seen from the step that made the pick).  The pick comes the
// way the log-probability stage gets it: the sampler's draw, or the lowest-index argmax of lm_head's partials with the embed
// kernel's compare rule and its clamp below the vocabulary.  Earlier columns come from the loop's own record: this step's embed
// kernel has already written column col - 1.  Lane j evaluates condition j (stop tokens first, then the sequences: at most 24), a
// ballot gives the lowest matching j, and lane 0 writes finish_col / reason of a row that had none.  A finished row is never
// evaluated again: its words do not change.  The stage only reads what the step left; comparisons of integers alone decide.
// Then row 0's wave tells the host, by stores to pinned host memory: done_col = f + 1 once every row has finished (f the highest
// finish column), and progress = col + 1 behind it, every step — in that order, so a host that reads progress first and finds done_col
// still 0 knows that the step of column f had not announced itself when progress was read.  Nothing here waits for the host.
// Every length read from device memory is clamped to its array; tokens are compared, never followed.

__global__ __launch_bounds__(512) void stop_step_kernel(const StopArgs a) {
    __shared__ int s_fin[kStopMaxRows];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_waves = a.batch > 4 ? 8 : 4;  // as launched
    const int col = min(max(a.col >= 0 ? a.col : a.ctrl->seq_len - 1, 0), a.stride - 1);
    const StopConds* __restrict__ c = a.conds;
    for (int b = wave; b < a.batch; b += n_waves) {
        int fin = a.finish_col[b];
        const int np = max(a.prompt_len[b], 0);
        if (fin < 0 && col >= np) {  // (uniform over the wave)
            int tok;
            if (a.picks) tok = a.picks[b];
            else if (a.pick_from_record) tok = a.tokens[(size_t)b * a.stride + col];
            else  // greedy: partials_first, the very pick embed_step_kernel makes of these partials one step later
                tok = partials_first(a.part_val + (size_t)b * a.part_stride, a.part_idx + (size_t)b * a.part_stride, a.n_part);
            tok = clamp_token(tok, a.vocab);
            const int n_ids = min(max(c->n_ids, 0), kStopMaxIds), n_seqs = min(max(c->n_seqs, 0), kStopMaxSeqs);
            bool hit = false;
            if (lane < n_ids) hit = c->ids[lane] == tok;
            else if (lane < n_ids + n_seqs) {
                const int k = lane - n_ids;
                const int len = min(max(c->seq_len[k], 1), kStopMaxSeqLen);
                const int first = col - len + 1;
                if (first >= np) {  // every column of the match is a picked one (np >= 0: never below the row)
                    hit = c->seq[k][len - 1] == tok;
                    for (int i = 0; i < len - 1 && hit; ++i) hit = a.tokens[(size_t)b * a.stride + first + i] == c->seq[k][i];
                }
            }
            const unsigned long long m = __ballot(hit);
            if (m != 0ull) {
                fin = col;
                if (lane == 0) {
                    a.finish_col[b] = col;
                    a.reason[b] = __ffsll((long long)m) - 1;
                }
            }
        }
        if (lane == 0) s_fin[b] = fin;
    }
    __syncthreads();
    if (threadIdx.x == 0 && a.host) {
        int hi = 0;
        bool all = true;
        for (int b = 0; b < a.batch; ++b) {
            all = all && s_fin[b] >= 0;
            hi = max(hi, s_fin[b]);
        }
        if (all) __hip_atomic_store(&a.host->done_col, (unsigned)(hi + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&a.host->progress, (unsigned)(col + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
