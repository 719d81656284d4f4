// api_gpt_debug.hip — model tier of the C ABI: everything that exists for tests and measurements.  The tap sink of a step and of
// a pass, the zg_debug_* row harnesses that run single stages on a caller's rows, the age, census, prefetch-stats and stamps
// entries, zg_gpt_profile_step and zg_gpt_time_kernel.  No product path reads this file.
#include <limits.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "api_gpt.h"

using namespace zg;

namespace {  // this unit only

// The device scratch of a per-call entry point (the zg_debug_* functions): one hipMalloc, freed on scope exit, handed out as typed
// 256-byte-aligned sub-buffers.  Sized the way carve() sizes the arena: the entry point's carving code runs once with no base
// (null pointers; the total is what it took) and once more with it.
struct DevScratch {
    Carver cv;
    char* base = nullptr;
    DevScratch() = default;
    DevScratch(const DevScratch&) = delete;
    ~DevScratch() { (void)hipFree(base); }
    template <class T>
    T* take(size_t bytes) {
        const size_t o = cv.take(bytes);
        return base ? reinterpret_cast<T*>(base + o) : nullptr;
    }
    template <class Carving>
    int carve(Carving carving) {
        carving();
        const size_t total = (cv.off + 255) & ~(size_t)255;
        cv = Carver{};
        ZG_HIP(hipMalloc(reinterpret_cast<void**>(&base), total));
        carving();
        return ZG_OK;
    }
};

}  // namespace

namespace zg {  // offered to the other units: api_gpt.h declares them

// One buffer into the sink: `rows` rows of row_bytes, src_pitch bytes apart in the source, packed in the arena
int tap_put(StepTaps* t, int cls, size_t layer, int buffer, int type, unsigned flags, const void* src, size_t rows, size_t row_bytes, size_t src_pitch,
            hipStream_t s) {
    static const size_t elem[5] = {4, 2, 2, 1, 4};
    const size_t off = (t->used + 255) & ~(size_t)255;
    zg_tap_entry e{};
    e.cls = cls, e.layer = (int)layer, e.buffer = buffer, e.type = type;
    e.offset = off, e.count = rows * row_bytes / elem[type], e.flags = flags;
    ZG_REQUIRE(!t->base || off + rows * row_bytes <= t->cap, ZG_ERR_ARG, "step taps: %zu bytes at %zu beyond the arena's %zu", rows * row_bytes, off, t->cap);
    t->table.push_back(e);
    t->used = off + rows * row_bytes;
    if (!t->base || rows * row_bytes == 0) return ZG_OK;
    if (rows == 1 || src_pitch == row_bytes) ZG_HIP(hipMemcpyAsync(t->base + off, src, rows * row_bytes, hipMemcpyDeviceToDevice, s));
    else ZG_HIP(hipMemcpy2DAsync(t->base + off, row_bytes, src, src_pitch, row_bytes, rows, hipMemcpyDeviceToDevice, s));
    return ZG_OK;
}

// Host ints (a launch's plan, the attention's geometry) into the sink: a table entry and room in the arena like any tap, filled on
// the host once the arena has been read back (zg_debug_gpt_pass_taps)
int tap_words(StepTaps* t, int cls, size_t layer, int buffer, const int* w, size_t n) {
    const size_t off = (t->used + 255) & ~(size_t)255;
    zg_tap_entry e{};
    e.cls = cls, e.layer = (int)layer, e.buffer = buffer, e.type = ZG_TAP_I32;
    e.offset = off, e.count = n;
    ZG_REQUIRE(!t->base || off + n * 4 <= t->cap, ZG_ERR_ARG, "taps: %zu bytes at %zu beyond the arena's %zu", n * 4, off, t->cap);
    t->table.push_back(e);
    t->used = off + n * 4;
    t->words.emplace_back(off, std::vector<int>(w, w + n));
    return ZG_OK;
}

// The K and V rows of positions < T of every (sequence, head) of layer l, [B][H][T][64] in storage format
int tap_caches(const zg_gpt* g, StepTaps* t, int cls, size_t l, unsigned flags, size_t T, hipStream_t s) {
    const size_t E = g->cfg.n_embed, B = g->batch, H = g->cfg.n_heads, C = g->cfg.context_size;
    const zg_layer& y = g->layers[l];
    const size_t lo = B * C * E * 2;
    const void* kv[2] = {y.k_cache, y.v_cache};
    for (int i = 0; i < 2; ++i) {
        const char* p = reinterpret_cast<const char*>(kv[i]);
        const int b0 = i ? ZG_TAP_V : ZG_TAP_K;
        if (g->kv_mode == 0) ZG_TRY(tap_put(t, cls, l, b0, ZG_TAP_F32, flags, p, B * H, T * 256, C * 256, s));
        else ZG_TRY(tap_put(t, cls, l, b0, g->kv_mode == 1 ? ZG_TAP_F16 : ZG_TAP_BF16, flags, p, B * H, T * 128, C * 128, s));
        if (g->kv_mode == 2) ZG_TRY(tap_put(t, cls, l, b0 + 1, ZG_TAP_U8, flags, p + lo, B * H, T * 64, C * 64, s));
    }
    return ZG_OK;
}

// What launch class cls of layer l wrote (include/zgpt2.h zg_debug_gpt_step_taps lists it), raw, in the handle's storage.
// cls -1: the layer's caches as the step finds them.  flags: ZG_TAP_* of the header.
int tap_class(const zg_gpt* g, StepTaps* t, int cls, size_t l, unsigned flags, hipStream_t s) {
    if (!t) return ZG_OK;
    const size_t E = g->cfg.n_embed, B = g->batch, H = g->cfg.n_heads, V = g->cfg.vocab_size;
    auto whole = [&](int buffer, int type, const void* src, size_t bytes, unsigned f) { return tap_put(t, cls, l, buffer, type, f, src, 1, bytes, bytes, s); };
    auto x_side = [&](bool planes_written) -> int {  // x and, with planes on, what travels with it
        ZG_TRY(whole(ZG_TAP_X, ZG_TAP_F32, g->x, B * E * 4, flags));
        if (g->modes.pl) ZG_TRY(whole(ZG_TAP_XP, ZG_TAP_BF16, g->xp, E * 48, flags | (planes_written ? 0u : ZG_TAP_NOT_WRITTEN)));
        if (g->modes.st) ZG_TRY(whole(ZG_TAP_XST, ZG_TAP_F32, g->xst, ((E + 15) / 16) * 8 * 2 * 4, flags | (planes_written ? 0u : ZG_TAP_NOT_WRITTEN)));
        return ZG_OK;
    };
    auto caches = [&]() { return tap_caches(g, t, cls, l, flags, t->seq_len, s); };  // positions < seq_len
    switch (cls) {
        case -1: return caches();
        case 0: return x_side(true);
        case 1:
            ZG_TRY(whole(ZG_TAP_Q, ZG_TAP_F32, g->q, B * E * 4, flags));
            return caches();
        case 2:
            if (g->modes.pl) return whole(ZG_TAP_AP, ZG_TAP_BF16, g->ap, E * 48, flags);
            return whole(ZG_TAP_PART, ZG_TAP_F32, g->part, B * H * g->max_splits * kPartStride * 4, flags);
        case 3: return x_side(true);
        case 4:
            if (g->modes.pl) return whole(ZG_TAP_HP, ZG_TAP_BF16, g->hp, 4 * E * 48, flags);
            return whole(ZG_TAP_H4, ZG_TAP_F32, g->h4, B * 4 * E * 4, flags);
        case 5: return x_side(l + 1 < g->cfg.n_layer);
        default:
            ZG_TRY(whole(ZG_TAP_LOGITS, ZG_TAP_F32, g->logits, B * V * 4, flags));
            ZG_TRY(tap_put(t, cls, l, ZG_TAP_PART_VAL, ZG_TAP_F32, flags, g->part_val, B, (size_t)g->lm_grid * 4, (size_t)g->lm_grid * 4, s));
            return tap_put(t, cls, l, ZG_TAP_PART_IDX, ZG_TAP_I32, flags, g->part_idx, B, (size_t)g->lm_grid * 4, (size_t)g->lm_grid * 4, s);
    }
}

}  // namespace zg

extern "C" {

// zg_gpt_forward(seq_len, tokens, compute_logits = 1) as an eager step whose launch classes are tapped (tests; include/zgpt2.h).
// arena_out == nullptr: nothing runs, the sizes alone are reported.  Allocates its device arena per call.
int zg_debug_gpt_step_taps(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, void* arena_out, size_t arena_bytes, size_t* arena_used,
                           zg_tap_entry* table_out, size_t table_len, size_t* n_entries, int* info, size_t n_info) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && tokens && arena_used && n_entries, ZG_ERR_ARG, "debug_gpt_step_taps: null argument");
    ZG_REQUIRE(seq_len >= 1 && seq_len <= g->cfg.context_size, ZG_ERR_SHAPE, "debug_gpt_step_taps: seq_len %zu outside 1..%zu", seq_len, g->cfg.context_size);
    const size_t L = g->cfg.n_layer;
    StepTaps plan;  // the sizing pass: the table of the step, nothing copied
    plan.seq_len = seq_len;
    ZG_TRY(tap_class(g, &plan, 0, 0, 0, nullptr));
    for (size_t l = 0; l < L; ++l)
        for (int cls = -1; cls <= 5; ++cls)
            if (cls != 0) ZG_TRY(tap_class(g, &plan, cls, l, 0, nullptr));
    ZG_TRY(tap_class(g, &plan, 6, 0, 0, nullptr));
    const size_t cap = plan.used + 256 * (plan.table.size() + 1);  // (the step's own order pads differently)
    *arena_used = cap;
    *n_entries = plan.table.size();
    if (info && n_info >= ZG_TAP_INFO_INTS) {
        const int v[ZG_TAP_INFO_INTS] = {g->modes.pl, g->modes.st, g->modes.tags, g->modes.fused, g->max_splits, g->lm_grid, bucket_t_hi(g, seq_len), g->kv_mode, g->wt};
        memcpy(info, v, sizeof(v));
    }
    if (!arena_out) return ZG_OK;
    ZG_REQUIRE(table_out && arena_bytes >= cap && table_len >= plan.table.size(), ZG_ERR_SHAPE, "debug_gpt_step_taps: %zu arena bytes and %zu table entries needed",
               cap, plan.table.size());
    hipStream_t s = gs(g);
    StepTaps taps;
    taps.seq_len = seq_len;
    taps.cap = cap;
    DevScratch ds;
    ZG_TRY(ds.carve([&] { taps.base = ds.take<char>(cap); }));
    ZG_HIP(hipMemsetAsync(taps.base, 0, cap, s));
    ZG_TRY(forward_enqueue(g, seq_len, tokens, n_tokens, 1, nullptr, 0, &taps));
    ZG_HIP(hipStreamSynchronize(s));
    ZG_TRY(check_fault(g));
    ZG_REQUIRE(taps.used <= cap && taps.table.size() == plan.table.size(), ZG_ERR_ARG, "debug_gpt_step_taps: the step tapped %zu entries in %zu bytes, planned %zu in %zu",
               taps.table.size(), taps.used, plan.table.size(), cap);
    ZG_HIP(hipMemcpy(arena_out, taps.base, taps.used, hipMemcpyDeviceToHost));
    memcpy(table_out, taps.table.data(), taps.table.size() * sizeof(zg_tap_entry));
    *arena_used = taps.used;
    return ZG_OK;
}

// zg_gpt_prefill / zg_gpt_extend / zg_gpt_score with every launch of the pass tapped (tests; include/zgpt2.h).  arena_out == nullptr:
// nothing runs; an upper bound of what a call needs is reported.  Allocates its device arena per call.
int zg_debug_gpt_pass_taps(zg_gpt* g, size_t past_len, const size_t* tokens, size_t token_stride, size_t n_tokens, int compute_logits, int score, size_t top_n,
                           float* logits_out, size_t logits_len, void* arena_out, size_t arena_bytes, size_t* arena_used, zg_tap_entry* table_out,
                           size_t table_len, size_t* n_entries, int* info, size_t n_info) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && tokens && arena_used && n_entries, ZG_ERR_ARG, "debug_gpt_pass_taps: null argument");
    ZG_REQUIRE(g->pass.x != nullptr, ZG_ERR_UNSUPPORTED, "debug_gpt_pass_taps: the handle was created with ZG_GPT_NO_PREFILL");
    const size_t C = g->cfg.context_size, E = g->cfg.n_embed, L = g->cfg.n_layer, B = g->batch;
    ZG_REQUIRE(n_tokens >= 1 && past_len + n_tokens <= C, ZG_ERR_SHAPE, "debug_gpt_pass_taps: %zu tokens behind %zu positions (context %zu)", n_tokens, past_len, C);
    ZG_REQUIRE(!score || g->score.logits != nullptr, ZG_ERR_UNSUPPORTED, "debug_gpt_pass_taps: the handle was created without ZG_GPT_SCORE");
    // an upper bound of the pass's taps: per layer two cache taps of K and V (at most 4 bytes an element, and the B24 byte plane
    // within that), x twice, pass.a four times, qkv, pass.h, three plans and the geometry; class 0 and 1 once; the score stage
    const size_t M = B * n_tokens, T = std::min(C, past_len + n_tokens + kPassTapRowsBehind), blocks = (M + kScoreRows - 1) / kScoreRows;
    const size_t per_layer = 4 * B * E * T * 4 + 2 * M * E * 4 + 4 * M * kSplit * E * 2 + M * 3 * E * 4 + M * kSplit * 4 * E * 2;
    const size_t entries = 2 + L * 24 + (score ? 1 + 3 * blocks : 0);
    const size_t cap = L * per_layer + M * E * 4 + M * kSplit * E * 2 + (score ? M * kSplit * E * 2 + M * g->score.v64 * 4 : 0) + 256 * (entries + 1);
    *arena_used = cap;
    *n_entries = entries;
    if (info && n_info >= ZG_PASS_INFO_INTS) {
        const bool f32w = g->wt != WT_BF16;
        const int v[ZG_PASS_INFO_INTS] = {f32w ? kSplit : (g->flags & ZG_GPT_PREFILL_2PLANE) ? 2 : kSplit, g->kv_mode, g->wt,
                                          (int)std::min(g->pass.ws_floats, (size_t)INT_MAX), !f32w && g->pass.sk_flags != nullptr, (int)g->score.v64, (int)kScoreRows};
        memcpy(info, v, sizeof(v));
    }
    if (!arena_out) return ZG_OK;
    ZG_REQUIRE(table_out && arena_bytes >= cap && table_len >= entries, ZG_ERR_SHAPE, "debug_gpt_pass_taps: %zu arena bytes and %zu table entries needed", cap,
               entries);
    hipStream_t s = gs(g);
    StepTaps taps;
    taps.cap = cap;
    DevScratch ds;
    ZG_TRY(ds.carve([&] { taps.base = ds.take<char>(cap); }));
    ZG_HIP(hipMemsetAsync(taps.base, 0, cap, s));
    if (score) {
        const ScoreCall sc{top_n, logits_out, logits_len};
        ZG_TRY(pass_impl(g, past_len, tokens, token_stride, n_tokens, 1, nullptr, 0, "debug_gpt_pass_taps", &sc, &taps));
    } else
        ZG_TRY(pass_impl(g, past_len, tokens, token_stride, n_tokens, compute_logits, logits_out, logits_len, "debug_gpt_pass_taps", nullptr, &taps));
    ZG_REQUIRE(taps.used <= cap && taps.table.size() <= entries, ZG_ERR_ARG, "debug_gpt_pass_taps: the pass tapped %zu entries in %zu bytes, bound %zu in %zu",
               taps.table.size(), taps.used, entries, cap);
    ZG_HIP(hipMemcpy(arena_out, taps.base, taps.used, hipMemcpyDeviceToHost));
    for (const auto& w : taps.words) memcpy(static_cast<char*>(arena_out) + w.first, w.second.data(), w.second.size() * 4);
    memcpy(table_out, taps.table.data(), taps.table.size() * sizeof(zg_tap_entry));
    *arena_used = taps.used;
    *n_entries = taps.table.size();
    return ZG_OK;
}

// The stop kernel alone on the caller's token rows (tests): one eager launch per column, the pick of column s being tokens[b][s].
// Allocates per call: the device scratch, and the pinned words the kernel stores to.
int zg_debug_stop_rows(const size_t* tokens, size_t batch, size_t stride, const size_t* first_cols, size_t n_cols, const zg_stop_conditions* stop,
                       size_t* finish_cols_out, int* reasons_out, size_t* done_col_out) {
    ZG_TRY(require_init());
    const size_t lim = 0x7fffffff;
    ZG_REQUIRE(tokens && first_cols && finish_cols_out && reasons_out && done_col_out && batch >= 1 && batch <= (size_t)kStopMaxRows && n_cols >= 1 &&
                   n_cols <= stride && stride <= (size_t)1 << 20,
               ZG_ERR_ARG, "debug_stop_rows: bad argument");
    ZG_TRY(check_stop(stop, lim, "debug_stop_rows"));
    std::vector<int> h_tok(batch * stride), h_first(batch);
    for (size_t b = 0; b < batch; ++b) {
        h_first[b] = (int)std::min(first_cols[b], lim);
        for (size_t i = 0; i < n_cols; ++i) {
            ZG_REQUIRE(tokens[b * stride + i] < lim, ZG_ERR_SHAPE, "debug_stop_rows: token %zu", tokens[b * stride + i]);
            h_tok[b * stride + i] = (int)tokens[b * stride + i];
        }
    }
    StopConds h_conds;
    fill_stop(&h_conds, *stop);
    struct Pinned {
        StopHost* p = nullptr;
        ~Pinned() { (void)hipHostFree(p); }
    } host;
    ZG_HIP(hipHostMalloc(reinterpret_cast<void**>(&host.p), sizeof(StopHost), hipHostMallocDefault));
    host.p->progress = host.p->done_col = 0u;
    hipStream_t s = ctx().stream;
    DevScratch ds;
    StopArgs a{};
    int *d_tok, *d_first;
    StopConds* d_conds;
    ZG_TRY(ds.carve([&] {
        d_tok = ds.take<int>(batch * stride * 4);
        d_first = ds.take<int>(batch * 4);
        d_conds = ds.take<StopConds>(sizeof(StopConds));
        a.finish_col = ds.take<int>(batch * 4);
        a.reason = ds.take<int>(batch * 4);
    }));
    ZG_HIP(hipMemcpyAsync(d_tok, h_tok.data(), batch * stride * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_first, h_first.data(), batch * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_conds, &h_conds, sizeof(StopConds), hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemsetAsync(a.finish_col, 0xff, batch * 4, s));
    ZG_HIP(hipMemsetAsync(a.reason, 0xff, batch * 4, s));
    a.conds = d_conds;
    a.tokens = d_tok;
    a.stride = (int)stride;
    a.prompt_len = d_first;
    a.batch = (int)batch;
    a.vocab = (int)lim;
    a.pick_from_record = 1;
    a.host = host.p;
    for (size_t c = 0; c < n_cols; ++c) {
        a.col = (int)c;
        ZG_TRY(launch_stop(a, s));
    }
    std::vector<int> fin(batch), reason(batch);
    ZG_HIP(hipMemcpyAsync(fin.data(), a.finish_col, batch * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipMemcpyAsync(reason.data(), a.reason, batch * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipStreamSynchronize(s));
    ZG_REQUIRE(host.p->progress == (unsigned)n_cols, ZG_ERR_HIP, "debug_stop_rows: the kernel reported column %u of %zu", host.p->progress, n_cols);
    for (size_t b = 0; b < batch; ++b) {
        finish_cols_out[b] = fin[b] < 0 ? ZG_STOP_NONE : (size_t)fin[b];
        reasons_out[b] = fin[b] < 0 ? -1 : reason[b];
    }
    *done_col_out = host.p->done_col;
    return ZG_OK;
}

// The beam kernel alone over the caller's lists (tests; include/zgpt2.h): launched eagerly once per column, state carried, on a
// scratch record whose columns are the caller's (column 0 here is first_col of the call).  Allocates per call.
int zg_debug_beam_rows(const int32_t* top_ids, const float* top_logprobs, size_t n_cols, size_t batch, size_t vocab, size_t first_col,
                       const zg_beam_options* beam, int32_t* tokens_out, int32_t* parents_out, float* scores_out, float* logprobs_out, float* pool_out,
                       int32_t* pool_n_out, int32_t* done_cols_out, size_t* done_col_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(top_ids && top_logprobs && tokens_out && parents_out && scores_out && logprobs_out && pool_out && pool_n_out && done_cols_out && done_col_out &&
                   n_cols >= 1 && n_cols <= 4096 && first_col <= (size_t)1 << 20 && vocab >= 1 && vocab <= 0x7fffffff,
               ZG_ERR_ARG, "debug_beam_rows: bad argument");
    ZG_REQUIRE(beam != nullptr && beam->size == sizeof(zg_beam_options), ZG_ERR_ARG, "debug_beam_rows: null options, or their size field is not sizeof(zg_beam_options)");
    const size_t W = beam->num_beams;
    ZG_REQUIRE(W >= 1 && W <= ZG_BEAM_MAX && batch >= 1 && batch <= (size_t)kBeamRows && batch % W == 0 && 2 * W <= vocab, ZG_ERR_ARG,
               "debug_beam_rows: num_beams %zu for %zu rows and %zu tokens", W, batch, vocab);
    ZG_REQUIRE(std::isfinite(beam->length_penalty), ZG_ERR_ARG, "debug_beam_rows: length_penalty is not finite");
    ZG_REQUIRE(beam->eos_id == ZG_BEAM_NO_EOS || beam->eos_id < vocab, ZG_ERR_SHAPE, "debug_beam_rows: eos_id %zu >= vocab %zu", beam->eos_id, vocab);
    const size_t K = ZG_LOGPROBS_TOP_MAX, T = 2 * W, G = batch / W;
    // the record layout the stage reads: [batch][n_cols][20]
    std::vector<int> h_ids(batch * n_cols * K, 0);
    std::vector<float> h_lp(batch * n_cols * K, 0.0f), h_pow(n_cols + 1);
    for (size_t c = 0; c < n_cols; ++c)
        for (size_t b = 0; b < batch; ++b)
            for (size_t j = 0; j < T; ++j) {
                h_ids[(b * n_cols + c) * K + j] = top_ids[(c * batch + b) * T + j];
                h_lp[(b * n_cols + c) * K + j] = top_logprobs[(c * batch + b) * T + j];
            }
    fill_lenpow(h_pow.data(), n_cols + 1, beam->length_penalty);
    BeamState h_st;
    fill_beam_state(&h_st, *beam, 0);
    struct Pinned {
        StopHost* p = nullptr;
        ~Pinned() { (void)hipHostFree(p); }
    } host;
    ZG_HIP(hipHostMalloc(reinterpret_cast<void**>(&host.p), sizeof(StopHost), hipHostMallocDefault));
    host.p->progress = host.p->done_col = 0u;
    hipStream_t s = ctx().stream;
    DevScratch ds;
    BeamArgs a{};
    int *d_ids, *d_tok;  // d_tok: the picks of every column, [n_cols][batch] — `sampled` copied behind each launch
    float *d_lp, *d_pow;
    ZG_TRY(ds.carve([&] {
        d_ids = ds.take<int>(h_ids.size() * 4);
        d_tok = ds.take<int>(n_cols * batch * 4);
        d_lp = ds.take<float>(h_lp.size() * 4);
        d_pow = ds.take<float>(h_pow.size() * 4);
        a.st = ds.take<BeamState>(sizeof(BeamState));
        a.sampled = ds.take<int>(batch * 4);
        a.parent = ds.take<int>(batch * n_cols * 4);
        a.score = ds.take<float>(batch * n_cols * 4);
        a.logprob = ds.take<float>(batch * n_cols * 4);
    }));
    ZG_HIP(hipMemcpyAsync(d_ids, h_ids.data(), h_ids.size() * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_lp, h_lp.data(), h_lp.size() * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_pow, h_pow.data(), h_pow.size() * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(a.st, &h_st, sizeof(BeamState), hipMemcpyHostToDevice, s));
    a.lenpow = d_pow;
    a.n_lenpow = (int)n_cols + 1;
    a.batch = (int)batch;
    a.vocab = (int)vocab;
    a.top_ids = d_ids;
    a.top_logprobs = d_lp;
    a.stride = (int)n_cols;
    a.host = host.p;
    for (size_t c = 0; c < n_cols; ++c) {
        a.col = (int)c;
        ZG_TRY(launch_beam(a, s));
        ZG_HIP(hipMemcpyAsync(d_tok + c * batch, a.sampled, batch * 4, hipMemcpyDeviceToDevice, s));
    }
    std::vector<int> par(batch * n_cols);
    std::vector<float> sc(batch * n_cols), lpv(batch * n_cols);
    ZG_HIP(hipMemcpyAsync(tokens_out, d_tok, n_cols * batch * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipMemcpyAsync(par.data(), a.parent, par.size() * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipMemcpyAsync(sc.data(), a.score, sc.size() * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipMemcpyAsync(lpv.data(), a.logprob, lpv.size() * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipMemcpyAsync(&h_st, a.st, sizeof(BeamState), hipMemcpyDeviceToHost, s));
    ZG_HIP(hipStreamSynchronize(s));
    ZG_REQUIRE(host.p->progress == (unsigned)n_cols, ZG_ERR_HIP, "debug_beam_rows: the kernel reported column %u of %zu", host.p->progress, n_cols);
    for (size_t c = 0; c < n_cols; ++c)
        for (size_t b = 0; b < batch; ++b) {
            parents_out[c * batch + b] = par[b * n_cols + c];
            scores_out[c * batch + b] = sc[b * n_cols + c];
            logprobs_out[c * batch + b] = lpv[b * n_cols + c];
        }
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t gr = 0; gr < G; ++gr) {
        pool_n_out[gr] = h_st.pool_n[gr];
        done_cols_out[gr] = h_st.done_col[gr] < 0 ? -1 : h_st.done_col[gr] + (int)first_col;
        for (size_t k = 0; k < W; ++k) {
            const size_t e = gr * W + k;
            const bool has = (int)k < h_st.pool_n[gr];
            pool_out[e * 4 + 0] = has ? h_st.pool_sum[e] : nan;
            pool_out[e * 4 + 1] = has ? h_st.pool_norm[e] : nan;
            pool_out[e * 4 + 2] = has ? (float)h_st.pool_parent[e] : nan;
            pool_out[e * 4 + 3] = has ? (float)(h_st.pool_col[e] + (int)first_col) : nan;
        }
    }
    *done_col_out = host.p->done_col ? host.p->done_col + first_col : 0;
    return ZG_OK;
}

// The greedy pick alone on the caller's partials (tests): the product's embed_step_kernel as zg_gpt_argmax launches it, on a scratch
// control block (step 0, generate mode).  Allocates per call.
int zg_debug_pick_rows(const float* part_val, const int32_t* part_idx, size_t batch, size_t n_part, size_t vocab, size_t* picks_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(part_val && part_idx && picks_out && batch >= 1 && batch <= 8 && n_part >= 1 && n_part <= 4096 && vocab >= 1 && vocab <= (size_t)0x7fffffff,
               ZG_ERR_ARG, "debug_pick_rows: bad argument");
    hipStream_t s = ctx().stream;
    DevScratch ds;
    float* d_val;
    int *d_idx, *d_zero, *d_pick;
    StepCtrl* d_ctrl;
    ZG_TRY(ds.carve([&] {
        d_val = ds.take<float>(batch * n_part * 4);
        d_idx = ds.take<int>(batch * n_part * 4);
        d_ctrl = ds.take<StepCtrl>(sizeof(StepCtrl));
        d_zero = ds.take<int>(batch * 4);  // what the kernel reads beside the partials and does not use in this form
        d_pick = ds.take<int>(batch * 4);
    }));
    ZG_HIP(hipMemcpyAsync(d_val, part_val, batch * n_part * 4, hipMemcpyDefault, s));
    ZG_HIP(hipMemcpyAsync(d_idx, part_idx, batch * n_part * 4, hipMemcpyDefault, s));
    ZG_HIP(hipMemsetAsync(d_ctrl, 0, sizeof(StepCtrl), s));
    ZG_HIP(hipMemsetAsync(d_zero, 0, batch * 4, s));
    EmbedArgs e{};
    e.ctrl = d_ctrl;
    e.part_val = d_val;
    e.part_idx = d_idx;
    e.part_stride = e.n_partials = (int)n_part;
    e.prompt = e.forced = e.sampled = d_zero;  // one token per row, no prompt lengths
    e.prompt_stride = 1;
    e.batch = (int)batch;
    e.vocab = (int)vocab;
    e.cur_token = d_pick;
    e.finish_only = 2;
    ZG_TRY(launch_embed_step(e, s));
    int h_pick[8];
    ZG_HIP(hipMemcpyAsync(h_pick, d_pick, batch * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipStreamSynchronize(s));
    for (size_t b = 0; b < batch; ++b) picks_out[b] = (size_t)h_pick[b];
    return ZG_OK;
}

// What the two debug entry points below share: the checks on top_n and its outputs ...
static int check_debug_top_n(size_t top_n, size_t vocab, const size_t* top_ids_out, const float* top_logprobs_out, const char* who) {
    ZG_TRY(check_top_n(top_n, vocab, who));
    ZG_REQUIRE(top_n == 0 || (top_ids_out && top_logprobs_out), ZG_ERR_ARG, "%s: top_n %zu without its outputs", who, top_n);
    return ZG_OK;
}
// ... record buffers [rows][stride], carved from the call's scratch ...
static LogprobRec debug_record(DevScratch& ds, size_t rows, size_t stride) {
    LogprobRec rec{};
    rec.logprob = ds.take<float>(rows * stride * 4);
    rec.top_ids = ds.take<int>(rows * stride * ZG_LOGPROBS_TOP_MAX * 4);
    rec.top_logprobs = ds.take<float>(rows * stride * ZG_LOGPROBS_TOP_MAX * 4);
    rec.stride = (int)stride;
    return rec;
}
// ... and the way back of its elements col0 .. col0 + n - 1: the outputs may be host or device memory, so the
// alternatives are packed on the host and leave in one copy each.  Drains the stream.
static int debug_record_out(const LogprobRec& rec, size_t col0, size_t n, size_t top_n, float* logprobs_out, size_t* top_ids_out, float* top_logprobs_out,
                            hipStream_t s) {
    const size_t K = ZG_LOGPROBS_TOP_MAX;
    std::vector<int> h_ids(n * K);
    std::vector<float> h_top(n * K);
    ZG_HIP(hipMemcpyAsync(logprobs_out, rec.logprob + col0, n * 4, hipMemcpyDefault, s));
    if (top_n) {
        ZG_HIP(hipMemcpyAsync(h_ids.data(), rec.top_ids + col0 * K, n * K * 4, hipMemcpyDeviceToHost, s));
        ZG_HIP(hipMemcpyAsync(h_top.data(), rec.top_logprobs + col0 * K, n * K * 4, hipMemcpyDeviceToHost, s));
    }
    ZG_HIP(hipStreamSynchronize(s));
    if (!top_n) return ZG_OK;
    std::vector<size_t> ids(n * top_n);
    std::vector<float> vals(n * top_n);
    unpack_top(h_ids.data(), h_top.data(), n, top_n, ids.data(), vals.data());
    ZG_HIP(hipMemcpy(top_ids_out, ids.data(), ids.size() * sizeof(size_t), hipMemcpyDefault));
    ZG_HIP(hipMemcpy(top_logprobs_out, vals.data(), vals.size() * 4, hipMemcpyDefault));
    return ZG_OK;
}

// The log-probability kernels on the caller's rows (tests): the two launches of the stage, a small kernel standing in for
// lm_head's partials.  Allocates its workspace per call.
int zg_debug_logprob_rows(const float* logits, size_t batch, size_t vocab, const size_t* tokens, size_t top_n, float* logprobs_out, size_t* top_ids_out,
                          float* top_logprobs_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(logits && tokens && logprobs_out && batch >= 1 && batch <= 64 && vocab >= 1 && vocab <= (size_t)64 * 4096, ZG_ERR_ARG,
               "debug_logprob_rows: bad argument");
    ZG_TRY(check_debug_top_n(top_n, vocab, top_ids_out, top_logprobs_out, "debug_logprob_rows"));
    std::vector<int> h_tok(batch);
    std::vector<size_t> h_tok_in(batch);
    ZG_HIP(hipMemcpy(h_tok_in.data(), tokens, batch * sizeof(size_t), hipMemcpyDefault));
    for (size_t b = 0; b < batch; ++b) {
        ZG_REQUIRE(h_tok_in[b] < vocab, ZG_ERR_SHAPE, "debug_logprob_rows: token %zu >= vocab %zu", h_tok_in[b], vocab);
        h_tok[b] = (int)h_tok_in[b];
    }
    const int B = (int)batch, V = (int)vocab, n_part = std::min(64, (V + 255) / 256);
    hipStream_t s = ctx().stream;
    DevScratch ds;
    float *d_logits, *d_part;
    int *d_tok, *d_top;
    LogprobWs ws;
    LogprobRec rec;
    ZG_TRY(ds.carve([&] {
        d_logits = ds.take<float>(batch * vocab * 4);
        ws = logprob_workspace(ds.take<char>(logprob_workspace_bytes(B, V)), B, V);
        d_part = ds.take<float>((size_t)B * n_part * 4);
        d_tok = ds.take<int>(batch * 4);
        d_top = ds.take<int>(4);
        rec = debug_record(ds, batch, 1);
    }));
    const int h_top_n = (int)top_n;
    ZG_HIP(hipMemcpyAsync(d_logits, logits, batch * vocab * 4, hipMemcpyDefault, s));
    ZG_HIP(hipMemcpyAsync(d_tok, h_tok.data(), batch * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_top, &h_top_n, 4, hipMemcpyHostToDevice, s));
    ZG_TRY(launch_row_max_partials(d_logits, B, V, d_part, n_part, s));
    ZG_TRY(launch_logprob(d_logits, B, V, d_part, nullptr, n_part, n_part, d_top, ws, d_tok, nullptr, nullptr, rec, s));
    return debug_record_out(rec, 0, batch, top_n, logprobs_out, top_ids_out, top_logprobs_out, s);
}

// The scoring kernels on the caller's rows (tests): the two launches of zg_gpt_score's statistics stage, the rows standing for one
// sequence of rows + 1 positions whose position r + 1 holds targets[r].  Allocates its workspace per call.
int zg_debug_score_rows(const float* logits, size_t rows, size_t vocab, size_t row_stride, const size_t* targets, size_t top_n, float* logprobs_out,
                        size_t* top_ids_out, float* top_logprobs_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(logits && targets && logprobs_out && rows >= 1 && rows <= 4096 && vocab >= 1 && vocab <= (size_t)64 * 4096 && row_stride >= vocab &&
                   row_stride <= (size_t)1 << 20,
               ZG_ERR_ARG, "debug_score_rows: bad argument");
    ZG_TRY(check_debug_top_n(top_n, vocab, top_ids_out, top_logprobs_out, "debug_score_rows"));
    const size_t cols = rows + 1;
    std::vector<int> h_tok(cols, 0);
    std::vector<size_t> h_tok_in(rows);
    ZG_HIP(hipMemcpy(h_tok_in.data(), targets, rows * sizeof(size_t), hipMemcpyDefault));
    for (size_t r = 0; r < rows; ++r) {
        ZG_REQUIRE(h_tok_in[r] < vocab, ZG_ERR_SHAPE, "debug_score_rows: target %zu >= vocab %zu", h_tok_in[r], vocab);
        h_tok[r + 1] = (int)h_tok_in[r];
    }
    const int R = (int)rows, V = (int)vocab;
    hipStream_t s = ctx().stream;
    DevScratch ds;
    float* d_logits;
    int *d_tok, *d_top;
    ScoreWs ws;
    LogprobRec rec;
    ZG_TRY(ds.carve([&] {
        d_logits = ds.take<float>(rows * row_stride * 4);
        ws = score_workspace(ds.take<char>(score_workspace_bytes(R, V)), R, V);
        d_top = ds.take<int>(4);
        d_tok = ds.take<int>(cols * 4);
        rec = debug_record(ds, 1, cols);
    }));
    const int h_top_n = (int)top_n;
    ZG_HIP(hipMemcpyAsync(d_logits, logits, rows * row_stride * 4, hipMemcpyDefault, s));
    ZG_HIP(hipMemcpyAsync(d_tok, h_tok.data(), cols * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_top, &h_top_n, 4, hipMemcpyHostToDevice, s));
    const ScoreTargets tg{d_tok, (int)cols, (int)cols, 0, 0};
    ZG_TRY(launch_score(d_logits, R, V, (int)row_stride, d_top, ws, tg, rec, s));
    return debug_record_out(rec, 1, rows, top_n, logprobs_out, top_ids_out, top_logprobs_out, s);
}

// The sampler chain on the caller's rows (tests), a small kernel standing in for lm_head's row-maximum partials: the body of
// zg_debug_edit_rows, and with edits null — no edit stage, no min-p — of zg_debug_sample_rows; with a table of the caller's
// (opt null, per_row), of zg_debug_sample_rows_each.  Allocates its workspace per call.
static int debug_sample_rows(const float* logits, size_t batch, size_t vocab, const zg_sample_options* opt, const zg_row_sampling* each,
                             const zg_logit_edits* edits, const float* uniforms, float* edited_out, size_t* tokens_out, float* probs_out,
                             float* thresholds_out, const char* who) {
    if (!each) ZG_TRY(check_sample_options(opt, who));
    ZG_REQUIRE(logits && uniforms && tokens_out && batch >= 1 && batch <= 64 && vocab >= 1 && vocab <= (size_t)64 * 4096, ZG_ERR_ARG, "%s: bad argument", who);
    std::vector<char> block(edits ? edit_block_bytes(vocab) : 0);
    bool stage_on = false;
    if (edits) ZG_TRY(build_edits(edits, vocab, who, block.data(), &stage_on));
    const int B = (int)batch, V = (int)vocab, n_part = std::min(64, (V + 255) / 256);
    std::vector<zg_row_sampling> table(batch);
    if (!each) uniform_rows(table.data(), batch, *opt, edits ? edits->min_p : 0.0f, nullptr, 0);
    std::vector<SampleParams> hp(batch);
    StepTail plan;
    ZG_TRY(plan_rows(each ? each : table.data(), batch, vocab, 0, who, hp.data(), nullptr, nullptr, &plan));
    const SamplerMode mode = plan.sampler;
    hipStream_t s = ctx().stream;
    DevScratch ds;
    char *d_filt, *d_edit;
    SampleParams* d_par;
    float* d_u;
    SamplerChain c{};
    c.batch = B, c.vocab = V, c.n_part = n_part, c.temp = each ? 1.0f : opt->temp, c.per_row = each != nullptr, c.write_probs = probs_out != nullptr;
    ZG_TRY(ds.carve([&] {
        d_filt = ds.take<char>(filter_workspace_bytes(B));
        c.filt = filter_workspace(d_filt, B);
        c.logits = ds.take<float>(batch * vocab * 4);
        c.seg_ws = ds.take<float>(sample_workspace_floats(B) * 4);
        c.part_val = ds.take<float>((size_t)B * n_part * 4);
        c.part_idx = ds.take<int>((size_t)B * n_part * 4);
        c.params = d_par = ds.take<SampleParams>(batch * sizeof(SampleParams));
        c.u = d_u = ds.take<float>(batch * 4);
        c.pick = ds.take<int>(batch * 4);
        d_edit = ds.take<char>(block.size());
    }));
    c.edit_tab = reinterpret_cast<const EditTable*>(d_edit);
    c.edit_keep = reinterpret_cast<const unsigned*>(d_edit + sizeof(EditTable));
    std::vector<int> h_tok(batch);
    std::vector<float> h_u(batch);
    for (size_t b = 0; b < batch; ++b) {  // (host or device memory)
        float u;
        ZG_HIP(hipMemcpy(&u, uniforms + b, 4, hipMemcpyDefault));
        ZG_REQUIRE(u >= 0.0f && u < 1.0f, ZG_ERR_ARG, "%s: uniform %f outside [0,1)", who, u);
        h_u[b] = u;
    }
    ZG_HIP(hipMemsetAsync(d_filt, 0, filter_workspace_bytes(B), s));  // (the selection chain starts from a zeroed workspace and leaves it so)
    ZG_HIP(hipMemcpyAsync(c.logits, logits, batch * vocab * 4, hipMemcpyDefault, s));
    ZG_HIP(hipMemcpyAsync(d_u, h_u.data(), batch * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_par, hp.data(), batch * sizeof(SampleParams), hipMemcpyHostToDevice, s));
    ZG_TRY(launch_row_max_partials(c.logits, B, V, c.part_val, n_part, s));  // (lm_head's stand-in: the partials of the row as the chain finds it)
    if (stage_on) ZG_HIP(hipMemcpyAsync(d_edit, block.data(), block.size(), hipMemcpyHostToDevice, s));
    // the chain in two parts, the edited rows leaving between them: the row stage (no sampler), then the sampler alone
    ZG_TRY(emit_sampler_chain(c, StepTail{GREEDY, false, false, false, stage_on}, s));
    if (edited_out) ZG_HIP(hipMemcpyAsync(edited_out, c.logits, batch * vocab * 4, hipMemcpyDefault, s));
    ZG_TRY(emit_sampler_chain(c, StepTail{mode}, s));
    ZG_HIP(hipMemcpyAsync(h_tok.data(), c.pick, batch * 4, hipMemcpyDeviceToHost, s));
    if (probs_out) ZG_HIP(hipMemcpyAsync(probs_out, c.logits, batch * vocab * 4, hipMemcpyDefault, s));
    std::vector<float> ninf(batch, -INFINITY);  // nothing truncates: nothing is dropped
    if (thresholds_out) ZG_HIP(hipMemcpyAsync(thresholds_out, threshold_sampler(mode) ? c.filt.tau : ninf.data(), batch * 4, hipMemcpyDefault, s));
    ZG_HIP(hipStreamSynchronize(s));
    for (size_t b = 0; b < batch; ++b) tokens_out[b] = (size_t)h_tok[b];
    return ZG_OK;
}

int zg_debug_sample_rows(const float* logits, size_t batch, size_t vocab, const zg_sample_options* opt, const float* uniforms, size_t* tokens_out,
                         float* probs_out, float* thresholds_out) {
    ZG_TRY(require_init());
    return debug_sample_rows(logits, batch, vocab, opt, nullptr, nullptr, uniforms, nullptr, tokens_out, probs_out, thresholds_out, "debug_sample_rows");
}

// ... with the edit stage in front of the sampler and min-p in it; here the edits are required.  Everything off: zg_debug_sample_rows.
int zg_debug_edit_rows(const float* logits, size_t batch, size_t vocab, const zg_sample_options* opt, const zg_logit_edits* edits, const float* uniforms,
                       float* edited_out, size_t* tokens_out, float* probs_out, float* thresholds_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(edits != nullptr, ZG_ERR_ARG, "debug_edit_rows: edits is null");
    return debug_sample_rows(logits, batch, vocab, opt, nullptr, edits, uniforms, edited_out, tokens_out, probs_out, thresholds_out, "debug_edit_rows");
}

// ... with one zg_row_sampling per row; the edits carry lists only and may be null
int zg_debug_sample_rows_each(const float* logits, size_t batch, size_t vocab, const zg_row_sampling* rows, size_t n_rows, const zg_logit_edits* edits,
                              const float* uniforms, float* edited_out, size_t* tokens_out, float* probs_out, float* thresholds_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(rows != nullptr, ZG_ERR_ARG, "debug_sample_rows_each: rows is null");
    ZG_REQUIRE(n_rows == batch, ZG_ERR_ARG, "debug_sample_rows_each: %zu rows for a batch of %zu", n_rows, batch);
    ZG_REQUIRE(!edits || edits->min_p == 0.0f, ZG_ERR_ARG, "debug_sample_rows_each: edits->min_p %f beside rows (min-p is the row's)", edits->min_p);
    return debug_sample_rows(logits, batch, vocab, nullptr, rows, edits, uniforms, edited_out, tokens_out, probs_out, thresholds_out, "debug_sample_rows_each");
}

// The guide's two kernels on the caller's rows (tests): the mask — with the edit stage's part in the same launch when
// the edits carry a list —, then the advance on the caller's picks.  Every row stands at a picked column (no control block).
// Allocates per call.
int zg_debug_guide_rows(const float* logits, size_t batch, size_t vocab, const zg_guide* guide, const size_t* states, const zg_logit_edits* edits,
                        const size_t* picks, float* edited_out, float* part_val_out, int32_t* part_idx_out, size_t* next_states_out) {
    ZG_TRY(require_init());
    const char* who = "debug_guide_rows";
    ZG_REQUIRE(logits && states && picks && edited_out && part_val_out && part_idx_out && next_states_out && batch >= 1 && batch <= 64 && vocab >= 1 &&
                   vocab <= (size_t)64 * 4096,
               ZG_ERR_ARG, "%s: bad argument", who);
    ZG_REQUIRE(!edits || edits->min_p == 0.0f, ZG_ERR_ARG, "%s: edits->min_p %f (the lists only)", who, edits->min_p);
    const size_t words = guide_keep_words(vocab);
    std::vector<unsigned> h_keep((size_t)ZG_GUIDE_MAX_STATES * words);
    ZG_TRY(build_guide(guide, vocab, who, h_keep.data()));
    std::vector<char> block(edits ? edit_block_bytes(vocab) : 0);
    bool stage_on = false, any = false;
    if (edits) ZG_TRY(build_edits(edits, vocab, who, block.data(), &stage_on));
    std::vector<int> h_state(batch), h_pick(batch);
    ZG_TRY(check_guide_call(h_keep.data(), guide->n_states, vocab, stage_on ? reinterpret_cast<const unsigned*>(block.data() + sizeof(EditTable)) : nullptr,
                            states, batch, false, who, h_state.data(), &any));
    for (size_t b = 0; b < batch; ++b) h_pick[b] = (int)std::min(picks[b], (size_t)INT_MAX);
    const int B = (int)batch, V = (int)vocab, n_part = std::min(64, (V + 255) / 256), n_states = (int)guide->n_states;
    hipStream_t s = ctx().stream;
    DevScratch ds;
    float *d_logits, *d_val;
    int *d_idx, *d_n, *d_state, *d_pick;
    unsigned short* d_next;
    unsigned* d_keep;
    char* d_edit;
    ZG_TRY(ds.carve([&] {
        d_logits = ds.take<float>(batch * vocab * 4);
        d_val = ds.take<float>(batch * n_part * 4);
        d_idx = ds.take<int>(batch * n_part * 4);
        d_next = ds.take<unsigned short>((size_t)n_states * vocab * 2);
        d_keep = ds.take<unsigned>((size_t)n_states * words * 4);
        d_n = ds.take<int>(4);
        d_state = ds.take<int>(batch * 4);
        d_pick = ds.take<int>(batch * 4);
        d_edit = ds.take<char>(block.size());
    }));
    ZG_HIP(hipMemcpyAsync(d_logits, logits, batch * vocab * 4, hipMemcpyDefault, s));
    ZG_HIP(hipMemcpyAsync(d_next, guide->next, (size_t)n_states * vocab * 2, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_keep, h_keep.data(), (size_t)n_states * words * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_n, &n_states, 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_state, h_state.data(), batch * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_pick, h_pick.data(), batch * 4, hipMemcpyHostToDevice, s));
    if (stage_on) ZG_HIP(hipMemcpyAsync(d_edit, block.data(), block.size(), hipMemcpyHostToDevice, s));
    SamplerChain c{};
    c.logits = d_logits, c.batch = B, c.vocab = V, c.part_val = d_val, c.part_idx = d_idx, c.n_part = n_part;
    c.edit_tab = reinterpret_cast<const EditTable*>(d_edit);
    c.edit_keep = reinterpret_cast<const unsigned*>(d_edit + sizeof(EditTable));
    c.guide = GuideArgs{d_next, d_keep, d_n, d_state, nullptr, 0, nullptr, nullptr};
    ZG_TRY(emit_sampler_chain(c, StepTail{GREEDY, false, false, false, stage_on, true}, s));  // (the row stage alone: no sampler)
    ZG_HIP(hipMemcpyAsync(edited_out, d_logits, batch * vocab * 4, hipMemcpyDefault, s));
    ZG_HIP(hipMemcpyAsync(part_val_out, d_val, batch * n_part * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipMemcpyAsync(part_idx_out, d_idx, batch * n_part * 4, hipMemcpyDeviceToHost, s));
    ZG_TRY(launch_guide_advance(c.guide, d_pick, B, V, s));
    ZG_HIP(hipMemcpyAsync(h_state.data(), d_state, batch * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipStreamSynchronize(s));
    for (size_t b = 0; b < batch; ++b) next_states_out[b] = h_state[b] < 0 ? ZG_GUIDE_NONE : (size_t)h_state[b];
    return ZG_OK;
}

// The ban stage on the caller's rows (tests): the ban launch, then the rebuild of the partials or — edits with a list
// given — the edit launch, which rebuilds them itself.  The history is the caller's, in order, a token outside the vocabulary
// included (it must match nothing); `picked` says where each row stands (no control block).  The rules are checked as a call's are,
// except for the bound that keeps a row from being emptied: a harness row may be left all -inf.  Allocates per call.
int zg_debug_ban_rows(const float* logits, size_t batch, size_t vocab, const zg_ban_rules* bans, const size_t* history, size_t history_stride,
                      const size_t* history_lens, const int64_t* picked, const zg_logit_edits* edits, float* edited_out, float* part_val_out,
                      int32_t* part_idx_out) {
    ZG_TRY(require_init());
    const char* who = "debug_ban_rows";
    ZG_REQUIRE(logits && bans && history_lens && picked && edited_out && part_val_out && part_idx_out && batch >= 1 && batch <= (size_t)kBanMaxRows && vocab >= 1 &&
                   vocab <= (size_t)64 * 4096,
               ZG_ERR_ARG, "%s: bad argument", who);
    ZG_REQUIRE(!edits || edits->min_p == 0.0f, ZG_ERR_ARG, "%s: edits->min_p %f (the lists only)", who, edits->min_p);
    size_t longest = 0;
    for (size_t b = 0; b < batch; ++b) {
        ZG_REQUIRE(history_lens[b] <= history_stride && (history_lens[b] == 0 || history), ZG_ERR_SHAPE, "%s: row %zu lists %zu tokens (stride %zu)", who, b,
                   history_lens[b], history_stride);
        longest = std::max(longest, history_lens[b]);
    }
    ZG_REQUIRE(longest <= (size_t)kPenMaxHistory, ZG_ERR_UNSUPPORTED, "%s: a history of %zu tokens exceeds the %d the LDS holds", who, longest, kPenMaxHistory);
    std::vector<char> block(edits ? edit_block_bytes(vocab) : 0);
    bool stage_on = false, on = false;
    if (edits) ZG_TRY(build_edits(edits, vocab, who, block.data(), &stage_on));
    ZG_TRY(check_bans(bans, batch, vocab, longest, (size_t)-1, 0, nullptr, false, false, who, &on));
    std::vector<BanRules> rules(1);
    fill_bans(rules.data(), *bans, batch, 0);
    const int B = (int)batch, V = (int)vocab, n_part = std::min(64, (V + 255) / 256);
    const size_t stride = std::max(longest, (size_t)1);
    std::vector<int> h_hist(batch * stride, 0), h_len(batch), h_picked(batch);
    for (size_t b = 0; b < batch; ++b) {
        h_len[b] = (int)history_lens[b];
        h_picked[b] = (int)std::min<int64_t>(std::max<int64_t>(picked[b], -1), INT_MAX);
        for (size_t i = 0; i < history_lens[b]; ++i) h_hist[b * stride + i] = (int)std::min(history[b * history_stride + i], (size_t)INT_MAX);
    }
    hipStream_t s = ctx().stream;
    DevScratch ds;
    float *d_logits, *d_val;
    int *d_idx, *d_hist, *d_len, *d_picked;
    BanRules* d_rules;
    char* d_edit;
    ZG_TRY(ds.carve([&] {
        d_logits = ds.take<float>(batch * vocab * 4);
        d_val = ds.take<float>(batch * n_part * 4);
        d_idx = ds.take<int>(batch * n_part * 4);
        d_hist = ds.take<int>(batch * stride * 4);
        d_len = ds.take<int>(batch * 4);
        d_picked = ds.take<int>(batch * 4);
        d_rules = ds.take<BanRules>(sizeof(BanRules));
        d_edit = ds.take<char>(block.size());
    }));
    ZG_HIP(hipMemcpyAsync(d_logits, logits, batch * vocab * 4, hipMemcpyDefault, s));
    ZG_HIP(hipMemcpyAsync(d_hist, h_hist.data(), batch * stride * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_len, h_len.data(), batch * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_picked, h_picked.data(), batch * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_rules, rules.data(), sizeof(BanRules), hipMemcpyHostToDevice, s));
    if (stage_on) ZG_HIP(hipMemcpyAsync(d_edit, block.data(), block.size(), hipMemcpyHostToDevice, s));
    SamplerChain c{};
    c.logits = d_logits, c.batch = B, c.vocab = V, c.part_val = d_val, c.part_idx = d_idx, c.n_part = n_part;
    c.edit_tab = reinterpret_cast<const EditTable*>(d_edit);
    c.edit_keep = reinterpret_cast<const unsigned*>(d_edit + sizeof(EditTable));
    c.hist.prior = d_hist, c.hist.prior_len = d_len, c.hist.prior_stride = (int)stride, c.hist.max_hist = (int)longest;
    c.ban = BanArgs{d_rules, nullptr, d_picked};
    ZG_TRY(emit_sampler_chain(c, StepTail{GREEDY, false, false, false, stage_on, false, true}, s));  // (the row stages alone: no sampler)
    ZG_HIP(hipMemcpyAsync(edited_out, d_logits, batch * vocab * 4, hipMemcpyDefault, s));
    ZG_HIP(hipMemcpyAsync(part_val_out, d_val, batch * n_part * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipMemcpyAsync(part_idx_out, d_idx, batch * n_part * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipStreamSynchronize(s));
    return ZG_OK;
}

// The penalty kernels on the caller's rows (tests): the launches of the penalised step, in place on a copy — the body of
// zg_debug_penalize_rows (pen: the same for every row) and of zg_debug_penalize_rows_each (each: the row's own).  Allocates per call.
static int debug_penalize_rows(const float* logits, size_t batch, size_t vocab, const zg_logit_penalties* pen, const zg_row_sampling* each,
                               const size_t* history, size_t history_stride, const size_t* history_lens, float* logits_out, unsigned* counts_out) {
    ZG_REQUIRE(logits && logits_out && history_lens && batch >= 1 && batch <= 64 && vocab >= 1 && vocab <= (size_t)64 * 4096, ZG_ERR_ARG,
               "debug_penalize_rows: bad argument");
    size_t longest = 0;
    for (size_t b = 0; b < batch; ++b) {
        ZG_REQUIRE(history_lens[b] <= history_stride && (history_lens[b] == 0 || history), ZG_ERR_SHAPE, "debug_penalize_rows: row %zu lists %zu tokens (stride %zu)",
                   b, history_lens[b], history_stride);
        for (size_t i = 0; i < history_lens[b]; ++i)
            ZG_REQUIRE(history[b * history_stride + i] < vocab, ZG_ERR_SHAPE, "debug_penalize_rows: token %zu >= vocab %zu", history[b * history_stride + i],
                       vocab);
        longest = std::max(longest, history_lens[b]);
    }
    ZG_REQUIRE(longest <= (size_t)kPenMaxHistory, ZG_ERR_UNSUPPORTED, "debug_penalize_rows: a history of %zu tokens exceeds the %d the LDS table holds", longest,
               kPenMaxHistory);
    const int B = (int)batch, V = (int)vocab, n_part = std::min(64, (V + 255) / 256);
    const size_t stride = std::max(longest, (size_t)1);
    hipStream_t s = ctx().stream;
    DevScratch ds;
    float* d_logits;
    unsigned* d_counts;
    int *d_hist, *d_len;
    PenParams* d_par;
    SamplerChain c{};  // the penalty stage alone, with the counts
    c.batch = B, c.vocab = V, c.n_part = n_part;
    ZG_TRY(ds.carve([&] {
        c.logits = d_logits = ds.take<float>(batch * vocab * 4);
        c.counts = d_counts = ds.take<unsigned>(batch * vocab * 4);
        d_hist = ds.take<int>(batch * stride * 4);
        c.part_val = ds.take<float>((size_t)B * n_part * 4);
        c.part_idx = ds.take<int>((size_t)B * n_part * 4);
        d_len = ds.take<int>(batch * 4);
        c.pen = d_par = ds.take<PenParams>(batch * sizeof(PenParams));
    }));
    std::vector<int> h_hist(batch * stride, 0), h_len(batch);
    for (size_t b = 0; b < batch; ++b) {
        h_len[b] = (int)history_lens[b];
        for (size_t i = 0; i < history_lens[b]; ++i) h_hist[b * stride + i] = (int)history[b * history_stride + i];
    }
    std::vector<PenParams> hp(batch);
    for (size_t b = 0; b < batch; ++b) {
        const zg_logit_penalties& p = each ? each[b].penalties : *pen;
        hp[b] = PenParams{p.repetition, p.presence, p.frequency, 0};
    }
    ZG_HIP(hipMemcpyAsync(d_logits, logits, batch * vocab * 4, hipMemcpyDefault, s));
    ZG_HIP(hipMemsetAsync(d_counts, 0, batch * vocab * 4, s));
    ZG_HIP(hipMemcpyAsync(d_hist, h_hist.data(), batch * stride * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_len, h_len.data(), batch * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_par, hp.data(), batch * sizeof(PenParams), hipMemcpyHostToDevice, s));
    c.hist.prior = d_hist;
    c.hist.prior_len = d_len;
    c.hist.prior_stride = (int)stride;
    c.hist.max_hist = (int)longest;
    ZG_TRY(emit_sampler_chain(c, StepTail{GREEDY, true}, s));
    // all penalties off: the call is the identity on the rows (the counts are still the history's); per row, the kernel leaves such
    // a row alone itself
    ZG_HIP(hipMemcpyAsync(logits_out, pen && penalties_off(*pen) ? logits : d_logits, batch * vocab * 4, hipMemcpyDefault, s));
    if (counts_out) ZG_HIP(hipMemcpyAsync(counts_out, d_counts, batch * vocab * 4, hipMemcpyDefault, s));
    ZG_HIP(hipStreamSynchronize(s));
    return ZG_OK;
}

int zg_debug_penalize_rows(const float* logits, size_t batch, size_t vocab, const zg_logit_penalties* pen, const size_t* history, size_t history_stride,
                           const size_t* history_lens, float* logits_out, unsigned* counts_out) {
    ZG_TRY(require_init());
    ZG_TRY(check_penalties(pen, "debug_penalize_rows"));
    return debug_penalize_rows(logits, batch, vocab, pen, nullptr, history, history_stride, history_lens, logits_out, counts_out);
}

int zg_debug_penalize_rows_each(const float* logits, size_t batch, size_t vocab, const zg_row_sampling* rows, size_t n_rows, const size_t* history,
                                size_t history_stride, const size_t* history_lens, float* logits_out, unsigned* counts_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(rows != nullptr, ZG_ERR_ARG, "debug_penalize_rows_each: rows is null");
    ZG_REQUIRE(n_rows == batch && batch <= 64, ZG_ERR_ARG, "debug_penalize_rows_each: %zu rows for a batch of %zu (<= 64)", n_rows, batch);
    StepTail plan;
    ZG_TRY(plan_rows(rows, n_rows, vocab ? vocab : 1, 0, "debug_penalize_rows_each", nullptr, nullptr, nullptr, &plan));
    return debug_penalize_rows(logits, batch, vocab, nullptr, rows, history, history_stride, history_lens, logits_out, counts_out);
}

int zg_gpt_profile_step(zg_gpt* g, size_t seq_len, int iters, float* us_out, size_t n_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && us_out && n_out >= 8 && iters > 0, ZG_ERR_ARG, "profile_step: bad argument");
    ZG_REQUIRE(seq_len >= 1 && seq_len + (size_t)iters - 1 <= g->cfg.context_size, ZG_ERR_SHAPE,
               "profile_step: positions %zu..%zu outside the context", seq_len, seq_len + iters - 1);
    hipStream_t s = gs(g);
    ZG_HIP(hipStreamSynchronize(s));
    ZG_TRY(ensure_ln_folded(g, s));
    g->hidden.src = HID_X;  // (steps ran: x is what they left)
    ZG_TRY(note_steps(g, (size_t)iters, s));
    for (size_t b = 0; b < g->batch; ++b) g->h_ints[b] = (int)(b % g->cfg.vocab_size);
    ZG_HIP(hipMemcpyAsync(g->forced, g->h_ints, g->batch * sizeof(int), hipMemcpyHostToDevice, s));
    ZG_TRY(stage_ctrl(g, seq_len - 1, seq_len, 1, s));
    static StepProf prof;  // events are created on first use and reused
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // All iterations are enqueued before the single synchronisation so that the queue stays ahead of
    // the GPU (an interval then is kernel + launch boundary, not kernel + host launch latency).
    prof.n = 0;
    StepOpts timed;
    timed.prof = &prof;
    double null_us = 0.0;
    for (int it = 0; it < iters; ++it) {
        ZG_TRY(enqueue_step(g, true, bucket_t_hi(g, seq_len + it), s, timed));  // eager; the embed kernel advances the position
        // calibration: a one-element copy recorded the same way = launch boundary + event overhead
        ZG_TRY(launch_copy_f32(g->q, g->q + 4, 1, s));
        ZG_TRY(prof_mark(&prof, 8, s));
    }
    ZG_HIP(hipStreamSynchronize(s));
    for (size_t i = 1; i < prof.n; ++i) {
        if (prof.cls[i] < 0) continue;  // interval between two steps
        float ms = 0.0f;
        ZG_HIP(hipEventElapsedTime(&ms, prof.ev[i - 1], prof.ev[i]));
        if (prof.cls[i] == 8) {
            null_us += ms * 1000.0;
            continue;
        }
        acc[prof.cls[i]] += ms * 1000.0;
        acc[7] += ms * 1000.0;
    }
    for (int i = 0; i < 8; ++i) us_out[i] = (float)(acc[i] / iters);
    if (n_out >= 9) us_out[8] = (float)(null_us / iters);
    return check_fault(g);  // (every event above was synchronised: timings of a faulted step are not reported)
}

int zg_gpt_time_kernel(zg_gpt* g, int which_and_options, int iters, float* avg_us, size_t* algorithmic_bytes) {
    ZG_TRY(require_init());
    const int which = which_and_options & 0xff;
    const bool cycle = (which_and_options & ZG_TIME_WALK_LAYERS) != 0;  // walk the layers, so that no launch finds its weights in the L2s
    const size_t t_opt = (size_t)((unsigned)which_and_options >> 16);    // another position for the attention kernel (0: mid-context)
    // (ZG_TIME_AT(t) occupies bits 16..30: t up to 32767 — every GPT-2 context; a larger t would set the sign bit)
    ZG_REQUIRE(g && avg_us && iters > 0 && which_and_options >= 0 && which <= 6, ZG_ERR_ARG, "time_kernel: bad argument (ZG_TIME_AT takes t < 32768)");
    hipStream_t s = gs(g);
    ZG_REQUIRE(s != nullptr, ZG_ERR_UNSUPPORTED, "time_kernel needs a capturable stream");
    const size_t E = g->cfg.n_embed, wb = g->wbytes;
    const size_t bytes_tab[7] = {0, 3 * E * E * wb, 0, E * E * wb, 4 * E * E * wb, 4 * E * E * wb, g->cfg.vocab_size * E * wb};
    // control block: a mid-context position so that the attention kernel has work
    size_t T = g->cfg.context_size / 2 > 0 ? g->cfg.context_size / 2 : 1;
    if (t_opt >= 1 && t_opt <= g->cfg.context_size) T = t_opt;
    ZG_HIP(hipStreamSynchronize(s));
    ZG_TRY(ensure_ln_folded(g, s));
    g->hidden.src = HID_X;
    const int chain = 64, reps = (iters + chain - 1) / chain;
    // one epoch per replay of the chain, warm-up included — and class 0 IS the embed kernel, which advances the epoch itself at
    // every one of the chain's launches
    ZG_TRY(note_steps(g, (size_t)(reps + 1) * (which == 0 ? (size_t)chain : 1), s));
    ZG_TRY(stage_ctrl(g, T - 1, T, 1, s));
    hipGraphExec_t exec = nullptr;
    ZG_TRY(capture_graph(s, &exec, [&] {
        // tagged hand-overs: a new epoch per replay and a launch id per chain position, so that every merging split / slice
        // waits for ITS writers as in a real step (one more tiny launch per 64)
        int st = ZG_OK;
        if ((g->modes.tags || g->modes.fused) && which != 0) st = launch_epoch_bump(g->hand.epoch, s);
        StepOpts o;
        o.only = which;
        for (int i = 0; i < chain && st == ZG_OK; ++i) {
            o.only_layer = cycle ? (size_t)i % g->cfg.n_layer : 0;
            o.salt = i;
            st = enqueue_step(g, true, bucket_t_hi(g, T), s, o);
        }
        return st;
    }));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0.0f;
    const int st = [&]() -> int {
        ZG_HIP(hipEventCreate(&e0));
        ZG_HIP(hipEventCreate(&e1));
        ZG_HIP(hipGraphLaunch(exec, s));
        ZG_HIP(hipStreamSynchronize(s));
        ZG_HIP(hipEventRecord(e0, s));
        for (int r = 0; r < reps; ++r) ZG_HIP(hipGraphLaunch(exec, s));
        ZG_HIP(hipEventRecord(e1, s));
        ZG_HIP(hipEventSynchronize(e1));
        ZG_HIP(hipEventElapsedTime(&ms, e0, e1));
        return ZG_OK;
    }();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipGraphExecDestroy(exec);
    ZG_TRY(st);
    *avg_us = ms * 1000.0f / (float)(reps * chain);
    if (algorithmic_bytes) *algorithmic_bytes = bytes_tab[which];
    return check_fault(g);
}

// A handle's age (tests; include/zgpt2.h): n_steps steps that wrote no tagged slot, counted by the production rule and added to
// the device epoch on the stream; the stream-K epoch on request.
int zg_debug_gpt_age(zg_gpt* g, size_t n_steps, int set_sk_epoch, unsigned sk_epoch) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g, ZG_ERR_ARG, "debug_gpt_age: null argument");
    if (set_sk_epoch) g->pass.sk_epoch = sk_epoch;
    if (!g->modes.tags && !g->modes.fused) return ZG_OK;
    hipStream_t s = gs(g);
    ZG_TRY(note_steps(g, n_steps, s));
    return launch_epoch_add(g->hand.epoch, (unsigned)n_steps, s);
}

int zg_debug_gpt_age_state(zg_gpt* g, unsigned long long* out, size_t n_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && out && n_out >= ZG_AGE_STATE_WORDS, ZG_ERR_ARG, "debug_gpt_age_state: need %d words", ZG_AGE_STATE_WORDS);
    ZG_HIP(hipStreamSynchronize(gs(g)));
    unsigned epoch = 0;
    ZG_HIP(hipMemcpy(&epoch, g->hand.epoch, sizeof(unsigned), hipMemcpyDeviceToHost));
    out[0] = epoch;
    out[1] = g->hand.epochs_since_clear;
    out[2] = g->hand.steps_counted;
    out[3] = g->hand.tag_clears;
    out[4] = g->pass.sk_epoch;
    out[5] = g->pass.sk_restarts;
    return ZG_OK;
}

int zg_debug_gpt_tag_census(zg_gpt* g, unsigned epoch24, unsigned sk_flag_value, size_t* counts, size_t n_counts) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && counts && n_counts >= 4 && epoch24 < (1u << 24), ZG_ERR_ARG, "debug_gpt_tag_census: need 4 counts and a 24-bit epoch");
    ZG_HIP(hipStreamSynchronize(gs(g)));
    const unsigned long long* const words[3] = {g->hand.sk_tag, g->hand.part_tag, g->hand.qkv_tag};
    const size_t bytes[3] = {g->hand.sk_tag_bytes, g->hand.part_tag_bytes, g->hand.qkv_tag_bytes};
    std::vector<unsigned long long> h;
    for (int i = 0; i < 3; ++i) {
        h.resize(bytes[i] / 8);
        ZG_HIP(hipMemcpy(h.data(), words[i], bytes[i], hipMemcpyDeviceToHost));
        counts[i] = 0;
        for (const unsigned long long w : h) {  // (value, tag): the tag is the upper word, epoch << 8 | launch id
            const unsigned tag = (unsigned)(w >> 32);
            if ((tag & 0xffu) != 0u && (tag >> 8) == epoch24) ++counts[i];
        }
    }
    counts[3] = 0;
    if (g->pass.sk_flags != nullptr) {
        unsigned f[kSkFlagWords];
        ZG_HIP(hipMemcpy(f, g->pass.sk_flags, sizeof(f), hipMemcpyDeviceToHost));
        for (const unsigned w : f) counts[3] += w == sk_flag_value;
    }
    return ZG_OK;
}

// The raw cache bytes of one row (tests of zg_gpt_kv_fork; include/zgpt2.h): [H][n_pos][64] elements in storage format, then, for a
// 24-bit cache, the byte plane [H][n_pos][64].  Drains the stream.
int zg_debug_gpt_kv_rows(zg_gpt* g, size_t layer, int which, size_t row, size_t first_pos, size_t n_pos, void* out, size_t out_bytes) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && out && (which == 0 || which == 1), ZG_ERR_ARG, "debug_gpt_kv_rows: bad argument");
    const size_t C = g->cfg.context_size, H = g->cfg.n_heads, E = g->cfg.n_embed, B = g->batch;
    ZG_REQUIRE(layer < g->cfg.n_layer && row < B && n_pos >= 1 && first_pos < C && n_pos <= C - first_pos, ZG_ERR_SHAPE,
               "debug_gpt_kv_rows: layer %zu, row %zu, positions %zu + %zu", layer, row, first_pos, n_pos);
    const size_t eb = g->kv_mode == 0 ? 4 : 2, need = H * n_pos * 64 * (eb + (g->kv_mode == 2 ? 1 : 0));
    ZG_REQUIRE(out_bytes >= need, ZG_ERR_SHAPE, "debug_gpt_kv_rows: %zu bytes for %zu", out_bytes, need);
    hipStream_t s = gs(g);
    const char* p = reinterpret_cast<const char*>(which ? g->layers[layer].v_cache : g->layers[layer].k_cache);
    const size_t at = (row * H * C + first_pos) * 64;  // elements; a head's strip is C * 64 of them
    ZG_HIP(hipMemcpy2DAsync(out, n_pos * 64 * eb, p + at * eb, C * 64 * eb, n_pos * 64 * eb, H, hipMemcpyDeviceToHost, s));
    if (g->kv_mode == 2)
        ZG_HIP(hipMemcpy2DAsync(reinterpret_cast<char*>(out) + H * n_pos * 64 * 2, n_pos * 64, p + B * C * E * 2 + at, C * 64, n_pos * 64, H,
                                hipMemcpyDeviceToHost, s));
    ZG_HIP(hipStreamSynchronize(s));
    return ZG_OK;
}

int zg_debug_prefetch_stats(zg_gpt* g, unsigned* out, size_t n_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && out && n_out >= 25, ZG_ERR_ARG, "prefetch_stats: need 25 words");
    memset(out, 0, n_out * sizeof(unsigned));
    out[0] = g->prefetch.on ? (g->prefetch.stalled ? 2u : 1u) : 0u;
    if (!g->prefetch.on) return ZG_OK;
    ZG_HIP(hipStreamSynchronize(gs(g)));
    ZG_HIP(hipStreamSynchronize(g->prefetch.stream));
    PfCtl h;
    ZG_HIP(hipMemcpy(&h, g->prefetch.ctl, sizeof(PfCtl), hipMemcpyDeviceToHost));
    for (int x = 0; x < 8; ++x) {
        out[1 + x] = h.ticket[x];
        out[9 + x] = h.exit_reason[x];
        out[17 + x] = h.jobs_done[x];
    }
    for (size_t i = 0; i < 256 && 25 + i < n_out; ++i) out[25 + i] = h.xcd_log[i];  // diagnostic (-DZG_STAMPS) builds only
    return ZG_OK;
}

#ifdef ZG_STAMPS
// Diagnostic build only: (re)arm the timestamp buffer / read it back (count, then 10 words per record).
int zg_debug_stamps_begin(void) {
    ZG_TRY(require_init());
    Ctx& c = ctx();
    const size_t bytes = (16 + 10 * 4096) * sizeof(unsigned long long);
    if (!c.dbg) ZG_HIP(hipMalloc(reinterpret_cast<void**>(&c.dbg), bytes));
    ZG_HIP(hipMemset(c.dbg, 0, bytes));
    return ZG_OK;
}
int zg_debug_stamps_read(unsigned long long* out, size_t n_words) {
    ZG_TRY(require_init());
    ZG_HIP(hipDeviceSynchronize());
    ZG_HIP(hipMemcpy(out, ctx().dbg, n_words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return ZG_OK;
}
#endif

}  // extern "C"
