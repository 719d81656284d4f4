// api_gpt.hip — model tier of the C ABI: GPTConfig/State/Block/GPT/generate of the reference's
// src/main.zig as one device-resident object.  Weights, per-sequence KV caches and all scratch
// live in a single arena allocated by zg_gpt_create (the State.init / load_gpt moment of the
// reference); a decode step is a fixed chain of kernels captured once into a hipGraph whose
// position, tokens and argmax all live in device memory, so a whole greedy generation is enqueued
// without a host round trip per token.  The other units of the tier (api_gpt.h lists them) work on this object.
//
// HBM layout (one hipMalloc, 256-B aligned sub-buffers):
//   [ weights: wte | wpe | ln_f | per layer: c_attn_w c_proj_w c_fc_w mlp_proj_w + fp32 vectors ]
//   [ KV cache: layer x {K,V} x batch x head x ctx x 64 ]   head-major: one head's keys are one
//                                                            contiguous [ctx, 64] slab, so no
//                                                            per-step transpose (ops.zig:153,158)
//   [ scratch: x q h4 attention partials logits argmax partials, control block, token buffers ]
#include <string.h>

#include <algorithm>

#include "api_gpt.h"

using namespace zg;

namespace {  // this unit only

size_t kv_elem_bytes(const zg_gpt* g) { return g->kv_mode == 1 ? 2 : g->kv_mode == 2 ? 3 : 4; }  // B24: a bf16 plane, then a byte plane

// One pass computes sizes (both bases nullptr) or assigns pointers: the weight region from wbase (the handle's own arena or the
// one it borrows), everything else — KV caches, scratch, control — from sbase.
void carve(zg_gpt* g, char* wbase, char* sbase) {
    const zg_gpt_config& c = g->cfg;
    const size_t E = c.n_embed, V = c.vocab_size, C = c.context_size, L = c.n_layer, B = g->batch;
    const size_t wb = g->wbytes, kvb = kv_elem_bytes(g);
    Carver cv;
    char* base = wbase;
    auto P = [&](size_t bytes) -> char* {
        const size_t o = cv.take(bytes);
        return base ? base + o : nullptr;
    };
    g->wte = P(V * E * wb);
    g->wpe = P(C * E * wb);
    g->ln_f_g = (float*)P(E * 4);
    g->ln_f_b = (float*)P(E * 4);
    g->lm_c2 = (float*)P(V * 4);
    g->lm_c3 = (float*)P(V * 4);
    g->layers.resize(L);
    for (size_t l = 0; l < L; ++l) {
        zg_layer& y = g->layers[l];
        y.c_attn_w = P(3 * E * E * wb);
        y.c_proj_w = P(E * E * wb);
        y.c_fc_w = P(4 * E * E * wb);
        y.mlp_proj_w = P(4 * E * E * wb);
        y.ln_1_g = (float*)P(E * 4);
        y.ln_1_b = (float*)P(E * 4);
        y.c_attn_b = (float*)P(3 * E * 4);
        y.c_proj_b = (float*)P(E * 4);
        y.ln_2_g = (float*)P(E * 4);
        y.ln_2_b = (float*)P(E * 4);
        y.c_fc_b = (float*)P(4 * E * 4);
        y.mlp_proj_b = (float*)P(E * 4);
        y.c_attn_c2 = (float*)P(3 * E * 4);
        y.c_attn_c3 = (float*)P(3 * E * 4);
        y.c_fc_c2 = (float*)P(4 * E * 4);
        y.c_fc_c3 = (float*)P(4 * E * 4);
        y.c_attn_p = y.c_proj_p = y.c_fc_p = y.mlp_proj_p = nullptr;
        if (g->wt != WT_BF16 && !(g->flags & ZG_GPT_NO_PREFILL)) {  // inside the weight region: broadcast with the weights
            y.c_attn_p = (bf16_t*)P(3 * E * E * kSplit * 2);
            y.c_proj_p = (bf16_t*)P(E * E * kSplit * 2);
            y.c_fc_p = (bf16_t*)P(4 * E * E * kSplit * 2);
            y.mlp_proj_p = (bf16_t*)P(4 * E * E * kSplit * 2);
        }
    }
    g->weight_region_bytes = (cv.off + 255) & ~(size_t)255;
    cv = Carver{};
    base = sbase;
    for (size_t l = 0; l < L; ++l) {
        g->layers[l].k_cache = P(B * C * E * kvb);
        g->layers[l].v_cache = P(B * C * E * kvb);
    }
    g->ctrl = (StepCtrl*)P(sizeof(StepCtrl));
    g->kv_region_bytes = L ? (size_t)(reinterpret_cast<char*>(g->ctrl) - reinterpret_cast<char*>(g->layers[0].k_cache)) : 0;
    g->x = (float*)P(B * E * 4);
    g->q = (float*)P(B * E * 4);
    g->h4 = (float*)P(B * 4 * E * 4);
    g->part = (float*)P(B * c.n_heads * g->max_splits * kPartStride * 4);
    g->logits = (float*)P(B * V * 4);
    g->part_val = (float*)P(B * 4096 * 4);
    g->part_idx = (int*)P(B * 4096 * 4);
    g->prompt = (int*)P(B * C * 4);
    g->prompt_len = (int*)P(B * 4);
    g->forced = (int*)P(B * 4);
    g->cur_token = (int*)P(B * 4);
    g->out_tokens = (int*)P(B * C * 4);
    g->samp.sampled = (int*)P(B * 4);
    g->samp.params = (SampleParams*)P(kRowsMax * sizeof(SampleParams));
    g->samp.ws = (float*)P(sample_workspace_floats((int)B) * 4);
    g->samp.filt = filter_workspace(P(filter_workspace_bytes((int)B)), (int)B);
    g->pen.prior = (int*)P(B * C * 4);
    g->pen.prior_len = (int*)P(B * 4);
    g->pen.params = (PenParams*)P(kRowsMax * sizeof(PenParams));
    g->xp = (bf16_t*)P(E * 48);
    g->hp = (bf16_t*)P(4 * E * 48);
    g->ap = (bf16_t*)P(E * 48);
    g->attn_cnt = (int*)P(8 * c.n_heads * 4);
    g->hand.epoch = (unsigned*)P(256);
    g->xst = (float*)P(((E + 15) / 16) * 8 * 2 * 4);
    g->hand.sk_tag_bytes = ((E + 15) / 16) * 4 * 128 * 8;
    g->hand.part_tag_bytes = 8 * c.n_heads * g->max_splits * kPartStride * 8;
    g->hand.sk_tag = (unsigned long long*)P(g->hand.sk_tag_bytes);
    g->hand.qkv_tag_bytes = 3 * E * 8;
    g->hand.qkv_tag = (unsigned long long*)P(g->hand.qkv_tag_bytes);
    g->hand.part_tag = (unsigned long long*)P(g->hand.part_tag_bytes);
    g->sk_tiles = (int)((E + 15) / 16);
    g->sk_ws = (float*)P((size_t)g->sk_tiles * 4 * 128 * 4);
    g->sk_cnt = (int*)P((size_t)g->sk_tiles * 4 * 4);  // [tile][4]: the four-wave plane-fed kernel takes one ticket per wave
    g->prefetch.njobs = (int)(2 + 5 * L);
    g->prefetch.ctl = (PfCtl*)P(sizeof(PfCtl));
    g->prefetch.jobs = (PfJob*)P((size_t)g->prefetch.njobs * sizeof(PfJob));
    g->pass.x = g->pass.qkv = g->pass.ws = nullptr;
    g->pass.sk_flags = nullptr;
    g->pass.sk_epoch = 0;
    g->pass.sk_restarts = 0;
    g->pass.sk_used = false;
    g->pass.a = g->pass.h = nullptr;
    g->pass.ws_floats = 0;
    if (!(g->flags & ZG_GPT_NO_PREFILL)) {
        g->pass.x = (float*)P(B * C * E * 4);
        g->pass.qkv = (float*)P(B * C * 3 * E * 4);
        g->pass.a = (bf16_t*)P(B * C * kSplit * E * 2);
        g->pass.h = (bf16_t*)P(B * C * kSplit * 4 * E * 2);
        // split-K partials of the prompt GEMMs; fp32 weights: three weight-plane passes of [B ctx, 4 E] at the least
        g->pass.ws_floats = g->wt == WT_BF16 ? (size_t)(16u << 20) : std::max((size_t)(16u << 20), 3 * B * C * 4 * E);
        g->pass.ws = (float*)P(g->pass.ws_floats * 4);
        g->pass.sk_flags = (unsigned*)P(kSkFlagWords * sizeof(unsigned));
    }
    // (behind everything else: handles that never ask for log-probabilities keep the layout they had)
    g->lp.ws = logprob_workspace(P(logprob_workspace_bytes((int)B, (int)V)), (int)B, (int)V);
    g->lp.top = (int*)P(256);
    g->lp.rec.logprob = (float*)P(B * C * 4);
    g->lp.rec.top_ids = (int*)P(B * C * ZG_LOGPROBS_TOP_MAX * 4);
    g->lp.rec.top_logprobs = (float*)P(B * C * ZG_LOGPROBS_TOP_MAX * 4);
    g->lp.rec.stride = (int)C;
    // (and behind those: handles that never ask for scoring keep the layout they had)
    g->score.logits = nullptr;
    g->score.ws = ScoreWs{};
    g->score.tail = g->score.planes = nullptr;
    g->score.gemm_ws = nullptr;
    g->score.gemm_ws_floats = 0;
    g->score.v64 = (V + 63) / 64 * 64;
    if ((g->flags & ZG_GPT_SCORE) && !(g->flags & ZG_GPT_NO_PREFILL)) {
        g->score.logits = (float*)P(kScoreRows * g->score.v64 * 4);
        g->score.ws = score_workspace(P(score_workspace_bytes((int)kScoreRows, (int)V)), (int)kScoreRows, (int)V);
        if (g->wt == WT_BF16) {
            if (V % 64) g->score.tail = (bf16_t*)P(64 * E * 2);
        } else {  // the three-pass GEMM sums its slabs [3][rows][score.v64] through a workspace: more than pass.ws holds at a real vocabulary
            g->score.planes = (bf16_t*)P(kSplit * g->score.v64 * E * 2);
            g->score.gemm_ws_floats = 3 * kScoreRows * g->score.v64;
            g->score.gemm_ws = (float*)P(g->score.gemm_ws_floats * 4);
        }
    }
    // (and behind everything: the stop stage's conditions and its two words per row; every layout above is what it was)
    g->stop.conds = (StopConds*)P(sizeof(StopConds));
    g->stop.fin = (int*)P(kStopMaxRows * 4);
    g->stop.reason = (int*)P(kStopMaxRows * 4);
    // (and the edit stage's bias table with the keep bitmap behind it)
    g->edit.tab = (EditTable*)P(edit_block_bytes(V));
    g->edit.keep = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(g->edit.tab) + sizeof(EditTable));
    // (and behind everything: the guide's table, bitmaps, states and record — handles without the flag keep the layout they had)
    g->guide.next = nullptr;
    g->guide.keep = nullptr;
    g->guide.n_states = g->guide.state = g->guide.rec = nullptr;
    if (g->flags & ZG_GPT_GUIDED_GENERATE) {
        g->guide.next = (unsigned short*)P((size_t)ZG_GUIDE_MAX_STATES * V * 2);
        g->guide.keep = (unsigned*)P((size_t)ZG_GUIDE_MAX_STATES * guide_keep_words(V) * 4);
        g->guide.n_states = (int*)P(256);
        g->guide.state = (int*)P(kRowsMax * 4);
        g->guide.rec = (int*)P(B * C * 4);
    }
    // (and behind that: the ban stage's rules, about 5 KB — no buffer above moves)
    g->ban.rules = (BanRules*)P(sizeof(BanRules));
    // (and behind that: the beam stage's state, its trace [batch][ctx] of parents and scores and the table lenpow — no buffer above moves)
    g->beam.state = (BeamState*)P(sizeof(BeamState));
    g->beam.parent = (int*)P(B * C * 4);
    g->beam.score = (float*)P(B * C * 4);
    g->beam.lenpow = (float*)P((C + 1) * 4);
    g->state_bytes = (cv.off + 255) & ~(size_t)255;
}

int upload_f32(const float* src, size_t n, void* dst, bool as_bf16, hipStream_t s) {
    // src may be host or device; matrices are converted on the device.
    Ctx& c = ctx();
    const float* dsrc = src;
    if (!is_device_ptr(src)) {
        if (!as_bf16) {
            ZG_HIP(hipMemcpyAsync(dst, src, n * 4, hipMemcpyHostToDevice, s));
            ZG_HIP(hipStreamSynchronize(s));
            return ZG_OK;
        }
        // chunk through the staging arena
        const size_t cap = c.stage.cap / 4;
        ZG_REQUIRE(cap > 0, ZG_ERR_STAGING, "no staging arena");
        for (size_t o = 0; o < n; o += cap) {
            const size_t m = (n - o < cap) ? (n - o) : cap;
            ZG_HIP(hipMemcpyAsync(c.stage.base, src + o, m * 4, hipMemcpyHostToDevice, s));
            ZG_TRY(launch_f32_to_bf16(reinterpret_cast<const float*>(c.stage.base), reinterpret_cast<bf16_t*>(dst) + o, m, s));
            ZG_HIP(hipStreamSynchronize(s));
        }
        return ZG_OK;
    }
    if (as_bf16) ZG_TRY(launch_f32_to_bf16(dsrc, reinterpret_cast<bf16_t*>(dst), n, s));
    else ZG_HIP(hipMemcpyAsync(dst, dsrc, n * 4, hipMemcpyDeviceToDevice, s));
    ZG_HIP(hipStreamSynchronize(s));
    return ZG_OK;
}

// A matrix of n = rows K fp32 elements (host or device) into B24 rows (zg_common.h b24_t), rounded on the device.  Whole rows at a
// time pass through the staging arena (also from device memory: the packer's 16-B loads then start aligned).  planes (optional):
// the plane-major split of the stored values for the whole-prompt GEMMs, made from the B24 matrix itself.
int upload_b24(const float* src, size_t n, size_t K, void* dst, bf16_t* planes, hipStream_t s) {
    Ctx& c = ctx();
    ZG_REQUIRE(K > 0 && K % 8 == 0 && n % K == 0 && K <= 65536, ZG_ERR_SHAPE, "B24 matrix: %zu elements in rows of %zu", n, K);
    const size_t rows = n / K, cap_rows = c.stage.cap / (4 * K);
    ZG_REQUIRE(cap_rows > 0, ZG_ERR_STAGING, "no staging arena for a %zu-float row", K);
    const hipMemcpyKind kind = is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    for (size_t r = 0; r < rows; r += cap_rows) {
        const size_t m = rows - r < cap_rows ? rows - r : cap_rows;
        ZG_HIP(hipMemcpyAsync(c.stage.base, src + r * K, m * K * 4, kind, s));
        ZG_TRY(launch_f32_to_b24(reinterpret_cast<const float*>(c.stage.base), m, (int)K, reinterpret_cast<char*>(dst) + r * 3 * K, s));
        ZG_HIP(hipStreamSynchronize(s));
    }
    if (planes) {
        ZG_TRY(launch_b24_split3(dst, rows, (int)K, planes, s));
        ZG_HIP(hipStreamSynchronize(s));
    }
    return ZG_OK;
}

// Everything a handle holds, also one that zg_gpt_create built only in part (new zg_gpt() zero-initialises): the only place
// that frees.
void release(zg_gpt* g) {
    (void)hipStreamSynchronize(gs(g));
    drop_prefetcher(g);
    drop_graphs(g);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    if (g->counted) --g->parent->n_children;
    if (g->arena) (void)hipFree(g->arena);
    if (g->h_ctrl) (void)hipHostFree(g->h_ctrl);
    if (g->h_ints) (void)hipHostFree(g->h_ints);
    if (g->lp.h_rec) (void)hipHostFree(g->lp.h_rec);
    if (g->stop.pinned) (void)hipHostFree(g->stop.pinned);
    if (g->edit.h_block) (void)hipHostFree(g->edit.h_block);
    if (g->ban.h_rules) (void)hipHostFree(g->ban.h_rules);
    delete g;
}

// zg_gpt_create behind the checks of its arguments: allocates, decides the decode modes, captures.  On failure the caller
// releases whatever g holds by then.
int build_handle(zg_gpt* g, const zg_gpt_options* opt) {
    const zg_gpt_config& c = g->cfg;
    const size_t batch = g->batch;
    zg_gpt* const parent = g->parent;
    carve(g, nullptr, nullptr);
    g->arena_bytes = (parent ? 0 : g->weight_region_bytes) + g->state_bytes;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&g->arena), g->arena_bytes);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(model arena)", __FILE__, __LINE__);
    g->wbase = parent ? parent->wbase : g->arena;
    char* const sbase = parent ? g->arena : g->arena + g->weight_region_bytes;
    carve(g, g->wbase, sbase);
    ZG_HIP(hipMemset(sbase, 0, g->state_bytes));  // (tags, counters and fault words start from zero)
    if (opt && opt->own_stream) {  // a private stream: its priority decides the hardware queue it shares (profiles/NOTEBOOK.md §5)
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);  // numerically: greatest <= 0 <= least
        const int pr = opt->stream_priority > 0 ? greatest : opt->stream_priority < 0 ? least : 0;
        e = hipStreamCreateWithPriority(&g->stream, hipStreamNonBlocking, pr);
        if (e != hipSuccess) return hip_fail(e, "hipStreamCreateWithPriority(handle stream)", __FILE__, __LINE__);
    }
    ZG_TRY(decide_step_modes(g));
    // (the control mirror and, in the same block, the fault word of the tagged hand-overs: pinned, written by the kernels)
    e = hipHostMalloc(reinterpret_cast<void**>(&g->h_ctrl), sizeof(PinnedCtrl), hipHostMallocDefault);
    // (h_ints, and behind it the staging of the penalties' prior / history: the same shape)
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&g->h_ints), 2 * (batch * c.context_size + batch) * sizeof(int), hipHostMallocDefault);
    // (the mirror of the log-probability record: a fetch copies its columns through it)
    if (e == hipSuccess)
        e = hipHostMalloc(reinterpret_cast<void**>(&g->lp.h_rec), batch * c.context_size * (1 + 2 * ZG_LOGPROBS_TOP_MAX) * sizeof(float), hipHostMallocDefault);
    // (the stop stage's block: a few hundred bytes, always there)
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&g->stop.pinned), sizeof(*g->stop.pinned), hipHostMallocDefault);
    // (the edit stage's mirror: the bias table and the keep bitmap)
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&g->edit.h_block), edit_block_bytes(c.vocab_size), hipHostMallocDefault);
    // (the ban stage's mirror: the rules of a call)
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&g->ban.h_rules), sizeof(BanRules), hipHostMallocDefault);
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc(control mirrors)", __FILE__, __LINE__);
    g->edit.build.assign(edit_block_bytes(c.vocab_size), 0);
    memset(g->stop.pinned, 0, sizeof(*g->stop.pinned));
    g->samp.h_params = g->h_ctrl->samp;
    g->hand.fault = &g->h_ctrl->fault;
    *g->hand.fault = 0;
    g->pen.h_params = g->h_ctrl->pen;
    g->pen.h_prior = g->h_ints + batch * c.context_size + batch;
    g->lp.h_top = &g->h_ctrl->top_n;
    g->guide.h_state = g->h_ctrl->guide_state;
    g->beam.h_state = &g->h_ctrl->beam;
    ZG_REQUIRE(!(g->flags & ZG_GPT_PENALIZED_GENERATE) || c.context_size <= (size_t)kPenMaxHistory, ZG_ERR_UNSUPPORTED,
               "ZG_GPT_PENALIZED_GENERATE: context_size %zu beyond the %d tokens the penalty kernel's LDS table holds", c.context_size, kPenMaxHistory);
    {   // decode steps per graph in the generate loop: a graph launch costs ~7 us of idle queue (124M: 224.8 us per token
        // with 1 step per graph, 220.4 with 2 / 4, 218.3 with 8, 219.5 with 16)
        const int k = env_int("ZGPT2_GRAPH_STEPS", 8);
        g->graph.steps = (k == 2 || k == 4 || k == 8 || k == 16 || k == 32 || k == 64) ? (size_t)k : 1;
    }
    g->graph.n_buckets = (c.context_size + 63) / 64;
    g->graph.execs.assign(kStepShapes * g->graph.n_buckets, nullptr);
    // every decode graph is captured and instantiated here, not on the first forward that needs it
    ZG_TRY(setup_prefetcher(g));
    ZG_TRY(capture_all(g, gs(g)));
    if (parent) {
        ++parent->n_children;
        g->counted = true;
    }
    return ZG_OK;
}

// A new sequence starts (position 1 of the token-at-a-time loop, a whole-prompt pass, a generation): the caches are cleared.  The
// decode attention loads the rows of its whole 64-position bucket and gives the ones at or behind the sequence length a
// probability of exactly 0 — which silences any finite leftover of an earlier sequence, but 0 x NaN is NaN: once a sequence had
// overflowed (or a checkpoint held a NaN) every later sequence on the handle came out NaN as well, repaired weights or not
// (tools/fuzz_errors_gpt.py).  124M, one sequence: 75 MB, ~20 us per generation of 217 ms.
// from_row > 0 (a whole-prompt pass writes rows 0 .. from_row - 1 itself): only the rows behind it, strip by strip — eight
// 1023-token prompts would otherwise pay a 600 MB memset (0.12 ms of a 5.4 ms pass) for one stale row per head.
// keep_head (a continuation: rows below from_row are the session): never the memset of the whole region.
// The caches of all layers lie one behind the other, K then V, the same number of bytes apart: that distance.
static int kv_cache_stride(const zg_gpt* g, size_t* out) {
    const size_t L = g->cfg.n_layer, elems = g->batch * g->cfg.context_size * g->cfg.n_embed;
    const size_t stride = L > 1 ? (size_t)(reinterpret_cast<char*>(g->layers[1].k_cache) - reinterpret_cast<char*>(g->layers[0].k_cache)) / 2
                                : (size_t)(reinterpret_cast<char*>(g->layers[0].v_cache) - reinterpret_cast<char*>(g->layers[0].k_cache));
    ZG_REQUIRE(stride >= elems * kv_elem_bytes(g) && reinterpret_cast<char*>(g->layers[0].v_cache) - reinterpret_cast<char*>(g->layers[0].k_cache) == (ptrdiff_t)stride,
               ZG_ERR_UNSUPPORTED, "kv caches: cache stride");
    *out = stride;
    return ZG_OK;
}

static int clear_kv(zg_gpt* g, hipStream_t s, size_t from_row = 0, bool keep_head = false) {
    if (g->kv_region_bytes == 0 || g->arena == nullptr) return ZG_OK;
    const size_t C = g->cfg.context_size, E = g->cfg.n_embed, B = g->batch, L = g->cfg.n_layer;
    if (keep_head && from_row >= C) return ZG_OK;
    if (!keep_head && (from_row == 0 || from_row * 2 < C)) {
        ZG_HIP(hipMemsetAsync(g->layers[0].k_cache, 0, g->kv_region_bytes, s));
        return ZG_OK;
    }
    const size_t elems = B * C * E;
    size_t stride = 0;
    ZG_TRY(kv_cache_stride(g, &stride));
    const int strips = (int)(B * g->cfg.n_heads);
    ZG_TRY(launch_kv_clear_tail(g->layers[0].k_cache, (int)(2 * L), stride, 0, g->kv_mode == 0 ? 256 : 128, strips, (int)C, (int)from_row, s));
    if (g->kv_mode == 2) ZG_TRY(launch_kv_clear_tail(g->layers[0].k_cache, (int)(2 * L), stride, elems * 2, 64, strips, (int)C, (int)from_row, s));
    return ZG_OK;
}

}  // namespace

namespace zg {  // offered to the other units: api_gpt.h declares them

// (Re)derive the folded-LayerNorm vectors from the weights in the arena: after loading, or on ranks that received
// the weight region by broadcast.  A handful of small launches outside any graph.
int ensure_ln_folded(zg_gpt* g, hipStream_t s) {
    zg_gpt* r = root(g);  // the vectors live in the weight region: one flag per region, kept by its owner
    if (r->ln_folded) return ZG_OK;
    const int E = (int)g->cfg.n_embed;
    for (const zg_layer& y : g->layers) {
        ZG_TRY(launch_ln_fold(y.c_attn_w, g->wt, y.ln_1_g, y.ln_1_b, y.c_attn_b, 3 * E, E, y.c_attn_c2, y.c_attn_c3, s));
        ZG_TRY(launch_ln_fold(y.c_fc_w, g->wt, y.ln_2_g, y.ln_2_b, y.c_fc_b, 4 * E, E, y.c_fc_c2, y.c_fc_c3, s));
    }
    ZG_TRY(launch_ln_fold(g->wte, g->wt, g->ln_f_g, g->ln_f_b, nullptr, (int)g->cfg.vocab_size, E, g->lm_c2, g->lm_c3, s));
    // handles that share the region run on other streams: the vectors must be complete before any of them reads the flag
    if (r->n_children > 0 || g->parent) ZG_HIP(hipStreamSynchronize(s));
    r->ln_folded = true;
    return ZG_OK;
}

// The tagged hand-overs of the lock-step batch poll with a bound; a poller that ran into it raised the fault word.  The
// results of such a step are wrong, so every entry point that drains the stream fails (and clears the word for the next
// call).  The word lives in pinned host memory the kernels store to directly: reading it costs no copy and no second
// synchronisation.  PRECONDITION: the stream has been drained since the steps in question.
int check_fault(zg_gpt* g) {
    // both words are read and cleared before anything is reported: a tag fault left latched behind a stream-K fault of the same
    // drain would be charged to a later, healthy call
    unsigned sk = 0, tag = 0;
    if (g->pass.sk_used) {  // a whole-prompt pass may have handed half tiles over inside gemm_s4: did a consumer give up waiting?
        g->pass.sk_used = false;
        ZG_TRY(gemm_s4_fault(&sk));
    }
    if (g->modes.tags || g->modes.fused) {
        volatile unsigned* f = g->hand.fault;
        tag = *f;
        if (tag) *f = 0;
    }
    if (sk) {
        set_error("a half-tile hand-over of the whole-prompt c_attn GEMM timed out%s: results discarded", tag ? " (and a tagged hand-over of the decode step)" : "");
        return ZG_ERR_HIP;
    }
    if (tag) {
        set_error("a tagged hand-over of the decode step timed out (a workgroup waited %u polls for its writers): results discarded", g->hand.spin_limit);
        return ZG_ERR_HIP;
    }
    return ZG_OK;
}

// A tag is (epoch << 8 | launch id) in 32 bits: 24 bits of the step counter survive, and a slot that is only written at long
// contexts (the high attention splits) could meet its own tag again 2^24 steps later — about an hour of decoding.  So the
// host counts the steps it enqueues and zeroes the tagged words (tag 0 is never valid: launch ids start at 1) on the stream
// every 2^23 of them, in front of the steps of the call that crosses the mark.
// The rule holds while the device runs fewer than two steps per counted one: every path that advances the epoch counts its steps
// here (an upper bound is fine), and tests/test_handle_age_gpu.py holds each to that (zg_debug_gpt_age_state).
int note_steps(zg_gpt* g, size_t n, hipStream_t s) {
    if (!g->modes.tags && !g->modes.fused) return ZG_OK;
    g->hand.epochs_since_clear += n;
    g->hand.steps_counted += n;
    if (g->hand.epochs_since_clear < ((size_t)1 << 23)) return ZG_OK;
    g->hand.epochs_since_clear = n;
    ++g->hand.tag_clears;
    ZG_HIP(hipMemsetAsync(g->hand.sk_tag, 0, g->hand.sk_tag_bytes, s));
    ZG_HIP(hipMemsetAsync(g->hand.part_tag, 0, g->hand.part_tag_bytes, s));
    ZG_HIP(hipMemsetAsync(g->hand.qkv_tag, 0, g->hand.qkv_tag_bytes, s));
    return ZG_OK;
}

// The control block of the steps enqueued next, through its pinned mirror (n_partials is always the lm_head grid).
int stage_ctrl(zg_gpt* g, size_t step, size_t seq_len, int mode, hipStream_t s) {
    StepCtrl& h = g->h_ctrl->ctrl;
    h.step = (int)step;
    h.seq_len = (int)seq_len;
    h.mode = mode;
    h.n_partials = g->lm_grid;
    ZG_HIP(hipMemcpyAsync(g->ctrl, &h, sizeof(StepCtrl), hipMemcpyHostToDevice, s));
    return ZG_OK;
}

// n floats from device memory to a caller's pointer, which may be host or device.
int copy_out_f32(float* dst, const float* src, size_t n, hipStream_t s) {
    ZG_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    return ZG_OK;
}

// The cache policy of a whole-prompt pass over rows past .. end - 1.  past == 0, a new sequence: everything behind the pass is
// cleared (clear_kv).  A continuation: the rows behind it are cleared if anything was written there since they were last clean (a
// rollback, or zg_gpt_forward calls out of order) — the decode attention reads its whole 64-position bucket, and what a
// discarded row holds (a NaN, say) must not come back.  Rows below past are never touched.
int clear_for_pass(zg_gpt* g, hipStream_t s, size_t past, size_t end) {
    if (past == 0) ZG_TRY(clear_kv(g, s, end));
    else if (g->kv_dirty_hi > end) ZG_TRY(clear_kv(g, s, end, true));
    g->kv_dirty_hi = end;
    return ZG_OK;
}

// The row-to-row copy of all caches (elementwise.hip, kv_fork_kernel) on stream s, its grid sized for t_hi positions.  src / len in
// device memory (a captured beam step), or null: the table src_imm (four bits per row) and the length len_imm travel by value.
int enqueue_kv_fork(zg_gpt* g, int t_hi, const int* src, const int* len, unsigned src_imm, int len_imm, hipStream_t s) {
    KvForkArgs a{};
    a.base = reinterpret_cast<char*>(g->layers[0].k_cache);
    ZG_TRY(kv_cache_stride(g, &a.cache_stride));
    a.lo_off = g->batch * g->cfg.context_size * g->cfg.n_embed * 2;
    a.n_caches = (int)(2 * g->cfg.n_layer);
    a.batch = (int)g->batch;
    a.heads = (int)g->cfg.n_heads;
    a.ctx = (int)g->cfg.context_size;
    a.kv_mode = g->kv_mode;
    a.t_hi = t_hi;
    a.src = src;
    a.len = len;
    a.src_imm = src_imm;
    a.len_imm = len_imm;
    return launch_kv_fork(a, s);
}

// GPT.forward enqueued on the handle's stream, nothing drained (zg_gpt_forward drains; zg_gpt_sample puts its sampler behind it first)
// taps (zg_debug_gpt_step_taps): the same step launched eagerly, with copies of what each launch class wrote behind it
int forward_enqueue(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, int compute_logits, float* logits_out, size_t logits_len,
                    StepTaps* taps) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && tokens, ZG_ERR_ARG, "gpt_forward: null argument");
    ZG_REQUIRE(n_tokens == g->batch, ZG_ERR_SHAPE, "gpt_forward: %zu tokens for batch %zu", n_tokens, g->batch);
    ZG_REQUIRE(seq_len >= 1 && seq_len <= g->cfg.context_size, ZG_ERR_SHAPE, "gpt_forward: seq_len %zu outside 1..%zu",
               seq_len, g->cfg.context_size);
    const size_t V = g->cfg.vocab_size;
    ZG_REQUIRE(!logits_out || (compute_logits && logits_len >= g->batch * V), ZG_ERR_SHAPE,
               "gpt_forward: logits_out needs compute_logits and %zu elements", g->batch * V);
    hipStream_t s = gs(g);
    for (size_t b = 0; b < g->batch; ++b) {
        ZG_REQUIRE(tokens[b] < V, ZG_ERR_SHAPE, "gpt_forward: token %zu >= vocab %zu", tokens[b], V);
        g->h_ints[b] = (int)tokens[b];
    }
    ZG_HIP(hipMemcpyAsync(g->forced, g->h_ints, g->batch * sizeof(int), hipMemcpyHostToDevice, s));
    ZG_TRY(stage_ctrl(g, seq_len - 1, seq_len, 1, s));
    if (seq_len == 1) {
        ZG_TRY(clear_kv(g, s));
        g->kv_dirty_hi = 0;
    }
    g->cached_len = seq_len;
    if (seq_len > g->kv_dirty_hi) g->kv_dirty_hi = seq_len;
    ZG_TRY(note_steps(g, 1, s));
    ZG_TRY(ensure_ln_folded(g, s));
    g->hidden.src = HID_X;
    if (taps) {
        StepOpts o;
        o.taps = taps;
        ZG_TRY(enqueue_step(g, compute_logits != 0, bucket_t_hi(g, seq_len), s, o));
    } else
        ZG_TRY(run_step(g, compute_logits != 0, seq_len, s));
    if (logits_out) ZG_TRY(copy_out_f32(logits_out, g->logits, g->batch * V, s));
    return ZG_OK;
}

}  // namespace zg

extern "C" {

int zg_gpt_create(zg_gpt** out, const zg_gpt_config* config, size_t batch, unsigned flags) {
    return zg_gpt_create_ex(out, config, batch, flags, nullptr);
}

int zg_gpt_create_ex(zg_gpt** out, const zg_gpt_config* config, size_t batch, unsigned flags, const zg_gpt_options* opt) {
    ZG_TRY(require_init());
    ZG_REQUIRE(out && config, ZG_ERR_ARG, "zg_gpt_create: null argument");
    const zg_gpt_config& c = *config;
    zg_gpt* parent = opt ? opt->share_weights_with : nullptr;
    if (parent) {
        ZG_REQUIRE(parent->parent == nullptr, ZG_ERR_ARG, "zg_gpt_create_ex: share_weights_with must own its weights");
        ZG_REQUIRE(memcmp(&parent->cfg, config, sizeof(zg_gpt_config)) == 0, ZG_ERR_SHAPE, "zg_gpt_create_ex: a handle shares weights with one of the same config only");
        const unsigned same = ZG_GPT_WEIGHTS_F32 | ZG_GPT_WEIGHTS_B24 | ZG_GPT_NO_PREFILL;  // what decides the layout of the weight region
        ZG_REQUIRE((parent->flags & same) == (flags & same), ZG_ERR_ARG, "zg_gpt_create_ex: weight type / prefill flags differ from the weight owner's");
    }
    ZG_REQUIRE(c.n_heads > 0 && c.n_embed % c.n_heads == 0 && c.n_embed / c.n_heads == 64, ZG_ERR_UNSUPPORTED,
               "head_dim %zu != 64 (GPT-2 family only)", c.n_heads ? c.n_embed / c.n_heads : (size_t)0);
    ZG_REQUIRE(c.n_embed % 8 == 0 && c.n_embed * 4 <= 8192, ZG_ERR_UNSUPPORTED, "n_embed %zu unsupported", c.n_embed);
    ZG_REQUIRE(batch >= 1 && batch <= 8, ZG_ERR_UNSUPPORTED, "batch %zu outside 1..8", batch);
    ZG_REQUIRE(c.vocab_size > 0 && c.context_size > 0 && c.n_layer > 0, ZG_ERR_ARG, "empty config");
    ZG_REQUIRE(!(flags & ZG_GPT_KV_F16) || !(flags & ZG_GPT_KV_B24), ZG_ERR_ARG, "ZG_GPT_KV_F16 and ZG_GPT_KV_B24 exclude each other");
    ZG_REQUIRE(!(flags & ZG_GPT_WEIGHTS_F32) || !(flags & ZG_GPT_WEIGHTS_B24), ZG_ERR_ARG,
               "ZG_GPT_WEIGHTS_F32 and ZG_GPT_WEIGHTS_B24 exclude each other");
    zg_gpt* g = new zg_gpt();  // (every member zero: release() relies on it)
    g->cfg = c;
    g->batch = batch;
    g->flags = flags;
    g->wt = (flags & ZG_GPT_WEIGHTS_F32) ? WT_F32 : (flags & ZG_GPT_WEIGHTS_B24) ? WT_B24 : WT_BF16;
    g->wbytes = g->wt == WT_BF16 ? 2 : g->wt == WT_B24 ? 3 : 4;
    g->kv_mode = (flags & ZG_GPT_KV_F16) ? 1 : (flags & ZG_GPT_KV_B24) ? 2 : 0;
    g->max_splits = (int)((c.context_size + kAttnChunk - 1) / kAttnChunk);
    g->parent = parent;
    const int st = build_handle(g, opt);
    if (st != ZG_OK) {
        release(g);
        return st;
    }
    *out = g;
    return ZG_OK;
}

int zg_gpt_destroy(zg_gpt* g) {
    if (!g) return ZG_OK;
    ZG_REQUIRE(g->n_children == 0, ZG_ERR_ARG, "zg_gpt_destroy: %d handle(s) still borrow this one's weights (destroy them first)", g->n_children);
    release(g);
    return ZG_OK;
}

int zg_gpt_stream(zg_gpt* g, void** hip_stream_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && hip_stream_out, ZG_ERR_ARG, "zg_gpt_stream: null argument");
    *hip_stream_out = gs(g);
    return ZG_OK;
}

// Where a tensor slot lives: a vector of n floats (K = 0), or a matrix of n elements in rows of K inputs with, on handles that
// keep them, its bf16 planes for the whole-prompt GEMMs.
struct Slot {
    void* dst;
    size_t n, K;
    bf16_t* planes;
};

static int load_slot(zg_gpt* g, const Slot& t, const char* what, int slot, const float* src, size_t len) {
    ZG_REQUIRE(t.dst != nullptr, ZG_ERR_ARG, "unknown %s %d", what, slot);
    ZG_REQUIRE(len == t.n, ZG_ERR_SHAPE, "%s %d expects %zu elements, got %zu", what, slot, t.n, len);
    const bool mat = t.K != 0;
    g->ln_folded = false;
    if (mat && g->wt == WT_B24) return upload_b24(src, t.n, t.K, t.dst, t.planes, gs(g));
    ZG_TRY(upload_f32(src, t.n, t.dst, mat && g->wt == WT_BF16, gs(g)));
    if (g->wt == WT_F32 && t.planes) {  // exact bf16 planes of the fp32 matrix for the whole-prompt GEMMs
        // plane-major [3][out][in]: the matrix as ONE row of out * in elements
        ZG_REQUIRE(t.n <= (size_t)2147483647 / 3, ZG_ERR_SHAPE, "weight matrix of %zu elements", t.n);  // (split3_kernel indexes 3 n in int)
        ZG_TRY(launch_split3(reinterpret_cast<const float*>(t.dst), 1, (int)t.n, t.planes, gs(g)));
        ZG_HIP(hipStreamSynchronize(gs(g)));
    }
    return ZG_OK;
}

int zg_gpt_load_block_tensor(zg_gpt* g, size_t layer, int slot, const float* src, size_t len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && src && layer < g->cfg.n_layer, ZG_ERR_ARG, "load_block_tensor: bad argument");
    ZG_REQUIRE(g->parent == nullptr, ZG_ERR_ARG, "load_block_tensor: this handle borrows its weights (load them into their owner)");
    const size_t E = g->cfg.n_embed;
    zg_layer& y = g->layers[layer];
    Slot t{};
    switch (slot) {  // (a matrix: K = its input width)
        case ZG_LN_1_G: t = {y.ln_1_g, E, 0, nullptr}; break;
        case ZG_LN_1_B: t = {y.ln_1_b, E, 0, nullptr}; break;
        case ZG_C_ATTN_W: t = {y.c_attn_w, 3 * E * E, E, y.c_attn_p}; break;
        case ZG_C_ATTN_B: t = {y.c_attn_b, 3 * E, 0, nullptr}; break;
        case ZG_C_PROJ_W: t = {y.c_proj_w, E * E, E, y.c_proj_p}; break;
        case ZG_C_PROJ_B: t = {y.c_proj_b, E, 0, nullptr}; break;
        case ZG_LN_2_G: t = {y.ln_2_g, E, 0, nullptr}; break;
        case ZG_LN_2_B: t = {y.ln_2_b, E, 0, nullptr}; break;
        case ZG_C_FC_W: t = {y.c_fc_w, 4 * E * E, E, y.c_fc_p}; break;
        case ZG_C_FC_B: t = {y.c_fc_b, 4 * E, 0, nullptr}; break;
        case ZG_MLP_PROJ_W: t = {y.mlp_proj_w, 4 * E * E, 4 * E, y.mlp_proj_p}; break;
        case ZG_MLP_PROJ_B: t = {y.mlp_proj_b, E, 0, nullptr}; break;
    }
    return load_slot(g, t, "block slot", slot, src, len);
}

int zg_gpt_load_tensor(zg_gpt* g, int slot, const float* src, size_t len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && src, ZG_ERR_ARG, "load_tensor: bad argument");
    ZG_REQUIRE(g->parent == nullptr, ZG_ERR_ARG, "load_tensor: this handle borrows its weights (load them into their owner)");
    const size_t E = g->cfg.n_embed;
    Slot t{};
    switch (slot) {
        case ZG_WTE: t = {g->wte, g->cfg.vocab_size * E, E, nullptr}; break;
        case ZG_WPE: t = {g->wpe, g->cfg.context_size * E, E, nullptr}; break;
        case ZG_LN_F_G: t = {g->ln_f_g, E, 0, nullptr}; break;
        case ZG_LN_F_B: t = {g->ln_f_b, E, 0, nullptr}; break;
    }
    ZG_TRY(load_slot(g, t, "slot", slot, src, len));
    if (slot == ZG_WTE) {  // the scoring lm_head's strip / planes of the new wte: here for this handle, at their next score for its borrowers
        ++g->w_gen;
        ZG_TRY(ensure_score_weights(g, gs(g)));
        ZG_HIP(hipStreamSynchronize(gs(g)));
    }
    return ZG_OK;
}

int zg_gpt_weight_arena(zg_gpt* g, void** device_ptr, size_t* bytes) {
    ZG_REQUIRE(g && device_ptr && bytes, ZG_ERR_ARG, "weight_arena: null argument");
    // The folded-LayerNorm vectors (c2 / c3) live inside the region handed out here.  A sender has to hold valid
    // ones before its bytes are copied, and a receiver must re-derive them from whatever lands in the region — also a
    // receiver that has run before (its flag would still say "folded").  So: fold now if needed (sender side: a few
    // small launches, drained), and mark the vectors stale for the next forward (receiver side: one re-fold).
    if (!root(g)->ln_folded) {
        ZG_TRY(require_init());
        ZG_TRY(ensure_ln_folded(g, gs(g)));
        ZG_HIP(hipStreamSynchronize(gs(g)));
    }
    root(g)->ln_folded = false;
    ++root(g)->w_gen;  // (zg_gpt_score re-derives its strip / planes likewise)
    *device_ptr = g->wbase;
    *bytes = g->weight_region_bytes;
    return ZG_OK;
}

// load_gpt (src/main.zig:304-314) on ONE GPU of the node, then this: the weight region goes to every other rank's arena in one
// RCCL broadcast on the library's stream (dist.hip).  ms_out (optional): device time of the broadcast.
int zg_gpt_broadcast_weights(zg_gpt* g, int root, float* ms_out) {
    ZG_TRY(require_init());
    void* p = nullptr;
    size_t n = 0;
    ZG_TRY(zg_gpt_weight_arena(g, &p, &n));  // (sender: folded vectors valid; receiver: re-fold at the next forward)
    hipStream_t s = gs(g);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ms_out) {
        ZG_HIP(hipEventCreate(&e0));
        ZG_HIP(hipEventCreate(&e1));
        ZG_HIP(hipEventRecord(e0, s));
    }
    const int st = zg::dist_broadcast(p, n, root, s);
    if (ms_out && st == ZG_OK) ZG_HIP(hipEventRecord(e1, s));
    const hipError_t he = hipStreamSynchronize(s);
    if (ms_out) {
        if (st == ZG_OK && he == hipSuccess) (void)hipEventElapsedTime(ms_out, e0, e1);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    ZG_TRY(st);
    ZG_HIP(he);
    return ZG_OK;
}

int zg_gpt_step_bytes(zg_gpt* g, size_t seq_len, size_t* weight_bytes, size_t* kv_bytes) {
    ZG_REQUIRE(g, ZG_ERR_ARG, "step_bytes: null argument");
    const size_t E = g->cfg.n_embed;
    // wbytes * (sum_layers in*out + V*E) + kvbytes * 2 * T * E * L (per sequence)
    if (weight_bytes) *weight_bytes = g->wbytes * (g->cfg.n_layer * 12 * E * E + g->cfg.vocab_size * E);
    if (kv_bytes) *kv_bytes = kv_elem_bytes(g) * 2 * seq_len * E * g->cfg.n_layer * g->batch;
    return ZG_OK;
}

int zg_gpt_forward(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, int compute_logits,
                   float* logits_out, size_t logits_len) {
    ZG_TRY(forward_enqueue(g, seq_len, tokens, n_tokens, compute_logits, logits_out, logits_len));
    // h_ints / h_ctrl are reused by the next call: drain before returning.
    ZG_HIP(hipStreamSynchronize(gs(g)));
    return check_fault(g);
}

int zg_gpt_cached_len(zg_gpt* g, size_t* len_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && len_out, ZG_ERR_ARG, "gpt_cached_len: null argument");
    *len_out = g->cached_len;
    return ZG_OK;
}

int zg_gpt_kv_fork(zg_gpt* g, const size_t* src_rows, size_t n_rows) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && src_rows, ZG_ERR_ARG, "gpt_kv_fork: null argument");
    const size_t B = g->batch;
    ZG_REQUIRE(n_rows == B, ZG_ERR_ARG, "gpt_kv_fork: %zu source rows for batch %zu", n_rows, B);
    for (size_t b = 0; b < B; ++b) ZG_REQUIRE(src_rows[b] < B, ZG_ERR_SHAPE, "gpt_kv_fork: row %zu copies row %zu of %zu", b, src_rows[b], B);
    unsigned table = 0;
    bool moves = false;
    for (size_t b = 0; b < B; ++b) {
        ZG_REQUIRE(src_rows[src_rows[b]] == src_rows[b], ZG_ERR_ARG, "gpt_kv_fork: row %zu copies row %zu, which is itself overwritten (from row %zu)", b,
                   src_rows[b], src_rows[src_rows[b]]);
        table |= (unsigned)src_rows[b] << (4 * b);
        moves = moves || src_rows[b] != b;
    }
    if (!moves || g->cached_len == 0) return ZG_OK;
    return enqueue_kv_fork(g, bucket_t_hi(g, g->cached_len), nullptr, nullptr, table, (int)g->cached_len, gs(g));
}

int zg_gpt_argmax(zg_gpt* g, size_t* tokens_out, size_t n_tokens) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && tokens_out && n_tokens == g->batch, ZG_ERR_ARG, "gpt_argmax: bad argument");
    hipStream_t s = gs(g);
    ZG_TRY(launch_embed_step(embed_args(g, 2), s));
    ZG_HIP(hipMemcpyAsync(g->h_ints, g->cur_token, g->batch * sizeof(int), hipMemcpyDeviceToHost, s));
    ZG_HIP(hipStreamSynchronize(s));
    for (size_t b = 0; b < g->batch; ++b) tokens_out[b] = (size_t)g->h_ints[b];
    return ZG_OK;
}

int zg_gpt_hidden(zg_gpt* g, float* x_out, size_t len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && x_out && len >= g->batch * g->cfg.n_embed, ZG_ERR_ARG, "gpt_hidden: bad argument");
    hipStream_t s = gs(g);
    const size_t B = g->batch, E = g->cfg.n_embed;
    // ln_f exists only folded into lm_head (lm_head_args): here it runs out of place, in h4 — scratch every step and pass rewrites
    // before reading it.  x stays the residual stream the next argmax / sample / step expects.
    if (g->hidden.src == HID_X) ZG_TRY(launch_copy_f32(g->x, g->h4, B * E, s));
    else {
        const size_t P = g->hidden.P;
        if (g->hidden.src == HID_PASS_OPEN) {
            ZG_TRY(ensure_ln_folded(g, s));
            ZG_TRY(enqueue_prefill(g, g->hidden.pos0, P, true, s, nullptr, true));
        }
        ZG_HIP(hipMemcpy2DAsync(g->h4, E * 4, g->pass.x + (P - 1) * E, P * E * 4, E * 4, B, hipMemcpyDeviceToDevice, s));
    }
    ZG_TRY(launch_layernorm(g->h4, (int)B, (int)E, g->ln_f_g, g->ln_f_b, 1e-5f, s));
    ZG_TRY(copy_out_f32(x_out, g->h4, B * E, s));
    ZG_HIP(hipStreamSynchronize(s));
    return check_fault(g);
}

}  // extern "C"
