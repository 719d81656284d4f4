// api_gpt_pass.hip — model tier of the C ABI: the whole-prompt pass, which exists once (pass_impl: zg_gpt_prefill is zg_gpt_extend
// at 0, zg_gpt_score the same pass with the scoring stage behind it).
#include <algorithm>

#include "api_gpt.h"

using namespace zg;

namespace {  // this unit only

// The epoch of the next stream-K launch (gemm_s4.hip SK: the producer stores it into sk_flags, the consumer waits until its flag
// word equals it).  One per layer per pass in 32 bits: days of continuous prefill wrap it.  0 is what every flag word holds that no
// launch has written, and behind the wrap a small value is what a word may still hold from the handle's first launches — a
// consumer would take a half tile nobody produced, with no fault raised.  So 0 is never handed out, and where the count begins
// again the flag words are zeroed on the stream in front of the launch (as note_steps does for the decode tags): every word then
// holds 0, and from there on every epoch handed out is larger than every word written before it.
int next_sk_epoch(zg_gpt* g, hipStream_t s, unsigned* out) {
    if (++g->pass.sk_epoch == 0u) {
        ZG_HIP(hipMemsetAsync(g->pass.sk_flags, 0, kSkFlagWords * sizeof(unsigned), s));
        g->pass.sk_epoch = 1u;
        ++g->pass.sk_restarts;
    }
    *out = g->pass.sk_epoch;
    return ZG_OK;
}

// The scoring stage of a pass of n new positions per sequence behind `past` cached ones, whose residual stream of every row is
// in pass.x: ln_f of all rows once (pass.a is free: the pass is over), then block by block of kScoreRows rows the lm_head on the
// matrix cores into score.logits, the two statistics launches, and on request the block's logits to the caller.
// taps (zg_debug_gpt_pass_taps): class 7 — the ln_f planes, then per block (the table's layer field) each GEMM's plan and the block's rows of score.logits.
static int enqueue_score(zg_gpt* g, size_t past, size_t n, float* logits_out, hipStream_t s, StepTaps* taps = nullptr) {
    const size_t E = g->cfg.n_embed, V = g->cfg.vocab_size, C = g->cfg.context_size, V64 = g->score.v64, head = V / 64 * 64, M = g->batch * n;
    const int iE = (int)E, ld = (int)V64;
    const int np = (g->flags & ZG_GPT_PREFILL_2PLANE) ? 2 : kSplit;
    ZG_TRY(ensure_score_weights(g, s));
    ZG_TRY(launch_ln_split(g->pass.x, (int)M, iE, g->ln_f_g, g->ln_f_b, 1e-5f, g->pass.a, s));
    PrefillGemmPlan plan{};
    PrefillGemmPlan* const plan_out = taps ? &plan : nullptr;
    auto tap_plan = [&](size_t block) {
        if (!taps) return (int)ZG_OK;
        int v[ZG_PREFILL_PLAN_INTS];
        prefill_plan_ints(plan, v);
        return tap_words(taps, 7, block, ZG_TAP_PLAN, v, ZG_PREFILL_PLAN_INTS);
    };
    if (taps) ZG_TRY(tap_put(taps, 7, 0, ZG_TAP_A, ZG_TAP_BF16, 0, g->pass.a, 1, M * kSplit * E * 2, M * kSplit * E * 2, s));
    for (size_t r0 = 0; r0 < M; r0 += kScoreRows) {
        const int rows = (int)std::min(kScoreRows, M - r0);
        const bf16_t* A = g->pass.a + r0 * kSplit * E;
        if (g->wt != WT_BF16) {  // the planes hold zero rows up to V64: one launch
            ZG_TRY(launch_prefill_gemm(A, g->score.planes, nullptr, g->score.logits, rows, ld, iE, ld, PF_F32, g->score.gemm_ws, g->score.gemm_ws_floats, nullptr, s, nullptr,
                                       kWeightPlanes, nullptr, plan_out));
            ZG_TRY(tap_plan(r0 / kScoreRows));
        } else {  // the whole 64-row groups of wte where they lie, then the strip: no row behind V - 1 of wte is read
            if (head) {
                ZG_TRY(launch_prefill_gemm(A, reinterpret_cast<const bf16_t*>(g->wte), nullptr, g->score.logits, rows, (int)head, iE, ld, PF_F32, g->pass.ws,
                                           g->pass.ws_floats, nullptr, s, nullptr, np, nullptr, plan_out));
                ZG_TRY(tap_plan(r0 / kScoreRows));
            }
            if (g->score.tail) {
                ZG_TRY(launch_prefill_gemm(A, g->score.tail, nullptr, g->score.logits + head, rows, 64, iE, ld, PF_F32, g->pass.ws, g->pass.ws_floats, nullptr, s, nullptr, np,
                                           nullptr, plan_out));
                ZG_TRY(tap_plan(r0 / kScoreRows));
            }
        }
        if (taps) ZG_TRY(tap_put(taps, 7, r0 / kScoreRows, ZG_TAP_LOGITS, ZG_TAP_F32, 0, g->score.logits, 1, (size_t)rows * V64 * 4, (size_t)rows * V64 * 4, s));
        const ScoreTargets tg{g->prompt, (int)C, (int)n, (int)past, (int)r0};
        ZG_TRY(launch_score(g->score.logits, rows, (int)V, ld, g->lp.top, g->score.ws, tg, g->lp.rec, s));
        if (logits_out)
            ZG_HIP(hipMemcpy2DAsync(logits_out + r0 * V, V * 4, g->score.logits, V64 * 4, V * 4, (size_t)rows,
                                    is_device_ptr(logits_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    }
    return ZG_OK;
}

}  // namespace

namespace zg {  // offered to the other units: api_gpt.h declares them

// (Re)derive what the scoring lm_head reads beside the weight region (the tail strip, or wte's planes) from the wte in the arena:
// after ZG_WTE was loaded, and on handles whose region was filled some other way (a borrowed region, a broadcast).
int ensure_score_weights(zg_gpt* g, hipStream_t s) {
    if (!g->score.logits || g->score.gen == root(g)->w_gen + 1) return ZG_OK;
    const size_t E = g->cfg.n_embed, V = g->cfg.vocab_size, head = V / 64 * 64;
    if (g->wt != WT_BF16) ZG_TRY(launch_wte_planes(g->wte, g->wt, V, g->score.v64, (int)E, g->score.planes, s));
    else if (g->score.tail) {
        ZG_HIP(hipMemsetAsync(g->score.tail, 0, 64 * E * 2, s));
        ZG_HIP(hipMemcpyAsync(g->score.tail, reinterpret_cast<const bf16_t*>(g->wte) + head * E, (V - head) * E * 2, hipMemcpyDeviceToDevice, s));
    }
    g->score.gen = root(g)->w_gen + 1;
    return ZG_OK;
}

// Whole-prompt forward of positions 0..P-1 of every sequence (tokens in g->prompt): fills the KV caches
// exactly as P calls of GPT.forward would (main.zig:331-334) and leaves the residual stream of all rows in
// pass.x.  With `last_block_full` false the last Block stops after its cache append: nothing downstream of
// it is needed when generation re-feeds the last prompt token (main.zig:337).
// fp32 weights (ZG_GPT_WEIGHTS_F32): the same pass; the weight operand is then the exact three-term bf16 split of the fp32
// matrix (plane-major, made when the tensor is loaded; B24 weights: the split of the 24-bit values, the same pass) and every GEMM runs as three partial passes of the same kernel — the
// six plane products above 2^-24 of the leading one, fp32-sgemm grade (prefill.hip prefill_gemm_wp_kernel).
// (Measured and dropped in round 4: replaying this pass from a hipGraph per prompt length.  0.844 against 0.749 ms at 64
// tokens, 1.645 against 1.553 ms at 1023 — the ~10 us a launch costs here is the kernels' own latency at these sizes, not host
// overhead, and a graph launch adds its own ~10 us; profiles/round4_prefill_graph.jsonl.)
// pos0 > 0 (a continuation): the P rows are positions pos0 .. pos0 + P - 1 (tokens g->prompt[b][pos0 + t]); they are appended
// behind the pos0 cached rows, and the attention reads every key, old and new, from the caches in their storage format.
// taps (zg_debug_gpt_pass_taps): behind every launch, copies of what it wrote (include/zgpt2.h lists them); the launches are the same.
// resume_last_block (zg_gpt_hidden behind a pass that stopped there): only what such a pass left out — the last Block from its
// attention on, over the q columns pass.qkv still holds, the caches and the residual stream in pass.x.  hidden records which of the
// two the handle is behind.
int enqueue_prefill(zg_gpt* g, size_t pos0, size_t P, bool last_block_full, hipStream_t s, StepTaps* taps, bool resume_last_block) {
    const bool f32w = g->wt != WT_BF16;
    const int np = f32w ? kWeightPlanes : (g->flags & ZG_GPT_PREFILL_2PLANE) ? 2 : kSplit;
    const size_t E = g->cfg.n_embed, L = g->cfg.n_layer, H = g->cfg.n_heads, C = g->cfg.context_size;
    const int B = (int)g->batch, M = (int)(g->batch * P), iE = (int)E;
    const size_t Mz = (size_t)M, T_tap = std::min(C, pos0 + P + kPassTapRowsBehind);
    PrefillGemmPlan plan{};
    PrefillGemmPlan* const plan_out = taps ? &plan : nullptr;
    auto tap_x = [&](int cls, size_t l) { return taps ? tap_put(taps, cls, l, ZG_TAP_X, ZG_TAP_F32, 0, g->pass.x, 1, Mz * E * 4, Mz * E * 4, s) : ZG_OK; };
    auto tap_a = [&](int cls, size_t l, unsigned f) {
        return taps ? tap_put(taps, cls, l, ZG_TAP_A, ZG_TAP_BF16, f, g->pass.a, 1, Mz * kSplit * E * 2, Mz * kSplit * E * 2, s) : ZG_OK;
    };
    auto tap_plan = [&](int cls, size_t l) {
        if (!taps) return (int)ZG_OK;
        int v[ZG_PREFILL_PLAN_INTS];
        prefill_plan_ints(plan, v);
        return tap_words(taps, cls, l, ZG_TAP_PLAN, v, ZG_PREFILL_PLAN_INTS);
    };
    const bool resume = resume_last_block;
    g->hidden.src = HID_X;  // until every launch below is enqueued: a pass that fails halfway leaves no claim on pass.x
    if (!resume) {
        ZG_TRY(launch_embed_prefill(g->prompt, (int)C, B, (int)P, g->wte, g->wpe, g->wt, iE, g->pass.x, s, (int)pos0));
        ZG_TRY(tap_x(0, 0));
        ZG_TRY(launch_ln_split(g->pass.x, M, iE, g->layers[0].ln_1_g, g->layers[0].ln_1_b, 1e-5f, g->pass.a, s));
        ZG_TRY(tap_a(1, 0, 0));
    }
    for (size_t l = resume ? L - 1 : 0; l < L; ++l) {
        const zg_layer& y = g->layers[l];
        if (!resume) {
            // pass.a holds split(ln_1(x)) here: from the line above or from the tail of the previous Block's last GEMM
            // c_attn with the cache append of ops.zig:152-157 in its epilogue
            PrefillQkv qa{(int)P, iE, (int)H, (int)C, g->kv_mode, y.k_cache, y.v_cache, g->batch * C * E * 2};
            qa.pos0 = (int)pos0;
            if (!f32w && g->pass.sk_flags != nullptr) {  // (the persistent GEMM may hand half tiles over between workgroups: gemm_s4.hip SK)
                qa.sk_ws = g->pass.ws;
                qa.sk_ws_bytes = g->pass.ws_floats * 4;
                qa.sk_flags = g->pass.sk_flags;
                qa.sk_flags_words = (unsigned)kSkFlagWords;
                ZG_TRY(next_sk_epoch(g, s, &qa.sk_epoch));
                g->pass.sk_used = true;
            }
            if (taps) ZG_TRY(tap_caches(g, taps, -1, l, 0, T_tap, s));
            ZG_TRY(launch_prefill_gemm(g->pass.a, f32w ? y.c_attn_p : (const bf16_t*)y.c_attn_w, y.c_attn_b, g->pass.qkv, M, 3 * iE, iE, 3 * iE, PF_QKV,
                                       g->pass.ws, g->pass.ws_floats, nullptr, s, &qa, np, nullptr, plan_out));
            if (taps) {  // q, then the k | v columns: the persistent kernel leaves those to an fp32 cache (gemm_s4.hip S4_QKV)
                const unsigned kv_cols = plan.family == PFF_S4 && g->kv_mode == 0 ? ZG_TAP_NOT_WRITTEN : 0u;
                ZG_TRY(tap_plan(2, l));
                ZG_TRY(tap_put(taps, 2, l, ZG_TAP_Q, ZG_TAP_F32, 0, g->pass.qkv, Mz, E * 4, 3 * E * 4, s));
                ZG_TRY(tap_put(taps, 2, l, ZG_TAP_QKV_KV, ZG_TAP_F32, kv_cols, g->pass.qkv + E, Mz, 2 * E * 4, 3 * E * 4, s));
                ZG_TRY(tap_caches(g, taps, 2, l, 0, T_tap, s));
            }
            if (l + 1 == L && !last_block_full) {
                g->hidden = {HID_PASS_OPEN, pos0, P};
                return ZG_OK;
            }
        }
        // K and V: the caches — except a whole prompt on an fp16 / B24 cache, which reads the unrounded k / v columns of qkv (an fp32
        // cache is read directly: the c_attn epilogue then need not store those columns)
        PrefillKv kv;
        if (pos0 > 0 || g->kv_mode == 0) kv = PrefillKv{y.k_cache, y.v_cache, g->kv_mode, g->batch * C * E * 2, (int)C};
        int ran[3] = {0, 0, 0};
        ZG_TRY(launch_attn_prefill(g->pass.qkv, g->pass.a, B, (int)pos0, (int)P, iE, (int)H, g->pass.ws, g->pass.ws_floats, kv, s, 0, taps ? ran : nullptr));
        if (taps) ZG_TRY(tap_words(taps, 3, l, ZG_TAP_GEO, ran, 3));
        ZG_TRY(tap_a(3, l, 0));
        const PrefillLn ln2{y.ln_2_g, y.ln_2_b, 1e-5f, g->pass.a};
        ZG_TRY(launch_prefill_gemm(g->pass.a, f32w ? y.c_proj_p : (const bf16_t*)y.c_proj_w, y.c_proj_b, g->pass.x, M, iE, iE, iE, PF_RESID, g->pass.ws,
                                   g->pass.ws_floats, &ln2, s, nullptr, np, nullptr, plan_out));
        ZG_TRY(tap_plan(4, l));
        ZG_TRY(tap_x(4, l));
        ZG_TRY(tap_a(4, l, 0));
        ZG_TRY(launch_prefill_gemm(g->pass.a, f32w ? y.c_fc_p : (const bf16_t*)y.c_fc_w, y.c_fc_b, g->pass.h, M, 4 * iE, iE, 0, PF_GELU_SPLIT, g->pass.ws,
                                   g->pass.ws_floats, nullptr, s, nullptr, np, nullptr, plan_out));
        ZG_TRY(tap_plan(5, l));
        if (taps) ZG_TRY(tap_put(taps, 5, l, ZG_TAP_HP, ZG_TAP_BF16, 0, g->pass.h, 1, Mz * kSplit * 4 * E * 2, Mz * kSplit * 4 * E * 2, s));
        const bool more = l + 1 < L;
        const PrefillLn ln1{more ? g->layers[l + 1].ln_1_g : nullptr, more ? g->layers[l + 1].ln_1_b : nullptr, 1e-5f, g->pass.a};
        ZG_TRY(launch_prefill_gemm(g->pass.h, f32w ? y.mlp_proj_p : (const bf16_t*)y.mlp_proj_w, y.mlp_proj_b, g->pass.x, M, iE, 4 * iE, iE, PF_RESID, g->pass.ws,
                                   g->pass.ws_floats, more ? &ln1 : nullptr, s, nullptr, np, nullptr, plan_out));
        ZG_TRY(tap_plan(6, l));
        ZG_TRY(tap_x(6, l));
        ZG_TRY(tap_a(6, l, more ? 0u : ZG_TAP_NOT_WRITTEN));
    }
    g->hidden = {HID_PASS_DONE, pos0, P};
    return ZG_OK;
}

size_t prefill_min() { return 4; }  // shorter prompts go through the decode chain (measured: the whole-prompt pass pays from 4 tokens up)

// The whole-prompt pass: n tokens of every sequence go to positions past_len .. past_len + n - 1 behind the cached
// ones — the prompt loop of generate (main.zig:331-334) at an offset — and, on request, ln_f + lm_head of each sequence's last new
// position run through the decode kernels.  Everything is checked before the handle or its staging is touched.
// sc (zg_gpt_score): behind the pass, the scoring stage over all of its rows.
int pass_impl(zg_gpt* g, size_t past_len, const size_t* tokens, size_t stride, size_t n, int compute_logits, float* logits_out, size_t logits_len,
              const char* who, const ScoreCall* sc, StepTaps* taps) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && tokens, ZG_ERR_ARG, "%s: null argument", who);
    ZG_REQUIRE(g->pass.x != nullptr, ZG_ERR_UNSUPPORTED, "%s: the handle was created with ZG_GPT_NO_PREFILL", who);
    const size_t C = g->cfg.context_size, V = g->cfg.vocab_size, B = g->batch, E = g->cfg.n_embed;
    if (sc) {
        ZG_REQUIRE(g->score.logits != nullptr, ZG_ERR_UNSUPPORTED, "%s: the handle was created without ZG_GPT_SCORE", who);
        ZG_TRY(check_top_n(sc->top_n, V, who));
        ZG_REQUIRE(V <= (size_t)64 * 4096, ZG_ERR_UNSUPPORTED, "%s: vocabulary of %zu beyond %d", who, V, 64 * 4096);
    }
    ZG_REQUIRE(past_len <= g->cached_len, ZG_ERR_ARG, "%s: past_len %zu beyond the %zu cached positions", who, past_len, g->cached_len);
    ZG_REQUIRE(n >= 1 && past_len + n <= C && n <= stride, ZG_ERR_SHAPE, "%s: %zu tokens behind %zu positions (context %zu, stride %zu)", who, n, past_len, C,
               stride);
    ZG_REQUIRE(!logits_out || (compute_logits && logits_len >= B * V), ZG_ERR_SHAPE, "%s: logits_out needs compute_logits and %zu elements", who, B * V);
    ZG_REQUIRE(!sc || !sc->logits_out || sc->logits_len >= B * n * V, ZG_ERR_SHAPE, "%s: logits_out needs %zu elements", who, B * n * V);
    for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < n; ++i) ZG_REQUIRE(tokens[b * stride + i] < V, ZG_ERR_SHAPE, "%s: token %zu >= vocab %zu", who, tokens[b * stride + i], V);
    hipStream_t s = gs(g);
    ZG_HIP(hipStreamSynchronize(s));
    for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < n; ++i) g->h_ints[b * C + past_len + i] = (int)tokens[b * stride + i];
    ZG_HIP(hipMemcpyAsync(g->prompt, g->h_ints, B * C * sizeof(int), hipMemcpyHostToDevice, s));
    const size_t end = past_len + n;
    ZG_TRY(clear_for_pass(g, s, past_len, end));
    g->cached_len = end;
    ZG_TRY(ensure_ln_folded(g, s));
    ZG_TRY(enqueue_prefill(g, past_len, n, compute_logits != 0, s, taps));
    if (compute_logits) {
        ZG_HIP(hipMemcpy2DAsync(g->x, E * 4, g->pass.x + (n - 1) * E, n * E * 4, E * 4, B, hipMemcpyDeviceToDevice, s));
        g->hidden.src = HID_X;
        ZG_TRY(stage_ctrl(g, end - 1, end, 1, s));
        ZG_TRY(enqueue_lm_head(g, s));
        if (logits_out) ZG_TRY(copy_out_f32(logits_out, g->logits, B * V, s));
    }
    if (sc) {  // a log-probability generation with this top_n: the record continues behind it (generate_from) and leaves through the same fetch
        ZG_TRY(stage_top_n(g, sc->top_n, s));
        // column past_len: its predicting row is not part of the pass (NaN: every byte 0xff)
        ZG_HIP(hipMemset2DAsync(g->lp.rec.logprob + past_len, C * sizeof(float), 0xff, sizeof(float), B, s));
        ZG_TRY(enqueue_score(g, past_len, n, sc->logits_out, s, taps));
    }
    ZG_HIP(hipStreamSynchronize(s));
    return check_fault(g);
}

}  // namespace zg

extern "C" {

int zg_gpt_score(zg_gpt* g, size_t past_len, const size_t* tokens, size_t token_stride, size_t n_tokens, size_t top_n, float* logits_out, size_t logits_len) {
    const ScoreCall sc{top_n, logits_out, logits_len};
    return pass_impl(g, past_len, tokens, token_stride, n_tokens, 1, nullptr, 0, "gpt_score", &sc);
}

int zg_gpt_prefill(zg_gpt* g, const size_t* tokens, size_t token_stride, size_t n_tokens, int compute_logits, float* logits_out, size_t logits_len) {
    return pass_impl(g, 0, tokens, token_stride, n_tokens, compute_logits, logits_out, logits_len, "gpt_prefill");
}

int zg_gpt_extend(zg_gpt* g, size_t past_len, const size_t* tokens, size_t token_stride, size_t n_tokens, int compute_logits, float* logits_out,
                  size_t logits_len) {
    return pass_impl(g, past_len, tokens, token_stride, n_tokens, compute_logits, logits_out, logits_len, "gpt_extend");
}

}  // extern "C"
