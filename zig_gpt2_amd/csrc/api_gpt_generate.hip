// api_gpt_generate.hip — model tier of the C ABI: drawing tokens from a handle.  The per-token calls (sample_impl) and the
// generation request, which exists once (every zg_gpt_generate*_enqueue fills a zg_generate_request, generate_request alone
// makes the GenRequest gen_run runs); a whole generation is enqueued without a host round trip per token.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "api_gpt.h"

using namespace zg;

namespace zg {  // offered to the other units: api_gpt.h declares them

// top_n of the record the call in flight writes, through its pinned word into the arena: from here on a fetch finds that record
int stage_top_n(zg_gpt* g, size_t top_n, hipStream_t s) {
    g->lp.valid = true;
    g->lp.top_n = top_n;
    *g->lp.h_top = (int)top_n;
    ZG_HIP(hipMemcpyAsync(g->lp.top, g->lp.h_top, sizeof(int), hipMemcpyHostToDevice, s));
    return ZG_OK;
}

}  // namespace zg

extern "C" {

// The set built in edit.build through its pinned mirror into the arena.  PRECONDITION: nothing in flight reads the mirror (every
// edited call drains, or begins by draining).
static int stage_edits(zg_gpt* g, hipStream_t s) {
    const size_t bytes = g->edit.build.size();
    memcpy(g->edit.h_block, g->edit.build.data(), bytes);
    ZG_HIP(hipMemcpyAsync(g->edit.tab, g->edit.h_block, bytes, hipMemcpyHostToDevice, s));
    return ZG_OK;
}

// The rules laid out in ban.build through their pinned mirror into the arena; the precondition is stage_edits'.
static int stage_bans(zg_gpt* g, hipStream_t s) {
    memcpy(g->ban.h_rules, &g->ban.build, sizeof(BanRules));
    ZG_HIP(hipMemcpyAsync(g->ban.rules, g->ban.h_rules, sizeof(BanRules), hipMemcpyHostToDevice, s));
    return ZG_OK;
}

// the counting kernel keeps a row's distinct tokens in an LDS table sized by the context
static int check_pen_handle(const zg_gpt* g, const char* who) {
    ZG_REQUIRE(g->cfg.context_size <= (size_t)kPenMaxHistory, ZG_ERR_UNSUPPORTED, "%s: context_size %zu beyond the %d tokens the penalty kernel's LDS table holds",
               who, g->cfg.context_size, kPenMaxHistory);
    return ZG_OK;
}

// A caller's token lists for the penalties ([batch][stride], lens[b] each; tokens null: no lists): lengths within the stride and,
// with `extra` more tokens to come from the loop's own record, within the context; tokens inside the vocabulary
static int check_history(const zg_gpt* g, const size_t* tokens, size_t stride, const size_t* lens, size_t extra, const char* who) {
    if (!tokens) {
        for (size_t b = 0; lens && b < g->batch; ++b) ZG_REQUIRE(lens[b] == 0, ZG_ERR_ARG, "%s: row %zu lists %zu tokens but the lists are null", who, b, lens[b]);
        return ZG_OK;
    }
    ZG_REQUIRE(lens != nullptr, ZG_ERR_ARG, "%s: token lists without their lengths", who);
    const size_t C = g->cfg.context_size, V = g->cfg.vocab_size;
    for (size_t b = 0; b < g->batch; ++b) {
        ZG_REQUIRE(lens[b] <= stride && lens[b] <= C && lens[b] + extra <= C, ZG_ERR_SHAPE, "%s: row %zu lists %zu tokens (stride %zu, context %zu, %zu to come)",
                   who, b, lens[b], stride, C, extra);
        for (size_t i = 0; i < lens[b]; ++i)
            ZG_REQUIRE(tokens[b * stride + i] < V, ZG_ERR_SHAPE, "%s: token %zu >= vocab %zu", who, tokens[b * stride + i], V);
    }
    return ZG_OK;
}

// The penalties of the call — pp[batch], one entry per row as plan_rows fills them — and its token lists (checked) through their
// pinned mirrors into the arena.  PRECONDITION: nothing in flight reads the mirrors (every penalised call drains, or begins by draining).
static int stage_penalties(zg_gpt* g, const PenParams* pp, const size_t* tokens, size_t stride, const size_t* lens, hipStream_t s) {
    const size_t C = g->cfg.context_size, B = g->batch;
    memcpy(g->pen.h_params, pp, B * sizeof(PenParams));
    int* h_len = g->pen.h_prior + B * C;
    for (size_t b = 0; b < B; ++b) {
        h_len[b] = tokens ? (int)lens[b] : 0;
        for (size_t i = 0; tokens && i < lens[b]; ++i) g->pen.h_prior[b * C + i] = (int)tokens[b * stride + i];
    }
    ZG_HIP(hipMemcpyAsync(g->pen.params, g->pen.h_params, B * sizeof(PenParams), hipMemcpyHostToDevice, s));
    if (tokens) ZG_HIP(hipMemcpyAsync(g->pen.prior, g->pen.h_prior, B * C * sizeof(int), hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(g->pen.prior_len, h_len, B * sizeof(int), hipMemcpyHostToDevice, s));
    return ZG_OK;
}

// GPT.sample (main.zig:198-207) behind one forward step: the checked body of the per-token family, under the name of the entry
// point that calls it; each entry point keeps in front what it is stricter about.  rows [batch]: the table of the call (a uniform
// entry point's: equal entries, per_row false — its plain sampler takes the temperature by value and stages nothing); with_history:
// the history is the caller's to get right (penalties were given / a row is penalised), else it is not read; an entry point without
// edits passes kNoEdits.  Everything the chain reads is staged first: the chain only launches.
static const zg_logit_edits kNoEdits{};
static int sample_impl(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, const zg_row_sampling* rows, bool per_row, bool with_history,
                       const size_t* history, size_t history_stride, const size_t* history_lens, const zg_logit_edits* edits, const float* uniforms,
                       size_t* tokens_out, float* probs_out, size_t probs_len, const char* who) {
    if (with_history) {
        ZG_TRY(check_pen_handle(g, who));
        ZG_TRY(check_history(g, history, history_stride, history_lens, 0, who));
    }
    bool edit_on = false;
    ZG_TRY(build_edits(edits, g->cfg.vocab_size, who, g->edit.build.data(), &edit_on));
    SampleParams sp[kRowsMax];
    PenParams pp[kRowsMax];
    StepTail plan;
    ZG_TRY(plan_rows(rows, g->batch, g->cfg.vocab_size, 0, who, sp, pp, nullptr, &plan));
    const bool pen_on = plan.pen;
    const SamplerMode mode = plan.sampler;
    if (pen_on || edit_on) ZG_HIP(hipStreamSynchronize(gs(g)));  // (an enqueued generation may still be reading the pinned mirrors; idle otherwise)
    ZG_REQUIRE(tokens && tokens_out, ZG_ERR_ARG, "gpt_sample: bad argument");
    const size_t V = g->cfg.vocab_size, B = g->batch;
    ZG_REQUIRE(!probs_out || probs_len >= B * V, ZG_ERR_SHAPE, "gpt_sample: probs_out needs %zu elements", B * V);
    for (size_t b = 0; uniforms && b < B; ++b)  // (checked before anything is enqueued)
        ZG_REQUIRE(uniforms[b] >= 0.0f && uniforms[b] < 1.0f, ZG_ERR_ARG, "gpt_sample: uniform %f outside [0,1)", uniforms[b]);
    ZG_TRY(forward_enqueue(g, seq_len, tokens, n_tokens, 1, nullptr, 0));  // main.zig:199 (not drained: the sampler goes behind it)
    hipStream_t s = gs(g);
    if (pen_on) ZG_TRY(stage_penalties(g, pp, history, history_stride, history_lens, s));
    if (edit_on) ZG_TRY(stage_edits(g, s));
    float* h_u = g->h_ctrl->uniforms;  // (pinned: h_ints[0 .. B) is still being read by the forward's token upload)
    // (no uniforms: the counter PRNG the device loop's sampler draws from, zg_common.h — of the row's own seed)
    for (size_t b = 0; b < B; ++b) h_u[b] = uniforms ? uniforms[b] : counter_uniform(sp[b].seed, seq_len, b);
    SamplerChain c = handle_chain(g, false);
    float* d_u = g->q;  // scratch: q is dead after the forward
    ZG_HIP(hipMemcpyAsync(d_u, h_u, B * sizeof(float), hipMemcpyHostToDevice, s));
    // (samp.h_params: nothing in flight reads it, forward_enqueue's callers drain; a uniform plain sampler takes its temperature by value)
    memcpy(g->samp.h_params, sp, B * sizeof(SampleParams));
    if (threshold_sampler(mode) || per_row) ZG_HIP(hipMemcpyAsync(g->samp.params, g->samp.h_params, B * sizeof(SampleParams), hipMemcpyHostToDevice, s));
    c.u = d_u, c.temp = rows[0].options.temp, c.per_row = per_row, c.write_probs = probs_out != nullptr, c.pick = g->cur_token;
    ZG_TRY(emit_sampler_chain(c, StepTail{mode, pen_on, false, false, edit_on}, s));  // main.zig:200-206
    ZG_HIP(hipMemcpyAsync(g->h_ints + B, g->cur_token, B * sizeof(int), hipMemcpyDeviceToHost, s));
    if (probs_out) ZG_TRY(copy_out_f32(probs_out, g->logits, B * V, s));
    ZG_HIP(hipStreamSynchronize(s));
    ZG_TRY(check_fault(g));
    for (size_t b = 0; b < B; ++b) tokens_out[b] = (size_t)g->h_ints[B + b];
    return ZG_OK;
}

// The uniform entry points of the family: what they have always checked first, then the table of `batch` equal rows.  penalties
// null: none, the history is not read.
static int sample_uniform(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, const zg_sample_options* opt, const zg_logit_penalties* pen,
                          const size_t* history, size_t history_stride, const size_t* history_lens, const zg_logit_edits* edits, const float* uniforms,
                          uint64_t seed, size_t* tokens_out, float* probs_out, size_t probs_len, const char* who) {
    ZG_TRY(require_init());
    ZG_TRY(check_sample_options(opt, who));
    ZG_REQUIRE(g != nullptr, ZG_ERR_ARG, "%s: null handle", who);
    if (pen) ZG_TRY(check_penalties(pen, who));
    zg_row_sampling rows[kRowsMax];
    // (a min_p that build_edits is about to refuse travels no further than that refusal)
    const float min_p = edits && edits->min_p >= 0.0f && edits->min_p < 1.0f ? edits->min_p : 0.0f;
    uniform_rows(rows, g->batch, *opt, min_p, pen, seed);
    return sample_impl(g, seq_len, tokens, n_tokens, rows, false, pen != nullptr, history, history_stride, history_lens, edits, uniforms, tokens_out,
                       probs_out, probs_len, who);
}

// Beside rows nothing else may say what the sampler does: the edits of a per-row call carry lists only
static int check_each_args(const zg_gpt* g, const zg_row_sampling* rows, size_t n_rows, const zg_logit_edits* edits, const char* who) {
    ZG_REQUIRE(g != nullptr, ZG_ERR_ARG, "%s: null handle", who);
    ZG_REQUIRE(rows != nullptr, ZG_ERR_ARG, "%s: rows is null", who);
    ZG_REQUIRE(n_rows == g->batch, ZG_ERR_ARG, "%s: %zu rows for a handle of batch %zu", who, n_rows, g->batch);
    ZG_REQUIRE(!edits || edits->min_p == 0.0f, ZG_ERR_ARG, "%s: edits->min_p %f beside rows (min-p is the row's)", who, edits->min_p);
    return ZG_OK;
}

int zg_gpt_sample_each(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, const zg_row_sampling* rows, size_t n_rows, const size_t* history,
                       size_t history_stride, const size_t* history_lens, const zg_logit_edits* edits, const float* uniforms, size_t* tokens_out,
                       float* probs_out, size_t probs_len) {
    ZG_TRY(require_init());
    ZG_TRY(check_each_args(g, rows, n_rows, edits, "gpt_sample_each"));
    StepTail plan;
    ZG_TRY(plan_rows(rows, n_rows, g->cfg.vocab_size, 0, "gpt_sample_each", nullptr, nullptr, nullptr, &plan));
    return sample_impl(g, seq_len, tokens, n_tokens, rows, true, plan.pen, history, history_stride, history_lens, edits ? edits : &kNoEdits, uniforms,
                       tokens_out, probs_out, probs_len, "gpt_sample_each");
}

int zg_gpt_sample(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, float temp, const float* uniforms,
                  uint64_t seed, size_t* tokens_out, float* probs_out, size_t probs_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(temp > 0.0f, ZG_ERR_ARG, "gpt_sample: bad argument");
    const zg_sample_options plain{temp, 0, 1.0f};
    return sample_uniform(g, seq_len, tokens, n_tokens, &plain, nullptr, nullptr, 0, nullptr, &kNoEdits, uniforms, seed, tokens_out, probs_out, probs_len,
                       "gpt_sample");
}

// zg_gpt_sample behind top-k / nucleus truncation (filters off: exactly zg_gpt_sample's launches)
int zg_gpt_sample_ex(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, const zg_sample_options* opt, const float* uniforms,
                     uint64_t seed, size_t* tokens_out, float* probs_out, size_t probs_len) {
    return sample_uniform(g, seq_len, tokens, n_tokens, opt, nullptr, nullptr, 0, nullptr, &kNoEdits, uniforms, seed, tokens_out, probs_out, probs_len,
                       "gpt_sample_ex");
}

// ... with the penalty stage in front, on the caller's history: here the penalties are required
int zg_gpt_sample_pen(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, const zg_sample_options* opt, const zg_logit_penalties* pen,
                      const size_t* history, size_t history_stride, const size_t* history_lens, const float* uniforms, uint64_t seed, size_t* tokens_out,
                      float* probs_out, size_t probs_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(pen != nullptr, ZG_ERR_ARG, "gpt_sample_pen: penalties is null");
    return sample_uniform(g, seq_len, tokens, n_tokens, opt, pen, history, history_stride, history_lens, &kNoEdits, uniforms, seed, tokens_out, probs_out,
                       probs_len, "gpt_sample_pen");
}

// ... and with the edit stage behind the penalties and min-p in the sampler: here the edits are required
int zg_gpt_sample_edit(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, const zg_sample_options* opt, const zg_logit_penalties* pen,
                       const size_t* history, size_t history_stride, const size_t* history_lens, const zg_logit_edits* edits, const float* uniforms,
                       uint64_t seed, size_t* tokens_out, float* probs_out, size_t probs_len) {
    return sample_uniform(g, seq_len, tokens, n_tokens, opt, pen, history, history_stride, history_lens, edits, uniforms, seed, tokens_out, probs_out,
                       probs_len, "gpt_sample_edit");
}

// A generation in three parts, so that several handles' generations can be fed to their streams side by side
// (zg_gpt_generate_enqueue_many): gen_begin — prompts, cache clearing, the whole-prompt pass, the prefetcher's start;
// gen_pump — ONE graph launch (graph.steps decode steps) or one single step, false when nothing is left; gen_end — the
// prefetcher's stop word and the record of the last pick.  After a successful gen_begin, gen_end must run (also on failure:
// the prefetcher must not wait for steps that never come).  A generation with stop conditions is the same three parts:
// gen_pump paces itself by the stop stage's progress word and feeds nothing once every row has finished (stop_pace), and gen_end
// sets the handle's lengths to the column actually reached.
// past > 0 (zg_gpt_generate_from_enqueue): the loop is entered at s = past — `prompts` are the new tokens of each row, device
// prompt[b][past + i], prompt_len[b] = past + prompt_lens[b]; everything the embed kernel and gen_pump compare is absolute, so the
// steps are the ones an uninterrupted generation would run at these positions.  The caches keep rows 0 .. past - 1 and the
// recorded tokens of positions below past stay where they are (zg_gpt_generate_fetch_range).

// What a generation is asked for, checked: what generate_request makes of a zg_generate_request for gen_begin
struct GenRequest {
    const size_t* prompts;  // [rows][stride], lens[rows] tokens each
    size_t stride;
    const size_t* lens;
    size_t n_steps, past;
    SamplerMode mode = GREEDY;  // GREEDY (sp unused), or the sampler the chain is launched as (plan_rows: the union of the rows' needs)
    SampleParams sp[kRowsMax];  // ... and each row's parameters as the kernels read them, for the ONE handle a sampler request goes to
    // penalties (a sampler only; pen_on false: none, the request is what it was without them), pp: each row's; and the caller's prior
    // of every row of that handle: [rows][prior_stride], prior_lens[rows] tokens each, or null
    bool pen_on = false;
    PenParams pp[kRowsMax];
    const size_t* prior = nullptr;
    size_t prior_stride = 0;
    const size_t* prior_lens = nullptr;
    // the log-probability stage behind every pick with top_n alternatives; lp_on false: the request is what it was
    bool lp_on = false;
    size_t top_n = 0;
    // stop conditions, checked (check_stop); stop_on false: the request is what it was
    bool stop_on = false;
    zg_stop_conditions stop{};
    // logit edits, checked, the set built in the ONE handle's edit.build: edit_on — the
    // edit stage runs (min-p is the sampler's: in sp).  Off: the request is what it was
    bool edit_on = false;
    // guided decoding: guide_call — the request came through zg_gpt_generate_guided_enqueue (the state record is the
    // call's to fill); guide_on — some row is guided: the mask and the advance run, from guide_state[b] (-1: the row has no guide).
    // Off: the request is what it was
    bool guide_call = false, guide_on = false;
    int guide_state[kRowsMax];
    // history-dependent bans, checked, the rules laid out in the ONE handle's ban.build: ban_on — the ban stage runs, on
    // the history the penalties read (prior, above).  Off: the request is what it was
    bool ban_on = false;
    // beam search, checked (check_beam): the greedy slot plus the log-probability stage (lp_on, top_n = 2 W, set by the
    // builder) with the beam launch and the cache fork behind it.  Off: the request is what it was
    bool beam_on = false;
    zg_beam_options beam{};
    GenRequest(const size_t* prompts, size_t stride, const size_t* lens, size_t n_steps, size_t past = 0)
        : prompts(prompts), stride(stride), lens(lens), n_steps(n_steps), past(past) {}
};

// Steps the host may be ahead of the stop stage's progress word before it feeds the next piece, where the caller names none:
// the smallest value whose rate is inside the run-to-run spread of an unpaced loop (tools/bench_stop.py)
constexpr size_t kStopLookahead = 16;

static int gen_begin(zg_gpt* g, const GenRequest& r) {
    const size_t n_steps = r.n_steps, past = r.past;
    ZG_REQUIRE(g && r.prompts && r.lens, ZG_ERR_ARG, "generate: null argument");
    const size_t C = g->cfg.context_size, V = g->cfg.vocab_size, B = g->batch;
    ZG_REQUIRE(past <= g->cached_len, ZG_ERR_ARG, "generate: past_len %zu beyond the %zu cached positions", past, g->cached_len);
    ZG_REQUIRE(n_steps >= 1 && past + n_steps <= C, ZG_ERR_SHAPE, "generate: n_steps %zu outside 1..%zu", n_steps, C - past);
    for (size_t b = 0; b < B; ++b) {  // (everything is checked before the handle's state is touched)
        const size_t np = r.lens[b];
        ZG_REQUIRE(np >= 1 && past + np <= C && np <= r.stride, ZG_ERR_SHAPE, "generate: prompt %zu has length %zu", b, np);
        for (size_t i = 0; i < np; ++i)
            ZG_REQUIRE(r.prompts[b * r.stride + i] < V, ZG_ERR_SHAPE, "generate: token %zu >= vocab %zu", r.prompts[b * r.stride + i], V);
    }
    const bool pen_on = r.pen_on && r.mode != GREEDY;
    const bool ban_on = r.ban_on && r.mode != GREEDY;
    if (pen_on || ban_on) {  // (a row's history, prior and recorded, never exceeds the context: the kernels' LDS is sized by it)
        ZG_TRY(check_pen_handle(g, "generate_pen"));
        ZG_TRY(check_history(g, r.prior, r.prior_stride, r.prior_lens, n_steps, "generate_pen"));
    }
    if (r.lp_on) {
        ZG_TRY(check_top_n(r.top_n, V, "generate_logprobs"));
        ZG_REQUIRE(V <= (size_t)64 * 4096, ZG_ERR_UNSUPPORTED, "generate_logprobs: vocabulary of %zu beyond %d", V, 64 * 4096);
    }
    hipStream_t s = gs(g);
    ZG_HIP(hipStreamSynchronize(s));  // pinned staging below is shared with earlier calls
    size_t min_prompt = C;
    memset(g->h_ints, 0, (B * C + B) * sizeof(int));
    for (size_t b = 0; b < B; ++b) {
        const size_t np = r.lens[b];
        for (size_t i = 0; i < np; ++i) g->h_ints[b * C + past + i] = (int)r.prompts[b * r.stride + i];
        g->h_ints[B * C + b] = (int)(past + np);
        if (np < min_prompt) min_prompt = np;
    }
    // The positions every sequence has a prompt token for go through the Blocks together (prefill); the
    // rest of the loop is main.zig:330-338 one position at a time.
    size_t first = 0;
    if (g->pass.x != nullptr && min_prompt >= prefill_min())
        first = min_prompt < n_steps ? min_prompt : n_steps;
    const bool edit_on = r.edit_on && r.mode != GREEDY;
    const bool guide_on = r.guide_on && r.mode != GREEDY;
    g->gen.tail = normalized(StepTail{r.mode, pen_on, r.lp_on, r.stop_on, edit_on, guide_on, ban_on, r.beam_on}, true);  // (normalized: pen_on / edit_on / guide_on / ban_on only with a sampler, and the steps it is for have lm_head)
    g->gen.stop_valid = false;
    g->gen.stop = r.stop_on;
    g->beam.valid = false;
    if (r.beam_on) {  // the options and the groups' start state through the pinned control block, lenpow through the record's mirror (the stream is drained)
        const size_t c0 = past + r.lens[0];
        fill_beam_state(g->beam.h_state, r.beam, c0);
        ZG_HIP(hipMemcpyAsync(g->beam.state, g->beam.h_state, sizeof(BeamState), hipMemcpyHostToDevice, s));
        fill_lenpow(g->lp.h_rec, C + 1, r.beam.length_penalty);
        ZG_HIP(hipMemcpyAsync(g->beam.lenpow, g->lp.h_rec, (C + 1) * sizeof(float), hipMemcpyHostToDevice, s));
        g->beam.valid = true;
        g->beam.W = r.beam.num_beams;
        g->beam.c0 = c0;
        g->beam.has_eos = r.beam.eos_id != ZG_BEAM_NO_EOS;
        g->beam.length_penalty = r.beam.length_penalty;
        if (g->beam.has_eos) {  // the beam stage ends the call early the way the stop stage does: the same two words, the same pacing
            g->gen.stop = true;
            g->stop.pinned->host.progress = g->stop.pinned->host.done_col = 0u;
            g->gen.lookahead = r.beam.lookahead ? std::min(r.beam.lookahead, C) : kStopLookahead;
        }
    }
    if (r.stop_on) {  // the conditions of this call; no row has finished; the stage has seen nothing (the stream is drained: the words are the host's)
        fill_stop(&g->stop.pinned->conds, r.stop);
        ZG_HIP(hipMemcpyAsync(g->stop.conds, &g->stop.pinned->conds, sizeof(StopConds), hipMemcpyHostToDevice, s));
        ZG_HIP(hipMemsetAsync(g->stop.fin, 0xff, kStopMaxRows * 4, s));
        ZG_HIP(hipMemsetAsync(g->stop.reason, 0xff, kStopMaxRows * 4, s));
        g->stop.pinned->host.progress = g->stop.pinned->host.done_col = 0u;
        g->gen.lookahead = r.stop.lookahead ? std::min(r.stop.lookahead, C) : kStopLookahead;  // (beyond the context: never waits)
    }
    if (r.mode != GREEDY) {
        memcpy(g->samp.h_params, r.sp, B * sizeof(SampleParams));
        ZG_HIP(hipMemcpyAsync(g->samp.params, g->samp.h_params, B * sizeof(SampleParams), hipMemcpyHostToDevice, s));
    }
    if (pen_on || ban_on) ZG_TRY(stage_penalties(g, r.pp, r.prior, r.prior_stride, r.prior_lens, s));  // (the prior is the history of both stages)
    if (ban_on) ZG_TRY(stage_bans(g, s));
    if (edit_on) ZG_TRY(stage_edits(g, s));
    g->guide.valid = false;
    if (r.guide_call) {  // the new columns record "none" (every byte 0xff) until the advance of a guided row's picked column says otherwise
        ZG_HIP(hipMemset2DAsync(g->guide.rec + past, C * sizeof(int), 0xff, n_steps * sizeof(int), B, s));
        g->guide.valid = true;
    }
    if (guide_on) {  // every row's start state through the pinned control block (the stream is drained: the mirror is the host's)
        memcpy(g->guide.h_state, r.guide_state, B * sizeof(int));
        ZG_HIP(hipMemcpyAsync(g->guide.state, g->guide.h_state, B * sizeof(int), hipMemcpyHostToDevice, s));
    }
    g->lp.valid = false;
    if (r.lp_on) {
        ZG_TRY(stage_top_n(g, r.top_n, s));
        // the new columns no step with lm_head reaches (the whole-prompt pass, steps that only feed a prompt token) record prompt
        // tokens: NaN (every byte 0xff); the stage itself writes the NaN of a longer row's prompt columns
        const size_t fed = std::min(min_prompt, n_steps);
        ZG_HIP(hipMemset2DAsync(g->lp.rec.logprob + past, C * sizeof(float), 0xff, fed * sizeof(float), B, s));
    }
    ZG_HIP(hipMemcpyAsync(g->prompt, g->h_ints, B * C * sizeof(int), hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(g->prompt_len, g->h_ints + B * C, B * sizeof(int), hipMemcpyHostToDevice, s));
    ZG_TRY(stage_ctrl(g, past + first, past + first, r.mode != GREEDY || r.beam_on ? 2 : 0, s));  // (mode 2: the embed kernel feeds `sampled`, the sampler's or the beam stage's)
    ZG_TRY(clear_for_pass(g, s, past, past + first));
    g->cached_len = g->kv_dirty_hi = past + n_steps;  // the last position the loop feeds
    ZG_TRY(ensure_ln_folded(g, s));
    if (first > 0) {
        if (past == 0) ZG_HIP(hipMemcpyAsync(g->out_tokens, g->prompt, B * C * sizeof(int), hipMemcpyDeviceToDevice, s));
        else  // only the new columns: the tokens recorded below past stay
            ZG_HIP(hipMemcpy2DAsync(g->out_tokens + past, C * sizeof(int), g->prompt + past, C * sizeof(int), first * sizeof(int), B, hipMemcpyDeviceToDevice, s));
        ZG_TRY(enqueue_prefill(g, past, first, false, s));
    }
    // Every graph the loop will replay exists before the prefetcher starts its idle clock (a capture between the steps would run
    // against it): all of create's on a stream create did not see, and this generation's own tail — whatever create did not
    // capture of it (graph_exec skips what exists) — for the buckets of its steps with lm_head
    if (!(g->flags & ZG_GPT_NO_GRAPH) && s != nullptr) {
        if (g->graph.stream != s) ZG_TRY(capture_all(g, s));
        if (!(g->gen.tail == StepTail{}) && min_prompt < n_steps)
            ZG_TRY(capture_tail(g, g->gen.tail, bucket_of(past + std::max(first, min_prompt) + 1), bucket_of(past + n_steps), s));
    }
    ZG_TRY(note_steps(g, n_steps, s));
    ZG_TRY(pf_start(g, past + n_steps, s));
    g->gen.pos = past + first;  // absolute, as gen.n and gen.min_prompt: gen_pump's steps, buckets and graph alignment follow the position
    g->gen.n = past + n_steps;
    g->gen.min_prompt = past + min_prompt;
    g->gen.since_sync = 0;
    g->gen.open = true;
    return ZG_OK;
}

// A stop generation before each piece it feeds: *ended when every row has finished — nothing more is fed —, else
// wait while the host is more than gen.lookahead steps ahead of the stop stage.  The stage counts steps with lm_head only, so the
// steps below gen.min_prompt (the default tail) are not paced over.  progress is read BEFORE done_col and the kernel stores them
// the other way round: a done_col still 0 then means that the finishing step had not announced itself when progress was read, which
// is what bounds `end`.  The wait is bounded by the device's state, not by a count: whenever the word has stood still over 16 polls
// the stream is asked, and a drained or failed stream ends the wait — a faulted device ends the call instead of spinning the host.
static int stop_pace(zg_gpt* g, hipStream_t s, bool* ended) {
    StopHost* const h = &g->stop.pinned->host;
    *ended = false;
    unsigned seen = ~0u;  // progress at the last look at the stream
    for (unsigned polls = 0;; ++polls) {
        const unsigned p = __atomic_load_n(&h->progress, __ATOMIC_ACQUIRE);
        const unsigned d = __atomic_load_n(&h->done_col, __ATOMIC_ACQUIRE);
        if (d != 0u) {
            *ended = true;
            return ZG_OK;
        }
        if (g->gen.pos <= std::max((size_t)p, g->gen.min_prompt) + g->gen.lookahead) return ZG_OK;
        if (polls < 64) continue;  // (a short wait costs no system call)
        if (polls % 16 == 0) {  // the stream is asked only while the word stands still: a healthy device moves it every step
            if (p == seen) {
                const hipError_t q = hipStreamQuery(s);
                if (q != hipErrorNotReady) {
                    if (q != hipSuccess) return hip_fail(q, "hipStreamQuery(stop generation)", __FILE__, __LINE__);
                    if (__atomic_load_n(&h->progress, __ATOMIC_ACQUIRE) == p) return ZG_OK;  // drained and nothing moved: nothing will
                }
            }
            seen = p;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

static int gen_pump(zg_gpt* g, bool* more) {
    hipStream_t s = gs(g);
    const size_t C = g->cfg.context_size, n_steps = g->gen.n, st = g->gen.pos;
    *more = false;
    if (st >= n_steps) return ZG_OK;
    if (g->gen.stop && st > g->gen.min_prompt) {  // (behind the first step with lm_head: nothing can have finished before)
        bool ended = false;
        ZG_TRY(stop_pace(g, s, &ended));
        if (ended) return ZG_OK;
    }
    const size_t K = ((g->flags & ZG_GPT_NO_GRAPH) || s == nullptr) ? 1 : g->graph.steps;
    // ZGPT2_SYNC_EVERY=n (profiling only): drain the stream every n steps — rocprofv3's counter collection has crashed
    // on this stack when tens of thousands of dispatches were queued ahead of it
    static const int sync_every = env_int("ZGPT2_SYNC_EVERY", 0);
    if (sync_every > 0 && ++g->gen.since_sync >= (size_t)sync_every) {
        g->gen.since_sync = 0;
        (void)hipStreamSynchronize(s);
    }
    if (K > 1 && st >= g->gen.min_prompt && st % K == 0 && st + K <= n_steps && st + K <= C) {
        if (g->graph.stream != s) ZG_TRY(capture_all(g, s));
        hipGraphExec_t e;  // sequence lengths st + 1 .. st + K share a bucket (K divides 64); captured by gen_begin (first use: the backstop)
        ZG_TRY(graph_exec(g, {true, true, g->gen.tail}, bucket_of(st + 1), s, &e));
        ZG_HIP(hipGraphLaunch(e, s));
        g->hidden.src = HID_X;
        g->gen.pos = st + K;
    } else {
        ZG_TRY(run_step(g, st >= g->gen.min_prompt, st + 1, s, g->gen.tail));
        g->gen.pos = st + 1;
    }
    *more = g->gen.pos < n_steps;
    return ZG_OK;
}

// gen_pump until nothing is left or it fails
static int gen_pump_all(zg_gpt* g) {
    int rs = ZG_OK;
    for (bool more = true; more && rs == ZG_OK;) rs = gen_pump(g, &more);
    return rs;
}

static int gen_end(zg_gpt* g, int rs) {
    hipStream_t s = gs(g);
    g->gen.open = false;
    ZG_TRY(pf_stop(g, s));  // also after a failed launch: the prefetcher must not wait for steps that never come
    ZG_TRY(rs);
    ZG_TRY(launch_embed_step(embed_args(g, 1), s));  // record the pick of the last step
    if (g->gen.stop) {  // the column actually reached: the one place that corrects what gen_begin set up front
        g->gen.n = g->cached_len = g->kv_dirty_hi = g->gen.stop_end = g->gen.pos;
        g->gen.stop_valid = !g->gen.tail.beam;  // (a beam generation ends early by its pools: it has no finish columns to report)
    }
    g->steps_enqueued = g->gen.n;
    return ZG_OK;
}

// One request for the rows of n handles, handle by handle: gen_begin for each, the pumps side by side, gen_end for each that began.
// Several handles: every handle decodes its own prompts on its own stream and the chip overlaps the chains, each of which leaves
// it idle across every one of its launch boundaries.  The handles are fed side by side: a hardware queue holds a fraction of a
// generation's dispatches, and a host that fed one handle to the end first would block on that queue while the others idle.
static int gen_run(zg_gpt* const* handles, size_t n_handles, GenRequest req) {
    size_t begun = 0;
    int rs = ZG_OK;
    for (; begun < n_handles && rs == ZG_OK; ++begun) {
        rs = gen_begin(handles[begun], req);
        if (rs != ZG_OK) break;  // (its message is picked up below)
        req.prompts += handles[begun]->batch * req.stride;
        req.lens += handles[begun]->batch;
    }
    char msg[512] = "";
    if (rs == ZG_OK && begun > 1) {
        // one feeder thread per handle: a hipGraphLaunch returns only when its hardware queue has room for the graph's
        // dispatches, so one thread feeding all queues in turn stands still whenever the slowest chain's queue is full
        std::vector<std::thread> th;
        std::vector<int> res(begun, ZG_OK);
        std::vector<std::string> errs(begun);
        const int dev = ctx().device;
        for (size_t i = 0; i < begun; ++i)
            th.emplace_back([&, i]() {
                res[i] = hipSetDevice(dev) == hipSuccess ? gen_pump_all(handles[i]) : ZG_ERR_HIP;
                if (res[i] != ZG_OK) errs[i] = zg_last_error();  // (the message is thread-local)
            });
        for (auto& t : th) t.join();
        for (size_t i = 0; i < begun && rs == ZG_OK; ++i)
            if (res[i] != ZG_OK) {
                rs = res[i];
                snprintf(msg, sizeof msg, "%s", errs[i].c_str());
            }
    } else {  // one handle: the calling thread pumps
        if (rs == ZG_OK) rs = gen_pump_all(handles[0]);
        if (rs != ZG_OK) snprintf(msg, sizeof msg, "%s", zg_last_error());
    }
    int first_err = rs;
    for (size_t i = 0; i < begun; ++i) {
        const int e = gen_end(handles[i], rs);
        if (first_err == ZG_OK && e != ZG_OK) {
            first_err = e;
            snprintf(msg, sizeof msg, "%s", zg_last_error());
        }
    }
    if (first_err != ZG_OK) set_error("%s", msg);
    return first_err;
}

// Everything of the generate family in one place: the one builder of a GenRequest, for every zg_gpt_generate*_enqueue entry point
// under its own name.  Each stage is a node of graphs of their own, its values in device memory: the selection launches in front of
// the sampler node (StepTail.sampler; filters off: the plain sampler's graphs), the penalty stage (StepTail.pen), the
// log-probability stage behind the sampler node, or behind lm_head of a greedy step (StepTail.lp; it only reads, so
// the tokens are those of the call without it), the stop stage last (StepTail.stop), the edit stage between the
// penalties and the sampler (StepTail.edit; min-p is the sampler's: SampleParams.min_p_off, alone MINP_ONLY).  A
// stage whose argument is null or all off leaves the request what it was without it.  Penalties, conditions and edits go to ONE
// handle, the first (zg_gpt_generate_enqueue_many has none of them).
// each (zg_gpt_generate_each_enqueue): the table of the call, one zg_row_sampling per row of the handle, in the place of q.options /
// q.penalties / q.edits->min_p / q.seed; null: the uniform request, whose table is `batch` equal rows.
// guide (zg_gpt_generate_guided_enqueue): the start state of every row of the handle, which has ZG_GPT_GUIDED_GENERATE; null: no guide.
// bans (zg_gpt_generate_banned_enqueue): the ban rules of the call; null or all off: the request is what it was.
static int generate_request(zg_gpt* const* handles, size_t n_handles, const zg_generate_request& q, const char* who, const zg_row_sampling* each = nullptr,
                            size_t n_each = 0, const size_t* guide = nullptr, const zg_ban_rules* bans = nullptr) {
    ZG_TRY(require_init());
    zg_gpt* const g = handles[0];
    ZG_REQUIRE(g != nullptr, ZG_ERR_ARG, "%s: null argument", who);
    if (each || n_each) {
        ZG_REQUIRE(!q.options && !q.penalties, ZG_ERR_ARG, "%s: options / penalties beside rows (they are the rows')", who);
        ZG_TRY(check_each_args(g, each, n_each, q.edits, who));
    }
    if (q.options) ZG_TRY(check_sample_options(q.options, who));
    ZG_REQUIRE(q.options || !q.penalties, ZG_ERR_ARG, "%s: penalties without sampler options (greedy picking with penalties is top_k = 1)", who);
    GenRequest r(q.prompts, q.prompt_stride, q.prompt_lens, q.n_steps, q.past_len);
    if (q.logprobs) {
        r.lp_on = true;
        r.top_n = q.top_n;
    }
    if (q.penalties) ZG_TRY(check_penalties(q.penalties, who));
    StepTail plan;
    if (each) ZG_TRY(plan_rows(each, n_each, g->cfg.vocab_size, q.past_len, who, r.sp, r.pp, nullptr, &plan));
    if (each ? plan.pen : (q.penalties && !penalties_off(*q.penalties))) {
        r.pen_on = true;
        r.prior = q.prior;
        r.prior_stride = q.prior_stride;
        r.prior_lens = q.prior_lens;
    } else if (q.penalties) {  // all off: the request stays what it was without them, but the lists are still the caller's to get right
        ZG_TRY(check_pen_handle(g, who));
        ZG_TRY(check_history(g, q.prior, q.prior_stride, q.prior_lens, 0, who));
    }
    if (q.stop && (q.stop->n_ids || q.stop->n_seqs)) {
        ZG_REQUIRE(g->batch <= (size_t)kStopMaxRows, ZG_ERR_UNSUPPORTED, "%s: batch %zu above %d", who, g->batch, kStopMaxRows);
        ZG_TRY(check_stop(q.stop, g->cfg.vocab_size, who));
        r.stop_on = true;
        r.stop = *q.stop;
    }
    if (q.edits) {
        ZG_TRY(build_edits(q.edits, g->cfg.vocab_size, who, g->edit.build.data(), &r.edit_on));
        ZG_REQUIRE(q.options || each || edits_off(*q.edits), ZG_ERR_ARG, "%s: edits without sampler options (greedy picking with edits is top_k = 1)", who);
    }
    if (q.options) {  // the uniform table: what plan_rows makes of `batch` equal rows (checked above: it cannot refuse them)
        zg_row_sampling rows[kRowsMax];
        uniform_rows(rows, g->batch, *q.options, q.edits ? q.edits->min_p : 0.0f, q.penalties, q.seed);
        ZG_TRY(plan_rows(rows, g->batch, g->cfg.vocab_size, q.past_len, who, r.sp, r.pp, nullptr, &plan));
    }
    if (q.options || each) r.mode = plan.sampler;
    if (bans) {  // (behind the edits: the rules are judged against the size of the call's own keep set, built above in edit.build)
        ZG_TRY(check_bans(bans, g->batch, g->cfg.vocab_size, g->cfg.context_size, edits_kept(r.edit_on ? g->edit.build.data() : nullptr, g->cfg.vocab_size),
                          q.n_steps, q.prior ? q.prior_lens : nullptr, !q.options && !each, guide != nullptr, who, &r.ban_on));
        if (r.ban_on) {
            fill_bans(&g->ban.build, *bans, g->batch, q.past_len);
            r.prior = q.prior;
            r.prior_stride = q.prior_stride;
            r.prior_lens = q.prior_lens;
        }
    }
    if (guide) {  // (behind the edits: an empty kept set is judged against the call's own keep bitmap, built above in edit.build)
        const unsigned* call_keep = r.edit_on ? reinterpret_cast<const unsigned*>(g->edit.build.data() + sizeof(EditTable)) : nullptr;
        ZG_TRY(check_guide_call(g->guide.loaded ? g->guide.h_keep.data() : nullptr, g->guide.loaded, g->cfg.vocab_size, call_keep, guide, g->batch,
                                !q.options && !each, who, r.guide_state, &r.guide_on));
        r.guide_call = true;
    }
    return gen_run(handles, n_handles, r);
}

// The positional arguments of the entry points as a request; what an entry point does not name is null / 0
static zg_generate_request request_of(size_t past_len, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens, size_t n_steps,
                                      const zg_sample_options* opt = nullptr, uint64_t seed = 0, const zg_logit_penalties* pen = nullptr,
                                      const size_t* prior = nullptr, size_t prior_stride = 0, const size_t* prior_lens = nullptr, int logprobs = 0,
                                      size_t top_n = 0, const zg_stop_conditions* stop = nullptr) {
    return zg_generate_request{sizeof(zg_generate_request), past_len, prompts, prompt_stride, prompt_lens, n_steps, opt, pen, prior, prior_stride, prior_lens, seed,
                               logprobs, top_n, stop, nullptr};  // (the fields in the header's order)
}

int zg_gpt_generate_enqueue(zg_gpt* g, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens, size_t n_steps) {
    return generate_request(&g, 1, request_of(0, prompts, prompt_stride, prompt_lens, n_steps), "generate");
}

// generate (src/main.zig:322-342) AS THE REFERENCE RUNS IT: every token behind the prompt is drawn by GPT.sample
// (main.zig:198-207, :336-338) — softmax(logits / temp), then the first index whose running sum exceeds u x total — with the
// whole loop on the device: the sampler is a node of the captured decode step (sample_step_kernel) and the next step's embed
// kernel feeds its draw.  The uniform of (sequence b, position T) is the counter PRNG of (seed, T, b) that zg_gpt_sample uses when
// it is given no uniforms, so this call returns exactly the tokens of a host loop `tok = zg_gpt_sample(g, T, tok, temp, NULL,
// seed, ...)` — without a host round trip per token.  Results through zg_gpt_generate_fetch.
int zg_gpt_generate_sample_enqueue(zg_gpt* g, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens, size_t n_steps,
                                   float temp, uint64_t seed) {
    ZG_TRY(require_init());
    ZG_REQUIRE(temp > 0.0f, ZG_ERR_ARG, "generate_sample: temperature %f", temp);
    const zg_sample_options plain{temp, 0, 1.0f};
    return generate_request(&g, 1, request_of(0, prompts, prompt_stride, prompt_lens, n_steps, &plain, seed), "generate_sample");
}

int zg_gpt_generate_sample(zg_gpt* g, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens, size_t n_steps, float temp,
                           uint64_t seed, size_t* out_tokens, size_t out_len) {
    ZG_REQUIRE(g && out_tokens && out_len >= g->batch * n_steps, ZG_ERR_SHAPE, "generate_sample: out_tokens too short");
    ZG_TRY(zg_gpt_generate_sample_enqueue(g, prompts, prompt_stride, prompt_lens, n_steps, temp, seed));
    return zg_gpt_generate_fetch(g, n_steps, out_tokens, out_len);
}

// The same behind top-k / nucleus truncation (include/zgpt2.h zg_sample_options; sample_filter.h); here the options are required
int zg_gpt_generate_sample_ex_enqueue(zg_gpt* g, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens, size_t n_steps,
                                      const zg_sample_options* opt, uint64_t seed) {
    ZG_TRY(require_init());
    ZG_REQUIRE(opt != nullptr, ZG_ERR_ARG, "generate_sample_ex: options is null");
    return generate_request(&g, 1, request_of(0, prompts, prompt_stride, prompt_lens, n_steps, opt, seed), "generate_sample_ex");
}

int zg_gpt_generate_sample_ex(zg_gpt* g, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens, size_t n_steps,
                              const zg_sample_options* opt, uint64_t seed, size_t* out_tokens, size_t out_len) {
    ZG_REQUIRE(g && out_tokens && out_len >= g->batch * n_steps, ZG_ERR_SHAPE, "generate_sample_ex: out_tokens too short");
    ZG_TRY(zg_gpt_generate_sample_ex_enqueue(g, prompts, prompt_stride, prompt_lens, n_steps, opt, seed));
    return zg_gpt_generate_fetch(g, n_steps, out_tokens, out_len);
}

// generate entered at s = past_len: the decode loop's own graphs at the absolute positions, the shortest new length
// through the whole-prompt pass first where the handle has one.  options null: greedy.
int zg_gpt_generate_from_enqueue(zg_gpt* g, size_t past_len, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens, size_t n_steps,
                                 const zg_sample_options* opt, uint64_t seed) {
    return generate_request(&g, 1, request_of(past_len, prompts, prompt_stride, prompt_lens, n_steps, opt, seed), "generate_from");
}

// zg_gpt_generate_from_enqueue with penalties; here options and penalties are required
int zg_gpt_generate_pen_enqueue(zg_gpt* g, size_t past_len, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens, size_t n_steps,
                                const zg_sample_options* opt, const zg_logit_penalties* pen, const size_t* prior, size_t prior_stride,
                                const size_t* prior_lens, uint64_t seed) {
    ZG_TRY(require_init());
    ZG_REQUIRE(opt != nullptr && pen != nullptr, ZG_ERR_ARG, "generate_pen: options or penalties is null");
    return generate_request(&g, 1, request_of(past_len, prompts, prompt_stride, prompt_lens, n_steps, opt, seed, pen, prior, prior_stride, prior_lens),
                            "generate_pen");
}

int zg_gpt_generate_logprobs_enqueue(zg_gpt* g, size_t past_len, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens, size_t n_steps,
                                     const zg_sample_options* opt, const zg_logit_penalties* pen, const size_t* prior, size_t prior_stride,
                                     const size_t* prior_lens, uint64_t seed, size_t top_n) {
    return generate_request(&g, 1, request_of(past_len, prompts, prompt_stride, prompt_lens, n_steps, opt, seed, pen, prior, prior_stride, prior_lens, 1, top_n),
                            "generate_logprobs");
}

int zg_gpt_generate_stop_enqueue(zg_gpt* g, size_t past_len, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens, size_t n_steps,
                                 const zg_sample_options* opt, const zg_logit_penalties* pen, const size_t* prior, size_t prior_stride,
                                 const size_t* prior_lens, uint64_t seed, int logprobs, size_t top_n, const zg_stop_conditions* stop) {
    return generate_request(
        &g, 1, request_of(past_len, prompts, prompt_stride, prompt_lens, n_steps, opt, seed, pen, prior, prior_stride, prior_lens, logprobs, top_n, stop),
        "generate_stop");
}

int zg_gpt_generate_request_enqueue(zg_gpt* g, const zg_generate_request* r) {
    ZG_REQUIRE(r != nullptr && r->size == sizeof(zg_generate_request), ZG_ERR_ARG, "generate_request: null request, or its size field is not sizeof(zg_generate_request)");
    return generate_request(&g, 1, *r, "generate_request");
}

int zg_gpt_generate_each_enqueue(zg_gpt* g, const zg_generate_request* r, const zg_row_sampling* rows, size_t n_rows) {
    ZG_REQUIRE(r != nullptr && r->size == sizeof(zg_generate_request), ZG_ERR_ARG, "generate_each: null request, or its size field is not sizeof(zg_generate_request)");
    ZG_REQUIRE(rows != nullptr, ZG_ERR_ARG, "generate_each: rows is null");
    return generate_request(&g, 1, *r, "generate_each", rows, n_rows);
}

// ---- History-dependent bans: the request call or, with rows, the per-row call, plus the rules
int zg_gpt_generate_banned_enqueue(zg_gpt* g, const zg_generate_request* r, const zg_row_sampling* rows, size_t n_rows, const zg_ban_rules* bans) {
    ZG_REQUIRE(r != nullptr && r->size == sizeof(zg_generate_request), ZG_ERR_ARG, "generate_banned: null request, or its size field is not sizeof(zg_generate_request)");
    ZG_REQUIRE(rows != nullptr || n_rows == 0, ZG_ERR_ARG, "generate_banned: %zu rows but rows is null", n_rows);
    return generate_request(&g, 1, *r, "generate_banned", rows, n_rows, nullptr, bans);
}

// ---- Guided decoding

// The table of a handle: checked and turned into bitmaps by build_guide (into a scratch, so that a refused table leaves the loaded
// one standing), then uploaded.  Synchronous; drains first — a generation in flight may be reading what is replaced.
int zg_gpt_guide_load(zg_gpt* g, const zg_guide* guide) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g != nullptr, ZG_ERR_ARG, "guide_load: null handle");
    ZG_REQUIRE(g->flags & ZG_GPT_GUIDED_GENERATE, ZG_ERR_UNSUPPORTED, "guide_load: the handle was created without ZG_GPT_GUIDED_GENERATE");
    const size_t V = g->cfg.vocab_size, words = guide_keep_words(V);
    std::vector<unsigned> keep;
    if (guide) {
        keep.assign((size_t)ZG_GUIDE_MAX_STATES * words, 0u);
        ZG_TRY(build_guide(guide, V, "guide_load", keep.data()));
    }
    hipStream_t s = gs(g);
    ZG_HIP(hipStreamSynchronize(s));
    const int n = guide ? (int)guide->n_states : 0;
    g->guide.loaded = 0;  // (a failed upload leaves no table rather than half of one)
    ZG_HIP(hipMemcpy(g->guide.n_states, &n, sizeof(int), hipMemcpyHostToDevice));
    if (guide) {
        ZG_HIP(hipMemcpy(g->guide.next, guide->next, (size_t)n * V * sizeof(uint16_t), hipMemcpyHostToDevice));
        ZG_HIP(hipMemcpy(g->guide.keep, keep.data(), (size_t)n * words * 4, hipMemcpyHostToDevice));
    }
    ZG_HIP(hipDeviceSynchronize());
    g->guide.h_keep.swap(keep);
    g->guide.loaded = (size_t)n;
    return ZG_OK;
}

int zg_gpt_generate_guided_enqueue(zg_gpt* g, const zg_generate_request* r, const zg_row_sampling* rows, size_t n_rows, const size_t* start_states) {
    ZG_REQUIRE(r != nullptr && r->size == sizeof(zg_generate_request), ZG_ERR_ARG, "generate_guided: null request, or its size field is not sizeof(zg_generate_request)");
    ZG_REQUIRE(g != nullptr, ZG_ERR_ARG, "generate_guided: null handle");
    ZG_REQUIRE(g->flags & ZG_GPT_GUIDED_GENERATE, ZG_ERR_UNSUPPORTED, "generate_guided: the handle was created without ZG_GPT_GUIDED_GENERATE");
    ZG_REQUIRE(start_states != nullptr, ZG_ERR_ARG, "generate_guided: start_states is null");
    ZG_REQUIRE(rows != nullptr || n_rows == 0, ZG_ERR_ARG, "generate_guided: %zu rows but rows is null", n_rows);
    return generate_request(&g, 1, *r, "generate_guided", rows, n_rows, start_states);
}

int zg_gpt_generate_fetch_guide_states(zg_gpt* g, size_t first, size_t n, size_t* states_out, size_t len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && states_out, ZG_ERR_ARG, "generate_fetch_guide_states: null argument");
    ZG_REQUIRE(g->flags & ZG_GPT_GUIDED_GENERATE, ZG_ERR_UNSUPPORTED, "generate_fetch_guide_states: the handle was created without ZG_GPT_GUIDED_GENERATE");
    ZG_REQUIRE(g->guide.valid, ZG_ERR_ARG, "generate_fetch_guide_states: the last generation did not come through zg_gpt_generate_guided_enqueue");
    const size_t C = g->cfg.context_size, B = g->batch;
    ZG_REQUIRE(first <= C && n <= C - first && len >= B * n, ZG_ERR_SHAPE, "generate_fetch_guide_states: positions %zu .. %zu of %zu, %zu elements", first,
               first + n, C, len);
    if (n == 0) return ZG_OK;
    hipStream_t s = gs(g);
    ZG_HIP(hipMemcpyAsync(g->h_ints, g->guide.rec, B * C * sizeof(int), hipMemcpyDeviceToHost, s));
    ZG_HIP(hipStreamSynchronize(s));
    ZG_TRY(check_fault(g));
    for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < n; ++i) {
            const int st = g->h_ints[b * C + first + i];
            states_out[b * n + i] = st < 0 ? ZG_GUIDE_NONE : (size_t)st;
        }
    return ZG_OK;
}

int zg_gpt_generate_stop_result(zg_gpt* g, size_t* end_out, size_t* finish_cols_out, int* reasons_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && end_out && finish_cols_out && reasons_out, ZG_ERR_ARG, "generate_stop_result: null argument");
    ZG_REQUIRE(g->gen.stop_valid, ZG_ERR_ARG, "generate_stop_result: the last generation had no stop conditions");
    hipStream_t s = gs(g);
    ZG_HIP(hipMemcpyAsync(g->stop.pinned->fin, g->stop.fin, g->batch * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipMemcpyAsync(g->stop.pinned->reason, g->stop.reason, g->batch * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipStreamSynchronize(s));
    ZG_TRY(check_fault(g));
    *end_out = g->gen.stop_end;
    for (size_t b = 0; b < g->batch; ++b) {
        const int f = g->stop.pinned->fin[b];
        finish_cols_out[b] = f < 0 ? ZG_STOP_NONE : (size_t)f;
        reasons_out[b] = f < 0 ? -1 : g->stop.pinned->reason[b];
    }
    return ZG_OK;
}

int zg_gpt_generate_fetch_logprobs(zg_gpt* g, size_t first, size_t n, size_t top_n, float* logprobs_out, size_t logprobs_len, size_t* top_ids_out,
                                   float* top_logprobs_out, size_t top_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && logprobs_out, ZG_ERR_ARG, "generate_fetch_logprobs: null argument");
    const size_t C = g->cfg.context_size, B = g->batch, K = ZG_LOGPROBS_TOP_MAX;
    ZG_REQUIRE(g->lp.valid, ZG_ERR_ARG, "generate_fetch_logprobs: the last generation recorded no log-probabilities");
    ZG_REQUIRE(top_n <= g->lp.top_n, ZG_ERR_ARG, "generate_fetch_logprobs: top_n %zu above the %zu the generation recorded", top_n, g->lp.top_n);
    ZG_REQUIRE(top_n == 0 || (top_ids_out && top_logprobs_out), ZG_ERR_ARG, "generate_fetch_logprobs: top_n %zu without its outputs", top_n);
    ZG_REQUIRE(first <= C && n <= C - first && logprobs_len >= B * n && (top_n == 0 || top_len >= B * n * top_n), ZG_ERR_SHAPE,
               "generate_fetch_logprobs: positions %zu .. %zu of %zu, %zu and %zu elements", first, first + n, C, logprobs_len, top_len);
    if (n == 0) return ZG_OK;
    hipStream_t s = gs(g);
    float* h_lp = g->lp.h_rec;
    int* h_ids = reinterpret_cast<int*>(g->lp.h_rec + B * C);
    float* h_top = g->lp.h_rec + B * C * (1 + K);
    // the columns asked for, packed [batch][n] and [batch][n][20]
    ZG_HIP(hipMemcpy2DAsync(h_lp, n * 4, g->lp.rec.logprob + first, C * 4, n * 4, B, hipMemcpyDeviceToHost, s));
    if (top_n) {
        ZG_HIP(hipMemcpy2DAsync(h_ids, n * K * 4, g->lp.rec.top_ids + first * K, C * K * 4, n * K * 4, B, hipMemcpyDeviceToHost, s));
        ZG_HIP(hipMemcpy2DAsync(h_top, n * K * 4, g->lp.rec.top_logprobs + first * K, C * K * 4, n * K * 4, B, hipMemcpyDeviceToHost, s));
    }
    ZG_HIP(hipStreamSynchronize(s));
    ZG_TRY(check_fault(g));
    memcpy(logprobs_out, h_lp, B * n * sizeof(float));
    unpack_top(h_ids, h_top, B * n, top_n, top_ids_out, top_logprobs_out);
    return ZG_OK;
}

// ---- Beam search: the request call plus the options.  A beam step is a greedy slot with the log-probability stage
// at top_n = 2 W; the beam launch and the cache fork follow it (enqueue_step).
int zg_gpt_generate_beam_enqueue(zg_gpt* g, const zg_generate_request* r, const zg_beam_options* beam) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g != nullptr, ZG_ERR_ARG, "generate_beam: null handle");
    ZG_TRY(check_beam(r, beam, g->batch, g->cfg.vocab_size, g->cfg.context_size, g->cached_len, "generate_beam"));
    GenRequest q(r->prompts, r->prompt_stride, r->prompt_lens, r->n_steps, r->past_len);
    q.lp_on = true;
    q.top_n = 2 * beam->num_beams;
    q.beam_on = true;
    q.beam = *beam;
    return gen_run(&g, 1, q);
}

namespace {

// A finished hypothesis on the host: a pool entry of the device (eos: the token behind column col - 1 of slot `parent`), or the
// beam a slot holds when the generation ends (its last token in column col - 1 of that slot)
struct BeamHyp {
    float sum, norm;
    int parent, col;
    bool eos;
};

// beam_key of sample_beam.h: NaN below every number, -0.0 equal to +0.0
unsigned host_beam_key(float v) {
    if (v != v) return 0u;
    if (v == 0.0f) return 0x80000000u;
    unsigned u;
    memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the pool's rule (sample_beam.h): room, or strictly better than the worst entry — lowest norm, among equals the highest index
void beam_pool_offer(std::vector<BeamHyp>& pool, size_t W, const BeamHyp& h) {
    if (pool.size() < W) {
        pool.push_back(h);
        return;
    }
    size_t w = 0;
    for (size_t k = 1; k < pool.size(); ++k)
        if (host_beam_key(pool[k].norm) <= host_beam_key(pool[w].norm)) w = k;
    if (host_beam_key(h.norm) > host_beam_key(pool[w].norm)) pool[w] = h;
}

}  // namespace

int zg_gpt_generate_fetch_beams(zg_gpt* g, size_t n_return, size_t* tokens_out, size_t stride, size_t* lens_out, float* scores_out, float* sum_logprobs_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && tokens_out && lens_out && scores_out && sum_logprobs_out, ZG_ERR_ARG, "generate_fetch_beams: null argument");
    ZG_REQUIRE(g->beam.valid, ZG_ERR_ARG, "generate_fetch_beams: the last generation did not come through zg_gpt_generate_beam_enqueue");
    const size_t C = g->cfg.context_size, B = g->batch, W = g->beam.W, G = B / W, c0 = g->beam.c0, end = g->gen.n;
    ZG_REQUIRE(n_return >= 1 && n_return <= W, ZG_ERR_ARG, "generate_fetch_beams: n_return %zu outside 1..%zu", n_return, W);
    ZG_REQUIRE(end > c0 && end <= C, ZG_ERR_ARG, "generate_fetch_beams: the generation ended at column %zu, its first pick was column %zu", end, c0);
    hipStream_t s = gs(g);
    int* const h_tok = g->h_ints;                 // [B][C] the recorded tokens
    int* const h_par = g->h_ints + B * C + B;     // [B][C] the recorded parents (the staging of the penalties' history: idle here)
    ZG_HIP(hipMemcpyAsync(h_tok, g->out_tokens, B * C * sizeof(int), hipMemcpyDeviceToHost, s));
    ZG_HIP(hipMemcpyAsync(h_par, g->beam.parent, B * C * sizeof(int), hipMemcpyDeviceToHost, s));
    ZG_HIP(hipMemcpyAsync(g->beam.h_state, g->beam.state, sizeof(BeamState), hipMemcpyDeviceToHost, s));
    ZG_HIP(hipStreamSynchronize(s));
    ZG_TRY(check_fault(g));
    const BeamState& st = *g->beam.h_state;
    const float lp_end = (float)pow((double)(end - c0), (double)g->beam.length_penalty);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<size_t> seq;
    // every length is known before anything is written: a stride too short for one of them refuses the whole call
    std::vector<std::vector<BeamHyp>> pools(G);
    for (size_t gr = 0; gr < G; ++gr) {
        std::vector<BeamHyp>& pool = pools[gr];
        const size_t n = (size_t)std::min(std::max(st.pool_n[gr], 0), (int)W);
        for (size_t k = 0; k < n; ++k) pool.push_back({st.pool_sum[gr * W + k], st.pool_norm[gr * W + k], st.pool_parent[gr * W + k], st.pool_col[gr * W + k], true});
        if (st.done_col[gr] < 0)
            for (size_t t = 0; t < W; ++t) beam_pool_offer(pool, W, {st.score[gr * W + t], st.score[gr * W + t] / lp_end, (int)(gr * W + t), (int)end, false});
        std::stable_sort(pool.begin(), pool.end(), [](const BeamHyp& x, const BeamHyp& y) { return host_beam_key(x.norm) > host_beam_key(y.norm); });
        for (size_t i = 0; i < n_return && i < pool.size(); ++i) {
            const size_t len = (size_t)pool[i].col - c0 + (pool[i].eos ? 1 : 0);
            ZG_REQUIRE((size_t)pool[i].col >= c0 && (size_t)pool[i].col <= end && len <= stride, ZG_ERR_SHAPE,
                       "generate_fetch_beams: a hypothesis of %zu tokens (column %d) for a stride of %zu", len, pool[i].col, stride);
        }
    }
    for (size_t gr = 0; gr < G; ++gr)
        for (size_t i = 0; i < n_return; ++i) {
            const size_t o = gr * n_return + i;
            if (i >= pools[gr].size()) {
                lens_out[o] = 0;
                scores_out[o] = sum_logprobs_out[o] = nan;
                continue;
            }
            const BeamHyp& h = pools[gr][i];
            seq.clear();
            if (h.eos) seq.push_back((size_t)st.eos);
            size_t cur = (size_t)h.parent;
            for (size_t c = (size_t)h.col; c-- > c0;) {  // columns col - 1 .. c0, following the parents (held inside the group)
                cur = std::min(std::max(cur, gr * W), gr * W + W - 1);
                seq.push_back((size_t)h_tok[cur * C + c]);
                cur = (size_t)std::max(h_par[cur * C + c], 0);
            }
            std::reverse(seq.begin(), seq.end());
            for (size_t k = 0; k < seq.size(); ++k) tokens_out[o * stride + k] = seq[k];
            lens_out[o] = seq.size();
            scores_out[o] = h.norm;
            sum_logprobs_out[o] = h.sum;
        }
    return ZG_OK;
}

int zg_gpt_generate_fetch_beam_trace(zg_gpt* g, size_t first, size_t n, int* parents_out, float* scores_out, size_t len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && parents_out && scores_out, ZG_ERR_ARG, "generate_fetch_beam_trace: null argument");
    ZG_REQUIRE(g->beam.valid, ZG_ERR_ARG, "generate_fetch_beam_trace: the last generation did not come through zg_gpt_generate_beam_enqueue");
    const size_t C = g->cfg.context_size, B = g->batch;
    ZG_REQUIRE(first <= C && n <= C - first && len >= B * n, ZG_ERR_SHAPE, "generate_fetch_beam_trace: positions %zu .. %zu of %zu, %zu elements", first,
               first + n, C, len);
    if (n == 0) return ZG_OK;
    hipStream_t s = gs(g);
    int* const h_par = g->h_ints;
    float* const h_sc = g->lp.h_rec;
    ZG_HIP(hipMemcpy2DAsync(h_par, n * 4, g->beam.parent + first, C * 4, n * 4, B, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipMemcpy2DAsync(h_sc, n * 4, g->beam.score + first, C * 4, n * 4, B, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipStreamSynchronize(s));
    ZG_TRY(check_fault(g));
    memcpy(parents_out, h_par, B * n * sizeof(int));
    memcpy(scores_out, h_sc, B * n * sizeof(float));
    return ZG_OK;
}

// The recorded tokens of positions first .. first + n - 1, packed [batch][n]: the body of both fetches (their arguments checked)
static int fetch_tokens(zg_gpt* g, size_t first, size_t n, size_t* out_tokens) {
    const size_t C = g->cfg.context_size, B = g->batch;
    hipStream_t s = gs(g);
    ZG_HIP(hipMemcpyAsync(g->h_ints, g->out_tokens, B * C * sizeof(int), hipMemcpyDeviceToHost, s));
    ZG_HIP(hipStreamSynchronize(s));
    ZG_TRY(check_fault(g));
    for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < n; ++i) out_tokens[b * n + i] = (size_t)g->h_ints[b * C + first + i];
    return ZG_OK;
}

int zg_gpt_generate_fetch_range(zg_gpt* g, size_t first, size_t n, size_t* out_tokens, size_t out_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && out_tokens, ZG_ERR_ARG, "generate_fetch_range: null argument");
    const size_t C = g->cfg.context_size, B = g->batch;
    ZG_REQUIRE(first <= C && n <= C - first && out_len >= B * n, ZG_ERR_SHAPE, "generate_fetch_range: positions %zu .. %zu of %zu, %zu elements", first,
               first + n, C, out_len);
    return fetch_tokens(g, first, n, out_tokens);
}

// generate (src/main.zig:322-342) for the prompts of SEVERAL handles at once: independent sequences need not run in lock step
// (the reference's batch restriction, ops.zig:126-128, lifted the other way): gen_run with one stream per handle
// (zg_gpt_create_ex: own_stream).
int zg_gpt_generate_enqueue_many(zg_gpt* const* handles, size_t n_handles, const size_t* prompts, size_t prompt_stride,
                                 const size_t* prompt_lens, size_t n_steps) {
    ZG_TRY(require_init());
    ZG_REQUIRE(handles && n_handles >= 1 && n_handles <= 64 && prompts && prompt_lens, ZG_ERR_ARG, "generate_many: bad argument");
    for (size_t i = 0; i < n_handles; ++i) {
        ZG_REQUIRE(handles[i] != nullptr, ZG_ERR_ARG, "generate_many: handle %zu is null", i);
        for (size_t j = 0; j < i; ++j) {
            ZG_REQUIRE(handles[i] != handles[j], ZG_ERR_ARG, "generate_many: handle %zu is handle %zu", i, j);
            ZG_REQUIRE(n_handles == 1 || gs(handles[i]) != gs(handles[j]), ZG_ERR_ARG,
                       "generate_many: handles %zu and %zu share a stream (create them with own_stream)", j, i);
        }
    }
    return generate_request(handles, n_handles, request_of(0, prompts, prompt_stride, prompt_lens, n_steps), "generate_many");
}

int zg_gpt_generate_fetch_many(zg_gpt* const* handles, size_t n_handles, size_t n_steps, size_t* out_tokens, size_t out_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(handles && n_handles >= 1 && out_tokens, ZG_ERR_ARG, "generate_fetch_many: null argument");
    size_t rows = 0;
    for (size_t i = 0; i < n_handles; ++i) {
        ZG_REQUIRE(handles[i] != nullptr, ZG_ERR_ARG, "generate_fetch_many: handle %zu is null", i);
        rows += handles[i]->batch;
    }
    ZG_REQUIRE(out_len >= rows * n_steps, ZG_ERR_SHAPE, "generate_fetch_many: out_tokens too short");
    size_t row = 0;
    int first_err = ZG_OK;
    char msg[512];
    for (size_t i = 0; i < n_handles; ++i) {  // every handle is drained, also behind a failed one
        const int e = zg_gpt_generate_fetch(handles[i], n_steps, out_tokens + row * n_steps, handles[i]->batch * n_steps);
        if (first_err == ZG_OK && e != ZG_OK) {
            first_err = e;
            snprintf(msg, sizeof msg, "%s", zg_last_error());
        }
        row += handles[i]->batch;
    }
    if (first_err != ZG_OK) set_error("%s", msg);
    return first_err;
}

int zg_gpt_generate_fetch(zg_gpt* g, size_t n_steps, size_t* out_tokens, size_t out_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && out_tokens, ZG_ERR_ARG, "generate_fetch: null argument");
    ZG_REQUIRE(n_steps <= g->cfg.context_size && out_len >= g->batch * n_steps, ZG_ERR_SHAPE, "generate_fetch: out_tokens too short");
    return fetch_tokens(g, 0, n_steps, out_tokens);
}

int zg_gpt_generate_greedy(zg_gpt* g, const size_t* prompts, size_t prompt_stride, const size_t* prompt_lens,
                           size_t n_steps, size_t* out_tokens, size_t out_len) {
    ZG_REQUIRE(g && out_tokens && out_len >= g->batch * n_steps, ZG_ERR_SHAPE, "generate: out_tokens too short");
    ZG_TRY(zg_gpt_generate_enqueue(g, prompts, prompt_stride, prompt_lens, n_steps));
    return zg_gpt_generate_fetch(g, n_steps, out_tokens, out_len);
}

}  // extern "C"
