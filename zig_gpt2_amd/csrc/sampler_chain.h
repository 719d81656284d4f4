// sampler_chain.h — the handle-free host side of the sampler (sampler_chain.hip).  What follows lm_head — which sampler, penalties or
// not, log-probabilities or not — travels as ONE value, StepTail, from the request to the launches; the sampler chain behind
// lm_head is emitted by emit_sampler_chain for every user: the decode step of a handle (api_gpt_step.hip), the per-token calls
// (api_gpt_generate.hip) and the row harnesses on a caller's rows (api_gpt_debug.hip).  Nothing here knows a handle.
#pragma once

#include "zg_runtime.h"

using namespace zg;

// What a step puts behind lm_head: nothing (greedy: the argmax partials of its epilogue are the pick), GPT.sample's tail, or that
// tail behind the selection launches of one filter (top-k or top-p) / of both.  The one form "how are tokens chosen" travels in.
// MINP_ONLY: min-p with both filters off — the threshold-aware tail kernels with no selection launch in front.
enum SamplerMode { GREEDY = 0, PLAIN, ONE_FILTER, TWO_FILTERS, MINP_ONLY };
constexpr size_t kSamplerModes = MINP_ONLY + 1;
static inline int filter_launches(SamplerMode m) { return m == TWO_FILTERS ? 6 : m == ONE_FILTER ? 3 : 0; }  // sample_filter.h: three levels per descent
static inline bool threshold_sampler(SamplerMode m) { return m == ONE_FILTER || m == TWO_FILTERS || m == MINP_ONLY; }  // the tail kernels that read tau

// Everything that follows lm_head in a decode step, as one value: the sampler, the penalty stage between lm_head and the sampler
// (DESIGN §3.6), the edit stage — logit bias, allow / ban lists — behind the penalties, the log-probability stage
// behind the sampler — of a greedy step: behind lm_head —, the stop stage behind everything.  The
// default is the greedy step the reference's argmax loop runs.
struct StepTail {
    SamplerMode sampler = GREEDY;
    bool pen = false, lp = false, stop = false, edit = false;
    bool guide = false;  // guided decoding: the mask behind (and in one launch with) the edits, the advance behind the sampler
    bool ban = false;    // history-dependent bans: the ban launch between the penalties and the edits
    bool beam = false;   // beam search: the beam launch and the cache fork behind the log-probability stage
    bool operator==(const StepTail& o) const {
        return sampler == o.sampler && pen == o.pen && lp == o.lp && stop == o.stop && edit == o.edit && guide == o.guide && ban == o.ban && beam == o.beam;
    }
};
// The tail a step can have: nothing is drawn from a step without lm_head (the default tail), a greedy pick has neither
// penalties, edits, a guide nor bans, and a beam step is a greedy slot plus the log-probability stage (the beam stage has its own
// early end: no stop stage)
static inline StepTail normalized(StepTail t, bool with_logits) {
    if (!with_logits) return StepTail{};
    if (t.beam) {
        t.sampler = GREEDY;
        t.lp = true;
        t.stop = false;
    }
    if (t.sampler == GREEDY) t.pen = t.edit = t.guide = t.ban = false;
    return t;
}

namespace zg {

// What the sampler chain — penalties, edits, selection launches, sampler — reads and writes.  The draw comes from one of two
// sources: the loop's control block (ctrl: the uniform is the counter PRNG of the position it holds), or a per-call buffer of
// uniforms (u, with the call's temperature and whether the probabilities are written back over the row).
struct SamplerChain {
    float* logits;
    int batch, vocab;
    float* part_val;  // row-maximum partials [batch][n_part] as lm_head's epilogue leaves them, and their indices
    int* part_idx;
    int n_part;
    const PenParams* pen;  // [batch]: one entry per row, as params below (a uniform call stages equal entries)
    PenHistory hist;
    unsigned* counts;  // (zg_debug_penalize_rows: the counts of every row's history)
    const EditTable* edit_tab;
    const unsigned* edit_keep;
    GuideArgs guide;  // the automaton, the rows' states and (the loop) the column in flight
    BanArgs ban;      // the rules of the call and where each row stands (the history is `hist`, the penalties')
    const SampleParams* params;
    float* seg_ws;
    FilterWs filt;
    const StepCtrl* ctrl;  // the loop's draws ...
    const float* u;        // ... or a call's
    float temp;            // a per-call plain sampler with per_row false takes it by value and reads no params
    bool per_row;          // ... with per_row true it reads params[b] like every other sampler
    bool write_probs;
    int* pick;
};

// ---- sampler_chain.hip
size_t edit_block_bytes(size_t vocab);
int emit_sampler_chain(const SamplerChain& c, StepTail t, hipStream_t s);
int check_top_n(size_t top_n, size_t vocab, const char* who);
void unpack_top(const int* ids, const float* vals, size_t rows, size_t top_n, size_t* ids_out, float* vals_out);
bool penalties_off(const zg_logit_penalties& p);
bool edits_off(const zg_logit_edits& e);
int build_edits(const zg_logit_edits* e, size_t vocab, const char* who, char* block, bool* stage_on);
size_t guide_keep_words(size_t vocab);
int build_guide(const zg_guide* gd, size_t vocab, const char* who, unsigned* keep);
int check_guide_call(const unsigned* guide_keep, size_t n_states, size_t vocab, const unsigned* call_keep, const size_t* start_states, size_t n, bool greedy,
                     const char* who, int* states_out, bool* any_out);
int check_bans(const zg_ban_rules* r, size_t batch, size_t vocab, size_t context, size_t kept, size_t n_steps, const size_t* prior_lens, bool greedy,
               bool guided, const char* who, bool* on_out);
void fill_bans(BanRules* d, const zg_ban_rules& r, size_t batch, size_t past_len);
size_t edits_kept(const char* block_or_null, size_t vocab);
SamplerMode fill_sample_params(SampleParams* p, size_t vocab, const zg_sample_options& o, uint64_t seed, float min_p);
int plan_rows(const zg_row_sampling* rows, size_t n_rows, size_t vocab, size_t past_len, const char* who, SampleParams* sp, PenParams* pp, int* forms,
              StepTail* tail);
void uniform_rows(zg_row_sampling* rows, size_t n_rows, const zg_sample_options& o, float min_p, const zg_logit_penalties* pen_or_null, uint64_t seed);
int check_penalties(const zg_logit_penalties* p, const char* who);
int check_sample_options(const zg_sample_options* o, const char* who);
int check_stop(const zg_stop_conditions* c, size_t vocab, const char* who);
void fill_stop(StopConds* d, const zg_stop_conditions& c);
int check_beam(const zg_generate_request* q, const zg_beam_options* o, size_t batch, size_t vocab, size_t context, size_t cached_len, const char* who);
void fill_beam_state(BeamState* d, const zg_beam_options& o, size_t c0);
void fill_lenpow(float* d, size_t n, float length_penalty);

}  // namespace zg
