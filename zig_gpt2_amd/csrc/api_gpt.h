// api_gpt.h — the model tier's internal header: the types that cross its units and, one block per unit, the functions a unit offers
// the others.  Not included by any kernel unit.
//   api_gpt.hip           the handle: arena, create / destroy, tensor loads, forward
//   api_gpt_step.hip      what a decode step launches and which graph replays it
//   api_gpt_pass.hip      the whole-prompt pass
//   api_gpt_generate.hip  drawing tokens from a handle
//   sampler_chain.hip     the handle-free host side of the sampler (sampler_chain.h)
//   api_gpt_debug.hip     everything that exists for tests and measurements
#pragma once

#include <stddef.h>
#include <stdlib.h>

#include <utility>
#include <vector>

#include "sampler_chain.h"

constexpr size_t kRowsMax = 8;  // rows of a handle (zg_gpt_create: batch <= 8): entries of the per-row parameter arrays
constexpr size_t kSkFlagWords = 512;  // flag words of the stream-K hand-over (zg_gpt.pass.sk_flags): four per shared tile, 128 shared tiles

struct zg_layer {
    void *c_attn_w, *c_proj_w, *c_fc_w, *mlp_proj_w;
    // ZG_GPT_WEIGHTS_F32 / _B24 handles only: the same matrices (the stored values) split exactly into bf16 planes [out][3 in] = [hi | mid | lo]
    // (filled when the tensor is loaded) — the B operand of the whole-prompt GEMMs
    bf16_t *c_attn_p, *c_proj_p, *c_fc_p, *mlp_proj_p;
    // LayerNorm folded out of the two LayerNorm-fed Linears (gemv_ksplit.hip, gemv_lnk_kernel): c2 = W g, c3 = W b + bias
    float *c_attn_c2, *c_attn_c3, *c_fc_c2, *c_fc_c3;
    float *ln_1_g, *ln_1_b, *c_attn_b, *c_proj_b, *ln_2_g, *ln_2_b, *c_fc_b, *mlp_proj_b;
    void *k_cache, *v_cache;
};

// The decode modes the step unit's builders lay the arguments out for: the handle's own (zg_gpt.modes) for a step, a candidate
// while decide_step_modes decides them
struct StepModes {
    bool pl, st, tags;  // activation planes between the kernels / LayerNorm statistics by tile / tagged hand-overs (lock-step batch)
    bool fused;         // one sequence: ln_1 + c_attn and the attention of a layer as ONE launch (attn_qkv.hip)
};

// The ONE pinned block behind zg_gpt.h_ctrl: the control mirror and the small words that travel beside it.  The kernels store to
// `fault`, the host stages the rest; the groups of zg_gpt hold pointers to their members.
struct PinnedCtrl {
    StepCtrl ctrl;
    alignas(128) SampleParams samp[kRowsMax];  // samp.h_params: one entry per row (batch <= 8)
    alignas(128) unsigned fault;     // hand.fault: written by the kernels
    alignas(64) float uniforms[8];   // the per-token family's draws (batch <= 8): h_ints[0 .. batch) is still being read by the forward's token upload
    alignas(128) PenParams pen[kRowsMax];      // pen.h_params: one entry per row
    alignas(32) int top_n;           // lp.h_top
    alignas(32) int guide_state[kRowsMax];  // guide.h_state: the start state of every row (-1: no guide)
    alignas(64) BeamState beam;      // beam.h_state: the options and the start state of a beam generation
};
static_assert(sizeof(SampleParams) == 24 && sizeof(PenParams) == 16 && offsetof(PinnedCtrl, samp) == 128 && offsetof(PinnedCtrl, fault) == 384 &&
                  offsetof(PinnedCtrl, uniforms) == 448 && offsetof(PinnedCtrl, pen) == 512 && offsetof(PinnedCtrl, top_n) == 640,
              "the pinned control block keeps its layout");

struct zg_gpt {
    zg_gpt_config cfg;
    size_t batch;
    unsigned flags;
    int wt;        // WT_BF16 / WT_F32 / WT_B24
    int kv_mode;
    size_t wbytes;  // bytes per matrix element (B24: 3, a row is [K upper halves | K low bytes])
    char* arena;
    size_t arena_bytes, weight_region_bytes, state_bytes;  // arena = [weight region (absent when borrowed) | state]
    size_t kv_region_bytes;  // the KV caches of all layers: one contiguous stretch of the arena from layers[0].k_cache
    void *wte, *wpe;
    float *ln_f_g, *ln_f_b;
    float *lm_c2, *lm_c3;  // ln_f folded out of lm_head (batched decode): wte g, wte b
    std::vector<zg_layer> layers;
    // state
    StepCtrl* ctrl;
    float *x, *q, *h4, *part, *logits, *part_val;
    int *part_idx, *prompt, *prompt_len, *forced, *cur_token, *out_tokens;
    // split-K combine area of the batched wide Linears (mlp c_proj): [sk_tiles][4][128] floats + one counter per tile
    float* sk_ws;
    int* sk_cnt;
    int sk_tiles;
    // lock-step batch with bf16 weights: activation planes between the kernels of a Block (GemvArgs.pl_in / pl_out):
    // xp = planes of g * x for the next LayerNorm-fed Linear [48 E bytes], hp = planes of gelu(c_fc) [48 * 4E bytes]
    // ap = planes of the merged attention output [48 E bytes], written by the last split of every (sequence, head)
    // (AttnArgs.pl_out; attn_cnt = its arrival counters)
    bf16_t *xp, *hp, *ap;
    int* attn_cnt;
    unsigned tail_off;    // AttnArgs.tail_off: ZGPT2_DECODE_PATHS_OFF's kStepPathsAtCreate bits, read once at create
    // LayerNorm statistics of x by 16-column tile, written by the producers of x (GemvArgs.st_out / st_in)
    float* xst;
    int max_splits, lm_grid;
    // pinned host mirrors for small control traffic
    PinnedCtrl* h_ctrl;
    int* h_ints;  // [batch * ctx] staging for prompts / tokens
    size_t w_gen;             // (the owner of a weight region) bumped whenever its wte may have changed
    size_t steps_enqueued;
    bool ln_folded;  // c2 / c3 of every layer match the weights currently in the arena
    // independent prompt groups on one GPU (zg_gpt_create_ex): a private stream, so that the decode chains of several handles
    // overlap on the chip, and a weight region borrowed from another handle of the same model
    hipStream_t stream;  // nullptr: the library stream of the moment (zg_set_stream)
    zg_gpt* parent;      // owner of the weight region this handle reads (nullptr: its own)
    bool counted;        // this handle is one of its parent's n_children
    int n_children;      // handles borrowing this one's weight region
    char* wbase;         // the weight region: arena, or the parent's
    // the session: positions the caches hold, and the row behind the last one written since the rows behind a pass
    // were last cleared — a continuation clears [its end, context) only when something may be there
    size_t cached_len, kv_dirty_hi;
    // zg_gpt_hidden — where the residual stream of the last forward lives: x (a decode step; a pass with logits copies its last rows
    // there), or the last of the P rows per sequence of pass.x.  A pass without logits stops its last Block behind the cache append
    // (enqueue_prefill): HID_PASS_OPEN, and zg_gpt_hidden runs the rest of that Block once, from pass.qkv and the caches, before it
    // reads the rows (HID_PASS_DONE).  No step or pass pays for it.
    struct {
        int src;  // HID_X / HID_PASS_OPEN / HID_PASS_DONE
        size_t pos0, P;
    } hidden;

    // What follows belongs to one unit each, which the comment names.  Every group is an aggregate that value-initialises to zeros
    // (new zg_gpt() zeroes the whole handle: release() relies on it); carve() and build_handle fill the pointers of all of them.

    // step (decided once at create: decide_step_modes): the decode modes of this handle's steps
    StepModes modes;
    // handle (note_steps, check_fault) — tagged hand-overs (GemvArgs.sk_tag, AttnArgs.part_tag): step counter advanced by the embed
    // kernel, (value, tag) words; the step unit hands the pointers to the launches
    struct {
        unsigned* epoch;
        unsigned spin_limit;  // polls before a poller of a tagged hand-over gives up
        unsigned* fault;  // set by a poller of a tagged hand-over whose bounded wait ran out; checked wherever a call drains the stream
        unsigned long long *sk_tag, *part_tag;
        size_t sk_tag_bytes, part_tag_bytes;
        size_t epochs_since_clear;  // steps enqueued since the tagged words were last zeroed (note_steps)
        size_t steps_counted, tag_clears;  // steps note_steps has counted in all, clears it has enqueued (zg_debug_gpt_age_state)
        // the fused launch of one sequence (modes.fused): q and the new k / v row handed over as (value, tag) words [3 E] (tags as
        // above: the embed kernel advances the epoch)
        unsigned long long* qkv_tag;
        size_t qkv_tag_bytes;
    } hand;
    // step — graphs [step_index(StepKey)][n_buckets]: one per (step shape, 64-position bucket of seq_len), captured on first use
    // (graph_exec).  The bucket's upper bound t_hi is baked into the attention / merge kernels so that their loads do not wait
    // for the exact seq_len (which lives in device memory).
    struct {
        std::vector<hipGraphExec_t> execs;
        size_t n_buckets;  // ceil(context / 64)
        size_t steps;      // decode steps per multi-step graph (ZGPT2_GRAPH_STEPS)
        hipStream_t stream;
    } graph;
    // step — side-stream L2 prefetcher of the decode chain (prefetch.hip); runs during zg_gpt_generate_enqueue only
    struct {
        PfCtl* ctl;
        PfJob* jobs;  // [njobs]: embed, 5 per layer, lm_head
        int njobs;
        bool on;
        bool ran;      // a prefetcher was launched by the last generate call
        bool stalled;  // one left on its idle limit (no concurrency with the decode stream, or a host hiccup): sitting out
        int strikes;   // idle-limit exits so far; the third one is final
        int sit_out;   // generate calls left before a stalled prefetcher is tried again
        hipStream_t stream;
        hipEvent_t ev_main, ev_side;
    } prefetch;
    // pass — whole-prompt (prefill) scratch, rows = batch * ctx: x fp32 [E], qkv fp32 [3E], split bf16 a [kSplit E] and h [kSplit 4E]
    // (the pf_x, pf_qkv, pf_a and pf_h of the pass taps, include/zgpt2.h), the split-K partials ws; all null under ZG_GPT_NO_PREFILL
    struct {
        float *x, *qkv, *ws;
        size_t ws_floats;
        unsigned* sk_flags;   // stream-K hand-over of the c_attn GEMM (PrefillQkv.sk_*): kSkFlagWords flag words, zeroed at create
        unsigned sk_epoch;    // the epoch last handed to a stream-K launch: never 0, the value of a flag word no launch has written (next_sk_epoch)
        size_t sk_restarts;   // times the epoch wrapped: the flag words were zeroed on the stream and the count began again at 1
        bool sk_used;         // a stream-K launch since the last check of gemm_s4_fault
        bf16_t *a, *h;
    } pass;
    // pass — scoring (zg_gpt_score; sample_score.h), carved under ZG_GPT_SCORE only: the logits of one block of kScoreRows
    // rows [kScoreRows][v64] (v64 = the vocabulary on the GEMMs' 64-column grid), the chunk workspace of that block, and the lm_head
    // operand the whole-prompt GEMM cannot take from the weight region: bf16 weights — the last vocab % 64 rows of wte as a [64][E]
    // strip, zero rows behind them; fp32 / B24 weights — wte's planes [3][v64][E], zero rows behind the vocabulary, and the
    // slab workspace of that launch.  gen: w_gen + 1 of the weights the strip / planes were made from (0: never made)
    struct {
        float* logits;
        ScoreWs ws;
        bf16_t *tail, *planes;
        float* gemm_ws;
        size_t gemm_ws_floats, v64, gen;
    } score;
    // generate / the step tail — the sampler of the generation in flight or of a per-token call
    struct {
        int* sampled;            // [batch]: the sampler's draw from the last step's logits
        float* ws;               // segment sums of the sampler (sample_workspace_floats)
        SampleParams* params;    // device [kRowsMax]: each row's temperature, filters and seed of the generation in flight
        SampleParams* h_params;  // pinned mirror (PinnedCtrl.samp)
        FilterWs filt;           // selection workspace of the truncated sampler (sample_filter.h), zero at create
    } samp;
    // generate — logit penalties (sample_penalty.h): the caller's prior / explicit history [batch][ctx] with its lengths,
    // the values of the call in flight, one entry per row ([kRowsMax]), their pinned mirrors (h_params: PinnedCtrl.pen; h_prior: [batch * ctx] tokens, then [batch]
    // lengths, behind h_ints).  The kernels' table is LDS: no workspace
    struct {
        int *prior, *prior_len;
        PenParams *params, *h_params;
        int* h_prior;
    } pen;
    // generate — log-probabilities (sample_logprob.h): the chunk workspace, top_n of the generation in flight (device
    // word `top` and its place in the pinned control block, `h_top`), the record buffers [batch][ctx] / [batch][ctx][20] and the
    // pinned mirror a fetch copies its columns through (h_rec: [batch * ctx] log-probabilities, then [batch * ctx * 20] ids, then
    // as many values)
    struct {
        LogprobWs ws;
        LogprobRec rec;
        int *top, *h_top;
        float* h_rec;
        bool valid;    // the last generation (or zg_gpt_score) recorded them: the record can be fetched
        size_t top_n;  // ... with this many alternatives
    } lp;
    // generate — stop conditions (sample_stop.h): the conditions of the generation in flight, finish column and reason of
    // every row (-1: none), and ONE pinned block: the staging mirror of the conditions, the way back of the two arrays, and the two
    // words the stop kernel stores to (host.progress, host.done_col)
    struct {
        StopConds* conds;
        int *fin, *reason;
        struct StopPinned {
            StopConds conds;
            int fin[kStopMaxRows], reason[kStopMaxRows];
            alignas(64) StopHost host;
        }* pinned;
    } stop;
    // generate — logit edits (sample_edit.h): the bias table and, behind it, the keep bitmap of vocab bits — one block
    // in the arena, its pinned mirror, and plain host memory of the same size in which a call's set is built and checked before
    // anything else is touched (build)
    struct {
        EditTable* tab;
        unsigned* keep;
        char* h_block;
        std::vector<char> build;
    } edit;
    // generate — guided decoding (sample_guide.h), carved under ZG_GPT_GUIDED_GENERATE only (all null without): the
    // transition table [256][vocab] uint16, the keep bitmap of every state [256][words], the device word n_states (0: no table), each
    // row's state ([kRowsMax]; its pinned mirror h_state: PinnedCtrl.guide_state) and the state record [batch][ctx] (-1: none); on the
    // host the bitmaps of the loaded table, kept for the checks of later calls
    struct {
        unsigned short* next;
        unsigned* keep;
        int *n_states, *state, *rec, *h_state;
        std::vector<unsigned> h_keep;
        size_t loaded;  // states of the table the handle holds (0: none)
        bool valid;     // the last generation came through zg_gpt_generate_guided_enqueue: the record can be fetched
    } guide;
    // generate — history-dependent bans (sample_ban.h): the rules of the call in flight — one small block carved
    // behind everything else in the arena —, its pinned mirror, and plain host memory in which a call's rules are laid out once they
    // are checked (build).  The history is the penalties' (pen.prior staged whenever penalties OR bans are on, and the loop's record)
    struct {
        BanRules *rules, *h_rules;
        BanRules build;
    } ban;
    // generate — beam search (sample_beam.h): the options and the groups' state, the trace of parents and cumulative
    // scores [batch][ctx] and the table lenpow [ctx + 1] — one block carved behind everything else in the arena —, the pinned mirror of
    // the state (PinnedCtrl.beam), and what the last beam generation was: fetch_beams finalises on the host from these
    struct {
        BeamState *state, *h_state;
        int* parent;
        float *score, *lenpow;
        bool valid;             // the last generation came through zg_gpt_generate_beam_enqueue
        size_t W, c0;
        bool has_eos;
        float length_penalty;
    } beam;
    // generate — a generation in flight between gen_begin and gen_end (zg_gpt_generate_enqueue / _many), and what the last one left
    struct {
        size_t pos, n, min_prompt, since_sync;
        bool open;
        StepTail tail;      // what follows lm_head in the steps of the generation in flight (normalized)
        bool stop;          // the generation in flight has conditions: gen_pump paces itself and may end early
        size_t lookahead;   // ... at most this many steps ahead of host.progress before each piece
        bool stop_valid;    // the last generation was one with conditions: zg_gpt_generate_stop_result can report it
        size_t stop_end;    // ... and ended here
    } gen;
};

// rows of pass.x per lm_head block of zg_gpt_score: one constant, decided by one measurement (profiles/NOTEBOOK.md §16: 256 rows take
// the 128 x 256 tiles and half the launches; -DZG_SCORE_ROWS=128 builds the other candidate)
#ifndef ZG_SCORE_ROWS
#define ZG_SCORE_ROWS 256
#endif
constexpr size_t kScoreRows = ZG_SCORE_ROWS;
constexpr size_t kPassTapRowsBehind = ZG_PASS_TAP_ROWS_BEHIND;  // cache rows a tapped pass copies behind its last position

static inline hipStream_t gs(const zg_gpt* g) { return g->stream ? g->stream : ctx().stream; }
static inline zg_gpt* root(zg_gpt* g) { return g->parent ? g->parent : g; }

namespace zg {

inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) {
        off = (off + 255) & ~(size_t)255;
        const size_t o = off;
        off += bytes;
        return o;
    }
};

// Optional per-kernel event recorder (zg_gpt_profile_step only).
struct StepProf {
    std::vector<hipEvent_t> ev;
    std::vector<int> cls;  // kernel class of the interval ENDING at ev[i]
    size_t n = 0;
};

// What enqueue_step does besides a plain step.
struct StepOpts {
    StepProf* prof = nullptr;  // zg_gpt_profile_step: an event behind every kernel class
    int only = -1;             // >= 0 (measurement): launch just that kernel class of layer only_layer
    size_t only_layer = 0;
    std::vector<PfJob>* rec = nullptr;  // nothing is launched; the step's launches are described for the prefetcher instead (emit_gemv)
    // >= 0 (measurement chains of one kernel class): launch ids of the tagged hand-overs by chain position instead of by
    // layer, so that consecutive launches of the chain never find each other's tags
    int salt = -1;
    StepTail tail;             // what follows lm_head (normalized: the default one without lm_head)
    struct StepTaps* taps = nullptr;  // zg_debug_gpt_step_taps: behind every launch class, copies of what it wrote (eager steps only)
};

// The tap sink of a step (tests): an arena in device memory that device-to-device copies on the step's own stream fill behind
// each launch class, and the table that says what lies where.  With no arena (base == nullptr) nothing is copied and the table
// and `used` alone are built: the sizing pass.  The launches of a tapped step are those of a plain one.
struct StepTaps {
    char* base = nullptr;
    size_t cap = 0, used = 0;
    size_t seq_len = 0;
    std::vector<zg_tap_entry> table;
    std::vector<std::pair<size_t, std::vector<int>>> words;  // tap_words: (arena offset, ints) the host writes behind the read-back
};

// The decode graphs of a handle, per 64-position bucket of the sequence length, keyed by what the graph contains:
//   with_logits  lm_head behind the Blocks (a step that only feeds a prompt token has none)
//   multi        graph.steps consecutive steps (all with lm_head, all in one bucket) as ONE graph: the position lives in device
//                memory, so the same kernels simply repeat; saves the gap between graph launches in the generate loop
//   tail         what follows lm_head (StepTail, normalized; the option values are read on the device)
// The table has a slot for every combination of the fields, indexed by them as mixed-radix digits; the slots of combinations
// that cannot occur (multi or a tail without lm_head, penalties or edits in front of a greedy pick) simply stay null.
struct StepKey {
    bool with_logits, multi;
    StepTail tail;
};
constexpr size_t kStepShapes = 2 * 2 * kSamplerModes * 2 * 2 * 2 * 2 * 2 * 2 * 2;  // the radices of step_index

// What body() enqueues on stream cs, captured and instantiated into *out.  Nothing is left behind on failure.
template <class Body>
int capture_graph(hipStream_t cs, hipGraphExec_t* out, Body body) {
    hipGraph_t graph = nullptr;
    ZG_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    const int st = body();
    hipError_t e = hipStreamEndCapture(cs, &graph);
    if (st == ZG_OK && e == hipSuccess) e = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    ZG_TRY(st);
    ZG_HIP(e);
    return ZG_OK;
}

// zg_gpt_score's part of a pass_impl call
struct ScoreCall {
    size_t top_n;
    float* logits_out;  // [batch][n][vocab], host or device, or null
    size_t logits_len;
};

// ---- api_gpt.hip: the handle
int ensure_ln_folded(zg_gpt* g, hipStream_t s);
int check_fault(zg_gpt* g);
int note_steps(zg_gpt* g, size_t n, hipStream_t s);
int stage_ctrl(zg_gpt* g, size_t step, size_t seq_len, int mode, hipStream_t s);
int copy_out_f32(float* dst, const float* src, size_t n, hipStream_t s);
int clear_for_pass(zg_gpt* g, hipStream_t s, size_t past, size_t end);
int enqueue_kv_fork(zg_gpt* g, int t_hi, const int* src, const int* len, unsigned src_imm, int len_imm, hipStream_t s);
int forward_enqueue(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, int compute_logits, float* logits_out, size_t logits_len,
                    StepTaps* taps = nullptr);

// ---- api_gpt_step.hip: the launches of a decode step, the graph table, the prefetcher
int bucket_t_hi(const zg_gpt* g, size_t seq_len);
EmbedArgs embed_args(const zg_gpt* g, int finish_only);
int prof_mark(StepProf* p, int cls, hipStream_t s);
int decide_step_modes(zg_gpt* g);
int enqueue_lm_head(zg_gpt* g, hipStream_t s, std::vector<PfJob>* rec = nullptr);
SamplerChain handle_chain(const zg_gpt* g, bool loop);
int enqueue_step(zg_gpt* g, bool with_logits, int t_hi, hipStream_t s, const StepOpts& o = StepOpts());
int setup_prefetcher(zg_gpt* g);
void drop_prefetcher(zg_gpt* g);
int pf_start(zg_gpt* g, size_t last_T, hipStream_t s);
int pf_stop(zg_gpt* g, hipStream_t s);
size_t bucket_of(size_t seq_len);
void drop_graphs(zg_gpt* g);
int graph_exec(zg_gpt* g, StepKey k, size_t b, hipStream_t s, hipGraphExec_t* out);
int capture_tail(zg_gpt* g, StepTail tail, size_t b0, size_t b1, hipStream_t s);
int capture_all(zg_gpt* g, hipStream_t s);
int run_step(zg_gpt* g, bool with_logits, size_t seq_len, hipStream_t s, StepTail tail = StepTail{});

// ---- api_gpt_pass.hip: the whole-prompt pass
int ensure_score_weights(zg_gpt* g, hipStream_t s);
enum { HID_X = 0, HID_PASS_OPEN, HID_PASS_DONE };  // zg_gpt.hidden.src
int enqueue_prefill(zg_gpt* g, size_t pos0, size_t P, bool last_block_full, hipStream_t s, StepTaps* taps = nullptr, bool resume_last_block = false);
size_t prefill_min();
int pass_impl(zg_gpt* g, size_t past_len, const size_t* tokens, size_t stride, size_t n, int compute_logits, float* logits_out, size_t logits_len,
              const char* who, const ScoreCall* sc = nullptr, StepTaps* taps = nullptr);

// ---- api_gpt_generate.hip
int stage_top_n(zg_gpt* g, size_t top_n, hipStream_t s);

// ---- api_gpt_debug.hip: the tap sink
int tap_put(StepTaps* t, int cls, size_t layer, int buffer, int type, unsigned flags, const void* src, size_t rows, size_t row_bytes, size_t src_pitch,
            hipStream_t s);
int tap_words(StepTaps* t, int cls, size_t layer, int buffer, const int* w, size_t n);
int tap_caches(const zg_gpt* g, StepTaps* t, int cls, size_t l, unsigned flags, size_t T, hipStream_t s);
int tap_class(const zg_gpt* g, StepTaps* t, int cls, size_t l, unsigned flags, hipStream_t s);

}  // namespace zg
