// api_gpt.hip — model tier of the C ABI: GPTConfig/State/Block/GPT/generate of the reference's
// src/main.zig as one device-resident object.  Weights, per-sequence KV caches and all scratch
// live in a single arena allocated by zg_gpt_create (the State.init / load_gpt moment of the
// reference); a decode step is a fixed chain of kernels captured once into a hipGraph whose
// position, tokens and argmax all live in device memory, so a whole greedy generation is enqueued
// without a host round trip per token.  Three things exist once each: the whole-prompt pass (pass_impl: zg_gpt_prefill is
// zg_gpt_extend at 0), the generation request (every zg_gpt_generate*_enqueue fills a zg_generate_request, generate_request alone
// makes the GenRequest gen_run runs) and the shape of a decode step (StepKey {with_logits, multi, StepTail}: what enqueue_step
// launches and which graph replays it; the sampler chain behind lm_head is emitted by emit_sampler_chain for every user).  What follows
// lm_head — which sampler, penalties or not, log-probabilities or not — travels as ONE value, StepTail, from the request to the
// launches: a generation holds one (zg_gpt::gen_tail), a step is told one (StepOpts::tail), a graph is keyed by one, and the graph
// table is indexed by its fields as mixed-radix digits (step_index).  ONE rule says which graphs exist when: create captures the
// default tail's and those of the tails its flags name (tails_of_flags), and a generation whose tail is another one captures that
// tail's graphs for the buckets it will touch when it begins (gen_begin), before its steps are counted and the prefetcher starts.
//
// HBM layout (one hipMalloc, 256-B aligned sub-buffers):
//   [ weights: wte | wpe | ln_f | per layer: c_attn_w c_proj_w c_fc_w mlp_proj_w + fp32 vectors ]
//   [ KV cache: layer x {K,V} x batch x head x ctx x 64 ]   head-major: one head's keys are one
//                                                            contiguous [ctx, 64] slab, so no
//                                                            per-step transpose (ops.zig:153,158)
//   [ scratch: x q h4 attention partials logits argmax partials, control block, token buffers ]
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <thread>
#include <utility>
#include <vector>

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
    bool operator==(const StepTail& o) const { return sampler == o.sampler && pen == o.pen && lp == o.lp && stop == o.stop && edit == o.edit; }
};
// The tail a step can have: nothing is drawn from a step without lm_head (the default tail), and a greedy pick has neither
// penalties nor edits
static inline StepTail normalized(StepTail t, bool with_logits) {
    if (!with_logits) return StepTail{};
    if (t.sampler == GREEDY) t.pen = t.edit = false;
    return t;
}

constexpr size_t kSkFlagWords = 512;  // flag words of the stream-K hand-over (zg_gpt.sk_flags): four per shared tile, 128 shared tiles

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
    // whole-prompt (prefill) scratch, rows = batch * ctx: x fp32 [E], qkv fp32 [3E], split bf16 [kSplit E] and [kSplit 4E]
    float *pf_x, *pf_qkv, *pf_ws;
    size_t pf_ws_floats;
    unsigned* sk_flags;   // stream-K hand-over of the c_attn GEMM (PrefillQkv.sk_*): kSkFlagWords flag words, zeroed at create
    unsigned sk_epoch;    // the epoch last handed to a stream-K launch: never 0, the value of a flag word no launch has written (next_sk_epoch)
    size_t sk_restarts;   // times the epoch wrapped: the flag words were zeroed on the stream and the count began again at 1
    bool sk_used;         // a stream-K launch since the last check of gemm_s4_fault
    bf16_t *pf_a, *pf_h;
    // lock-step batch with bf16 weights: activation planes between the kernels of a Block (GemvArgs.pl_in / pl_out):
    // xp = planes of g * x for the next LayerNorm-fed Linear [48 E bytes], hp = planes of gelu(c_fc) [48 * 4E bytes]
    // ap = planes of the merged attention output [48 E bytes], written by the last split of every (sequence, head)
    // (AttnArgs.pl_out; attn_cnt = its arrival counters)
    bf16_t *xp, *hp, *ap;
    int* attn_cnt;
    // tagged hand-overs (GemvArgs.sk_tag, AttnArgs.part_tag): step counter advanced by the embed kernel, (value, tag) words
    unsigned* epoch;
    unsigned spin_limit;  // polls before a poller of a tagged hand-over gives up
    unsigned tail_off;    // AttnArgs.tail_off: ZGPT2_DECODE_PATHS_OFF's kStepPathsAtCreate bits, read once at create
    unsigned* fault;  // set by a poller of a tagged hand-over whose bounded wait ran out; checked wherever a call drains the stream
    unsigned long long *sk_tag, *part_tag;
    size_t sk_tag_bytes, part_tag_bytes;
    size_t epochs_since_clear;  // steps enqueued since the tagged words were last zeroed (note_steps)
    size_t steps_counted, tag_clears;  // steps note_steps has counted in all, clears it has enqueued (zg_debug_gpt_age_state)
    bool tags_on;
    // one sequence: ln_1 + c_attn and the attention of a layer as ONE launch (attn_qkv.hip), q and the new k / v row handed over as
    // (value, tag) words [3 E] (tags as above: the embed kernel advances the epoch)
    unsigned long long* qkv_tag;
    size_t qkv_tag_bytes;
    bool fused_on;
    // LayerNorm statistics of x by 16-column tile, written by the producers of x (GemvArgs.st_out / st_in)
    float* xst;
    bool st_on;
    bool pl_on;
    int max_splits, lm_grid;
    // pinned host mirrors for small control traffic
    StepCtrl* h_ctrl;
    int* h_ints;  // [batch * ctx] staging for prompts / tokens
    // graphs [step_index(StepKey)][n_buckets]: one per (step shape, 64-position bucket of seq_len), captured on first use (graph_exec).
    // The bucket's upper bound t_hi is baked into the attention / merge kernels so that their loads
    // do not wait for the exact seq_len (which lives in device memory).
    std::vector<hipGraphExec_t> graphs;
    size_t n_buckets;         // ceil(context / 64)
    int* sampled;             // [batch]: the sampler's draw from the last step's logits
    float* samp_ws;           // segment sums of the sampler (sample_workspace_floats)
    SampleParams* samp;       // device: temperature and seed of the generation in flight
    SampleParams* h_samp;     // pinned mirror
    StepTail gen_tail;        // what follows lm_head in the steps of the generation in flight (normalized)
    FilterWs filt;            // selection workspace of the truncated sampler (sample_filter.h), zero at create
    // logit penalties (sample_penalty.h): the caller's prior / explicit history [batch][ctx] with its lengths, the values
    // of the call in flight, their pinned mirrors (h_prior: [batch * ctx] tokens, then [batch] lengths).  The kernels' table is LDS: no workspace
    int *prior, *prior_len;
    PenParams *pen, *h_pen;
    int* h_prior;
    // log-probabilities (sample_logprob.h): the chunk workspace, top_n of the generation in flight (device word and
    // its place in the pinned control block), the record buffers [batch][ctx] / [batch][ctx][20] and the pinned mirror a fetch
    // copies its columns through ([batch * ctx] log-probabilities, then [batch * ctx * 20] ids, then as many values)
    LogprobWs lp_ws;
    LogprobRec lp_rec;
    int *lp_top, *h_lp_top;
    float* h_lp;
    bool lp_valid;            // the last generation (or zg_gpt_score) recorded them: the record can be fetched
    size_t lp_top_n;          // ... with this many alternatives
    // stop conditions (sample_stop.h): the conditions of the generation in flight, finish column and reason of every
    // row (-1: none), and ONE pinned block: the staging mirror of the conditions, the way back of the two arrays, and the two
    // words the stop kernel stores to (host.progress, host.done_col)
    StopConds* stop;
    int *stop_fin, *stop_reason;
    struct StopPinned {
        StopConds conds;
        int fin[kStopMaxRows], reason[kStopMaxRows];
        alignas(64) StopHost host;
    }* h_stop;
    // logit edits (sample_edit.h): the bias table and, behind it, the keep bitmap of vocab bits — one block in the
    // arena, its pinned mirror, and plain host memory of the same size in which a call's set is built and checked before anything
    // else is touched (edit_build)
    EditTable* edit_tab;
    unsigned* edit_keep;
    char* h_edit;
    std::vector<char> edit_build;
    bool gen_stop;            // the generation in flight has conditions: gen_pump paces itself and may end early
    size_t gen_lookahead;     // ... at most this many steps ahead of host.progress before each piece
    bool stop_valid;          // the last generation was one with conditions: zg_gpt_generate_stop_result can report it
    size_t stop_end;          // ... and ended here
    // scoring (zg_gpt_score; sample_score.h), carved under ZG_GPT_SCORE only: the logits of one block of kScoreRows rows
    // [kScoreRows][sc_v64] (sc_v64 = the vocabulary on the GEMMs' 64-column grid), the chunk workspace of that block, and the lm_head
    // operand the whole-prompt GEMM cannot take from the weight region: bf16 weights — the last vocab % 64 rows of wte as a [64][E]
    // strip, zero rows behind them; fp32 / B24 weights — wte's planes [3][sc_v64][E], zero rows behind the vocabulary, and the
    // slab workspace of that launch.  sc_gen: w_gen + 1 of the weights the strip / planes were made from (0: never made)
    float* sc_logits;
    ScoreWs sc_ws;
    bf16_t *sc_tail, *sc_planes;
    float* sc_gemm_ws;
    size_t sc_gemm_ws_floats, sc_v64, sc_gen;
    size_t w_gen;             // (the owner of a weight region) bumped whenever its wte may have changed
    size_t graph_steps;
    hipStream_t graph_stream;
    size_t steps_enqueued;
    bool ln_folded;  // c2 / c3 of every layer match the weights currently in the arena
    // side-stream L2 prefetcher of the decode chain (prefetch.hip); runs during zg_gpt_generate_enqueue only
    PfCtl* pf_ctl;
    PfJob* pf_jobs;  // [pf_njobs]: embed, 5 per layer, lm_head
    int pf_njobs;
    bool pf_on;
    bool pf_ran;      // a prefetcher was launched by the last generate call
    bool pf_stalled;  // one left on its idle limit (no concurrency with the decode stream, or a host hiccup): sitting out
    int pf_strikes;   // idle-limit exits so far; the third one is final
    int pf_sit_out;   // generate calls left before a stalled prefetcher is tried again
    hipStream_t pf_stream;
    hipEvent_t pf_ev_main, pf_ev_side;
    // independent prompt groups on one GPU (zg_gpt_create_ex): a private stream, so that the decode chains of several handles
    // overlap on the chip, and a weight region borrowed from another handle of the same model
    hipStream_t stream;  // nullptr: the library stream of the moment (zg_set_stream)
    zg_gpt* parent;      // owner of the weight region this handle reads (nullptr: its own)
    bool counted;        // this handle is one of its parent's n_children
    int n_children;      // handles borrowing this one's weight region
    char* wbase;         // the weight region: arena, or the parent's
    // a generation in flight between gen_begin and gen_end (zg_gpt_generate_enqueue / _many)
    size_t gen_pos, gen_n, gen_min_prompt, gen_since_sync;
    bool gen_open;
    // the session: positions the caches hold, and the row behind the last one written since the rows behind a pass
    // were last cleared — a continuation clears [its end, context) only when something may be there
    size_t cached_len, kv_dirty_hi;
};

// rows of pf_x per lm_head block of zg_gpt_score: one constant, decided by one measurement (profiles/NOTEBOOK.md §16: 256 rows take
// the 128 x 256 tiles and half the launches; -DZG_SCORE_ROWS=128 builds the other candidate)
#ifndef ZG_SCORE_ROWS
#define ZG_SCORE_ROWS 256
#endif
constexpr size_t kScoreRows = ZG_SCORE_ROWS;
constexpr size_t kPassTapRowsBehind = ZG_PASS_TAP_ROWS_BEHIND;  // cache rows a tapped pass copies behind its last position

static inline hipStream_t gs(const zg_gpt* g) { return g->stream ? g->stream : ctx().stream; }
static inline zg_gpt* root(zg_gpt* g) { return g->parent ? g->parent : g; }

namespace {

int env_int(const char* name, int dflt) {
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

// the edit stage's block: the bias table, then the keep bitmap of `vocab` bits
size_t edit_block_bytes(size_t vocab) { return sizeof(EditTable) + (vocab + 31) / 32 * 4; }

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
    g->sampled = (int*)P(B * 4);
    g->samp = (SampleParams*)P(sizeof(SampleParams));
    g->samp_ws = (float*)P(sample_workspace_floats((int)B) * 4);
    g->filt = filter_workspace(P(filter_workspace_bytes((int)B)), (int)B);
    g->prior = (int*)P(B * C * 4);
    g->prior_len = (int*)P(B * 4);
    g->pen = (PenParams*)P(sizeof(PenParams));
    g->xp = (bf16_t*)P(E * 48);
    g->hp = (bf16_t*)P(4 * E * 48);
    g->ap = (bf16_t*)P(E * 48);
    g->attn_cnt = (int*)P(8 * c.n_heads * 4);
    g->epoch = (unsigned*)P(256);
    g->xst = (float*)P(((E + 15) / 16) * 8 * 2 * 4);
    g->sk_tag_bytes = ((E + 15) / 16) * 4 * 128 * 8;
    g->part_tag_bytes = 8 * c.n_heads * g->max_splits * kPartStride * 8;
    g->sk_tag = (unsigned long long*)P(g->sk_tag_bytes);
    g->qkv_tag_bytes = 3 * E * 8;
    g->qkv_tag = (unsigned long long*)P(g->qkv_tag_bytes);
    g->part_tag = (unsigned long long*)P(g->part_tag_bytes);
    g->sk_tiles = (int)((E + 15) / 16);
    g->sk_ws = (float*)P((size_t)g->sk_tiles * 4 * 128 * 4);
    g->sk_cnt = (int*)P((size_t)g->sk_tiles * 4 * 4);  // [tile][4]: the four-wave plane-fed kernel takes one ticket per wave
    g->pf_njobs = (int)(2 + 5 * L);
    g->pf_ctl = (PfCtl*)P(sizeof(PfCtl));
    g->pf_jobs = (PfJob*)P((size_t)g->pf_njobs * sizeof(PfJob));
    g->pf_x = g->pf_qkv = g->pf_ws = nullptr;
    g->sk_flags = nullptr;
    g->sk_epoch = 0;
    g->sk_restarts = 0;
    g->sk_used = false;
    g->pf_a = g->pf_h = nullptr;
    g->pf_ws_floats = 0;
    if (!(g->flags & ZG_GPT_NO_PREFILL)) {
        g->pf_x = (float*)P(B * C * E * 4);
        g->pf_qkv = (float*)P(B * C * 3 * E * 4);
        g->pf_a = (bf16_t*)P(B * C * kSplit * E * 2);
        g->pf_h = (bf16_t*)P(B * C * kSplit * 4 * E * 2);
        // split-K partials of the prompt GEMMs; fp32 weights: three weight-plane passes of [B ctx, 4 E] at the least
        g->pf_ws_floats = g->wt == WT_BF16 ? (size_t)(16u << 20) : std::max((size_t)(16u << 20), 3 * B * C * 4 * E);
        g->pf_ws = (float*)P(g->pf_ws_floats * 4);
        g->sk_flags = (unsigned*)P(kSkFlagWords * sizeof(unsigned));
    }
    // (behind everything else: handles that never ask for log-probabilities keep the layout they had)
    g->lp_ws = logprob_workspace(P(logprob_workspace_bytes((int)B, (int)V)), (int)B, (int)V);
    g->lp_top = (int*)P(256);
    g->lp_rec.logprob = (float*)P(B * C * 4);
    g->lp_rec.top_ids = (int*)P(B * C * ZG_LOGPROBS_TOP_MAX * 4);
    g->lp_rec.top_logprobs = (float*)P(B * C * ZG_LOGPROBS_TOP_MAX * 4);
    g->lp_rec.stride = (int)C;
    // (and behind those: handles that never ask for scoring keep the layout they had)
    g->sc_logits = nullptr;
    g->sc_ws = ScoreWs{};
    g->sc_tail = g->sc_planes = nullptr;
    g->sc_gemm_ws = nullptr;
    g->sc_gemm_ws_floats = 0;
    g->sc_v64 = (V + 63) / 64 * 64;
    if ((g->flags & ZG_GPT_SCORE) && !(g->flags & ZG_GPT_NO_PREFILL)) {
        g->sc_logits = (float*)P(kScoreRows * g->sc_v64 * 4);
        g->sc_ws = score_workspace(P(score_workspace_bytes((int)kScoreRows, (int)V)), (int)kScoreRows, (int)V);
        if (g->wt == WT_BF16) {
            if (V % 64) g->sc_tail = (bf16_t*)P(64 * E * 2);
        } else {  // the three-pass GEMM sums its slabs [3][rows][sc_v64] through a workspace: more than pf_ws holds at a real vocabulary
            g->sc_planes = (bf16_t*)P(kSplit * g->sc_v64 * E * 2);
            g->sc_gemm_ws_floats = 3 * kScoreRows * g->sc_v64;
            g->sc_gemm_ws = (float*)P(g->sc_gemm_ws_floats * 4);
        }
    }
    // (and behind everything: the stop stage's conditions and its two words per row; every layout above is what it was)
    g->stop = (StopConds*)P(sizeof(StopConds));
    g->stop_fin = (int*)P(kStopMaxRows * 4);
    g->stop_reason = (int*)P(kStopMaxRows * 4);
    // (and the edit stage's bias table with the keep bitmap behind it)
    g->edit_tab = (EditTable*)P(edit_block_bytes(V));
    g->edit_keep = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(g->edit_tab) + sizeof(EditTable));
    g->state_bytes = (cv.off + 255) & ~(size_t)255;
}

int bucket_t_hi(const zg_gpt* g, size_t seq_len) {
    const size_t hi = ((seq_len + 63) / 64) * 64;
    return (int)(hi < g->cfg.context_size ? hi : g->cfg.context_size);
}

GemvArgs base_gemv(const zg_gpt* g, const void* W, const float* bias, size_t N, size_t K, int t_hi) {
    GemvArgs a{};
    a.t_hi = t_hi;
    a.dbg = ctx().dbg;
    a.zero = ctx().d_zero;
    a.W = W;
    a.bias = bias;
    a.N = (int)N;
    a.K = (int)K;
    a.M = (int)g->batch;
    a.eps = 1e-5f;  // LayerNorm.eps default, ops.zig:76
    a.ctrl = g->ctrl;
    a.n_heads = (int)g->cfg.n_heads;
    a.head_dim = 64;
    a.max_splits = g->max_splits;
    a.ctx = (int)g->cfg.context_size;
    a.kv_mode = g->kv_mode;
    a.kv_lo = g->batch * g->cfg.context_size * g->cfg.n_embed * 2;
    a.sk_ws = g->sk_ws;
    a.sk_cnt = g->sk_cnt;
    a.sk_tiles = g->sk_tiles;
    a.progress = g->pf_on ? &g->pf_ctl->progress : nullptr;
    return a;
}

EmbedArgs embed_args(const zg_gpt* g, int finish_only) {
    EmbedArgs e{};
    e.ctrl = g->ctrl;
    e.wte = g->wte;
    e.wpe = g->wpe;
    e.weight_type = g->wt;
    e.n_embed = (int)g->cfg.n_embed;
    e.batch = (int)g->batch;
    e.vocab = (int)g->cfg.vocab_size;
    e.prompt = g->prompt;
    e.prompt_stride = (int)g->cfg.context_size;
    e.prompt_len = g->prompt_len;
    e.forced = g->forced;
    e.cur_token = g->cur_token;
    e.out_tokens = g->out_tokens;
    e.out_stride = (int)g->cfg.context_size;
    e.part_val = g->part_val;
    e.part_idx = g->part_idx;
    e.part_stride = g->lm_grid;  // the lm_head GEMV writes partials [batch][gridDim.x]
    e.n_partials = g->lm_grid;
    e.x = g->x;
    e.pl_out = g->pl_on ? g->xp : nullptr;
    e.pl_g = g->layers[0].ln_1_g;
    e.epoch = (((g->pl_on && g->tags_on) || g->fused_on) && finish_only != 1 && finish_only != 2) ? g->epoch : nullptr;
    e.st_out = g->st_on ? g->xst : nullptr;
    e.finish_only = finish_only;
    e.progress = g->pf_on ? &g->pf_ctl->progress : nullptr;
    e.sampled = g->sampled;
    return e;
}

// A planned decode launch: enqueue it, or (rec != nullptr: building the prefetcher's job table at create) describe
// the weight tiles its workgroups read.
int emit_gemv(const zg_gpt* g, const GemvArgs& a, const GemvPlan& p, hipStream_t s, std::vector<PfJob>* rec, unsigned cls) {
    if (!rec) return launch_gemv(a, p, g->wt, s);
    PfJob j{};
    j.cls = cls;
    const int rows = p.rows_per_wg;
    if (rows > 0) {
        j.kind = PF_WEIGHTS;
        j.base = reinterpret_cast<const char*>(a.W);
        j.total_bytes = (size_t)a.N * a.K * g->wbytes;
        j.wg_bytes = (unsigned)((size_t)rows * a.K * g->wbytes);
        j.n_wg = (unsigned)p.pf_tiles;
        j.touch_bytes = j.wg_bytes;
        if (a.M == 1) {
            const bool lnk = a.prologue == PRO_LAYERNORM && a.ln_c2 != nullptr;
            const float* v[3] = {lnk ? a.ln_g : nullptr, lnk ? a.ln_c2 : a.bias, lnk ? a.ln_c3 : nullptr};
            const size_t n[3] = {(size_t)a.K * 4, (size_t)a.N * 4, (size_t)a.N * 4};
            for (int i = 0; i < 3; ++i) {
                j.aux[i] = reinterpret_cast<const char*>(v[i]);
                j.aux_bytes[i] = v[i] ? (unsigned)n[i] : 0u;
            }
        }
        // a matrix far larger than the L2s (lm_head): only the head of every tile, about 16 MiB in all
        const size_t cap = (size_t)16 << 20;
        if (j.total_bytes > cap) j.touch_bytes = (unsigned)(((size_t)j.wg_bytes * cap / j.total_bytes + 127) & ~(size_t)127);
    }
    rec->push_back(j);
    return ZG_OK;
}

// Optional per-kernel event recorder (zg_gpt_profile_step only).
struct StepProf {
    std::vector<hipEvent_t> ev;
    std::vector<int> cls;  // kernel class of the interval ENDING at ev[i]
    size_t n = 0;
};
inline int prof_mark(StepProf* p, int cls, hipStream_t s) {
    if (!p) return ZG_OK;
    if (p->n == p->ev.size()) {
        hipEvent_t e;
        ZG_HIP(hipEventCreate(&e));
        p->ev.push_back(e);
        p->cls.push_back(cls);
    }
    p->cls[p->n] = cls;
    ZG_HIP(hipEventRecord(p->ev[p->n++], s));
    return ZG_OK;
}

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

// (Re)derive what the scoring lm_head reads beside the weight region (the tail strip, or wte's planes) from the wte in the arena:
// after ZG_WTE was loaded, and on handles whose region was filled some other way (a borrowed region, a broadcast).
int ensure_score_weights(zg_gpt* g, hipStream_t s) {
    if (!g->sc_logits || g->sc_gen == root(g)->w_gen + 1) return ZG_OK;
    const size_t E = g->cfg.n_embed, V = g->cfg.vocab_size, head = V / 64 * 64;
    if (g->wt != WT_BF16) ZG_TRY(launch_wte_planes(g->wte, g->wt, V, g->sc_v64, (int)E, g->sc_planes, s));
    else if (g->sc_tail) {
        ZG_HIP(hipMemsetAsync(g->sc_tail, 0, 64 * E * 2, s));
        ZG_HIP(hipMemcpyAsync(g->sc_tail, reinterpret_cast<const bf16_t*>(g->wte) + head * E, (V - head) * E * 2, hipMemcpyDeviceToDevice, s));
    }
    g->sc_gen = root(g)->w_gen + 1;
    return ZG_OK;
}

// The arguments of the decode launches of a Block and of lm_head, one builder per launch class: enqueue_step launches what they
// return, and zg_gpt_create plans (gemv_plan) the very same arguments.  The decode modes they lay the arguments out for are
// passed in: the handle's own (modes_of) for a step, a candidate while zg_gpt_create decides them.
struct StepModes {
    bool pl, st, tags;  // as zg_gpt pl_on / st_on / tags_on
};
inline StepModes modes_of(const zg_gpt* g) { return StepModes{g->pl_on, g->st_on, g->tags_on}; }

// ln_1 + c_attn + split_qkv + cache append (main.zig:121-123, ops.zig:143-157) and the attention over the cache (ops.zig:160 ->
// :249-307) of layer y: the arguments of their launches
GemvArgs c_attn_args(const zg_gpt* g, const zg_layer& y, int t_hi, const StepModes& m) {
    const size_t E = g->cfg.n_embed;
    GemvArgs a = base_gemv(g, y.c_attn_w, y.c_attn_b, 3 * E, E, t_hi);
    a.prologue = PRO_LAYERNORM;
    a.x = g->x;
    a.x_stride = (int)E;
    a.ln_g = y.ln_1_g;
    a.ln_b = y.ln_1_b;
    a.ln_c2 = y.c_attn_c2;
    a.ln_c3 = y.c_attn_c3;
    a.epilogue = EPI_QKV;
    a.pl_in = m.pl ? g->xp : nullptr;
    a.st_in = m.st ? g->xst : nullptr;
    a.q = g->q;
    a.k_cache = y.k_cache;
    a.v_cache = y.v_cache;
    return a;
}

AttnArgs attn_args(const zg_gpt* g, const zg_layer& y, int t_hi) {
    const size_t E = g->cfg.n_embed;
    AttnArgs a{};
    a.q = g->q;
    a.k = y.k_cache;
    a.v = y.v_cache;
    a.stride_b = (long)(g->cfg.context_size * E);
    a.stride_h = (long)(g->cfg.context_size * 64);
    a.stride_t = 64;
    a.kv_mode = g->kv_mode;
    a.kv_lo = g->batch * g->cfg.context_size * E * 2;
    a.n_heads = (int)g->cfg.n_heads;
    a.head_dim = 64;
    a.batch = (int)g->batch;
    a.ctrl = g->ctrl;
    a.t_hi = t_hi;
    a.max_splits = g->max_splits;
    a.part = g->part;
    a.progress = g->pf_on ? &g->pf_ctl->progress : nullptr;
    a.tail_off = g->tail_off;
    a.dbg = ctx().dbg;
    return a;
}

// merge heads + attn c_proj + residual: ops.zig:171-172, main.zig:136-139
GemvArgs c_proj_args(const zg_gpt* g, const zg_layer& y, int t_hi, const StepModes& m) {
    const size_t E = g->cfg.n_embed;
    GemvArgs a = base_gemv(g, y.c_proj_w, y.c_proj_b, E, E, t_hi);
    a.prologue = PRO_ATTN_MERGE;
    a.part = g->part;
    a.epilogue = EPI_RESIDUAL;
    a.y = g->x;
    a.y_stride = (int)E;
    a.resid = g->x;
    a.resid_stride = (int)E;
    if (m.pl) {  // the heads arrive merged, as planes
        a.prologue = PRO_NONE;
        a.pl_in = g->ap;
        a.pl_out = g->xp;
        a.pl_g = y.ln_2_g;
        a.st_out = m.st ? g->xst : nullptr;
    }
    return a;
}

// ln_2 + c_fc + gelu: main.zig:140, :79-80
GemvArgs c_fc_args(const zg_gpt* g, const zg_layer& y, int t_hi, const StepModes& m) {
    const size_t E = g->cfg.n_embed;
    GemvArgs a = base_gemv(g, y.c_fc_w, y.c_fc_b, 4 * E, E, t_hi);
    a.prologue = PRO_LAYERNORM;
    a.x = g->x;
    a.x_stride = (int)E;
    a.ln_g = y.ln_2_g;
    a.ln_b = y.ln_2_b;
    a.ln_c2 = y.c_fc_c2;
    a.ln_c3 = y.c_fc_c3;
    a.epilogue = EPI_GELU;
    a.y = g->h4;
    a.y_stride = (int)(4 * E);
    if (m.pl) {  // gelu(c_fc) leaves as planes only
        a.st_in = m.st ? g->xst : nullptr;
        a.pl_in = g->xp;
        a.pl_out = g->hp;
        a.y = nullptr;
    }
    return a;
}

// mlp c_proj + residual of layer l (main.zig:81, :142-145).  A tagged hand-over gets everything but its launch id, which is the
// caller's to give (a.sk_tag != nullptr says that one is due).
GemvArgs mlp_proj_args(const zg_gpt* g, size_t l, int t_hi, const StepModes& m) {
    const size_t E = g->cfg.n_embed;
    const zg_layer& y = g->layers[l];
    GemvArgs a = base_gemv(g, y.mlp_proj_w, y.mlp_proj_b, E, 4 * E, t_hi);
    a.prologue = PRO_NONE;
    a.x = g->h4;
    a.x_stride = (int)(4 * E);
    a.epilogue = EPI_RESIDUAL;
    a.y = g->x;
    a.y_stride = (int)E;
    a.resid = g->x;
    a.resid_stride = (int)E;
    if (m.pl) {
        if (m.tags && 2 * l + 2 <= 255) {
            a.epoch = g->epoch;
            a.sk_tag = g->sk_tag;
            a.fault = g->fault;
            a.spin_limit = g->spin_limit;
        }
        a.pl_in = g->hp;
        if (l + 1 < g->cfg.n_layer) {  // the next Block's ln_1 + c_attn (ln_f + lm_head reads x itself)
            a.pl_out = g->xp;
            a.pl_g = g->layers[l + 1].ln_1_g;
            a.st_out = m.st ? g->xst : nullptr;
        }
    }
    return a;
}

// ln_f (main.zig:189) + lm_head = wte, no bias (main.zig:192-194, :312) + greedy partial argmax
GemvArgs lm_head_args(const zg_gpt* g) {
    const size_t E = g->cfg.n_embed, V = g->cfg.vocab_size;
    GemvArgs a = base_gemv(g, g->wte, nullptr, V, E, 0);
    a.prologue = PRO_LAYERNORM;
    a.x = g->x;
    a.x_stride = (int)E;
    a.ln_g = g->ln_f_g;
    a.ln_b = g->ln_f_b;
    a.ln_c2 = g->lm_c2;
    a.ln_c3 = g->lm_c3;
    a.epilogue = EPI_ARGMAX;  // (the plan depends on the epilogue: workgroup width)
    a.logits = g->logits;
    a.logits_stride = (int)V;
    a.part_val = g->part_val;
    a.part_idx = g->part_idx;
    return a;
}

int enqueue_lm_head(zg_gpt* g, hipStream_t s, std::vector<PfJob>* rec = nullptr) {
    const GemvArgs a = lm_head_args(g);
    const GemvPlan p = gemv_plan(a, g->wt);
    ZG_REQUIRE(p.grid == g->lm_grid, ZG_ERR_ARG, "lm_head grid changed");
    return emit_gemv(g, a, p, s, rec, 6);
}

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
        if (g->pl_on) ZG_TRY(whole(ZG_TAP_XP, ZG_TAP_BF16, g->xp, E * 48, flags | (planes_written ? 0u : ZG_TAP_NOT_WRITTEN)));
        if (g->st_on) ZG_TRY(whole(ZG_TAP_XST, ZG_TAP_F32, g->xst, ((E + 15) / 16) * 8 * 2 * 4, flags | (planes_written ? 0u : ZG_TAP_NOT_WRITTEN)));
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
            if (g->pl_on) return whole(ZG_TAP_AP, ZG_TAP_BF16, g->ap, E * 48, flags);
            return whole(ZG_TAP_PART, ZG_TAP_F32, g->part, B * H * g->max_splits * kPartStride * 4, flags);
        case 3: return x_side(true);
        case 4:
            if (g->pl_on) return whole(ZG_TAP_HP, ZG_TAP_BF16, g->hp, 4 * E * 48, flags);
            return whole(ZG_TAP_H4, ZG_TAP_F32, g->h4, B * 4 * E * 4, flags);
        case 5: return x_side(l + 1 < g->cfg.n_layer);
        default:
            ZG_TRY(whole(ZG_TAP_LOGITS, ZG_TAP_F32, g->logits, B * V * 4, flags));
            ZG_TRY(tap_put(t, cls, l, ZG_TAP_PART_VAL, ZG_TAP_F32, flags, g->part_val, B, (size_t)g->lm_grid * 4, (size_t)g->lm_grid * 4, s));
            return tap_put(t, cls, l, ZG_TAP_PART_IDX, ZG_TAP_I32, flags, g->part_idx, B, (size_t)g->lm_grid * 4, (size_t)g->lm_grid * 4, s);
    }
}

// The history the penalty stage of a handle reads: the prior buffer alone (zg_gpt_sample_pen: the caller's explicit history), or
// followed by the generate loop's own record from PenParams.past_len on
PenHistory pen_history(const zg_gpt* g, bool loop) {
    PenHistory h{};
    h.prior = g->prior;
    h.prior_len = g->prior_len;
    h.prior_stride = (int)g->cfg.context_size;
    if (loop) {
        h.rec = g->out_tokens;
        h.rec_stride = (int)g->cfg.context_size;
        h.ctrl = g->ctrl;
    }
    h.max_hist = (int)g->cfg.context_size;  // (the entry points hold prior + recorded tokens to the context)
    return h;
}

// What the sampler chain — penalties, edits, selection launches, sampler — reads and writes.  The draw comes from one of two
// sources: the loop's control block (ctrl: the uniform is the counter PRNG of the position it holds), or a per-call buffer of
// uniforms (u, with the call's temperature and whether the probabilities are written back over the row).
struct SamplerChain {
    float* logits;
    int batch, vocab;
    float* part_val;  // row-maximum partials [batch][n_part] as lm_head's epilogue leaves them, and their indices
    int* part_idx;
    int n_part;
    const PenParams* pen;
    PenHistory hist;
    unsigned* counts;  // (zg_debug_penalize_rows: the counts of every row's history)
    const EditTable* edit_tab;
    const unsigned* edit_keep;
    const SampleParams* params;
    float* seg_ws;
    FilterWs filt;
    const StepCtrl* ctrl;  // the loop's draws ...
    const float* u;        // ... or a call's
    float temp;
    bool write_probs;
    int* pick;
};

// The chain of a handle: the loop's (draws by its control block into `sampled`, history = prior + its own record), or that of a
// per-token call, whose draw source and destination are the caller's to add
SamplerChain handle_chain(const zg_gpt* g, bool loop) {
    SamplerChain c{};
    c.logits = g->logits, c.batch = (int)g->batch, c.vocab = (int)g->cfg.vocab_size;
    c.part_val = g->part_val, c.part_idx = g->part_idx, c.n_part = g->lm_grid;
    c.pen = g->pen, c.hist = pen_history(g, loop);
    c.edit_tab = g->edit_tab, c.edit_keep = g->edit_keep;
    c.params = g->samp, c.seg_ws = g->samp_ws, c.filt = g->filt;
    if (loop) c.ctrl = g->ctrl, c.pick = g->sampled;
    return c;
}

// The launches of tail t behind lm_head, up to the pick: GPT.sample's tail (main.zig:200-206) behind the stages that rewrite the
// row.  Launches only — what they read is staged by the caller (enqueue_step runs under capture).  A GREEDY tail has no sampler
// launch: the partials are the pick.
int emit_sampler_chain(const SamplerChain& c, StepTail t, hipStream_t s) {
    // the penalties act on the raw logits, the edits on the row the penalties leave (HF's processor order); the row-maximum
    // partials every sampler starts from are rebuilt only behind the LAST stage that rewrites the row — the edit launch does it itself
    if (t.pen) ZG_TRY(launch_penalize(c.logits, c.batch, c.vocab, c.pen, c.hist, c.part_val, c.part_idx, c.n_part, c.counts, s, !t.edit));
    if (t.edit) ZG_TRY(launch_logit_edit(c.logits, c.batch, c.vocab, c.edit_tab, c.edit_keep, c.part_val, c.part_idx, c.n_part, s));
    if (t.sampler == GREEDY) return ZG_OK;
    if (threshold_sampler(t.sampler))  // a filter or min-p: the selection launches, then the tail kernels that read tau
        return launch_sample_filtered(c.logits, c.batch, c.vocab, c.params, filter_launches(t.sampler), c.u, c.ctrl, c.part_val, c.n_part, c.n_part, c.seg_ws,
                                      c.filt, c.pick, c.write_probs, s);
    if (c.ctrl) return launch_sample_step(c.logits, c.batch, c.vocab, c.params, c.ctrl, c.part_val, c.n_part, c.n_part, c.seg_ws, c.pick, s);
    return launch_sample(c.logits, c.batch, c.vocab, c.temp, c.u, c.part_val, c.n_part, c.n_part, c.seg_ws, c.pick, c.write_probs, s);
}

// One decode step = GPT.forward (main.zig:178-195) for all sequences.
int enqueue_step(zg_gpt* g, bool with_logits, int t_hi, hipStream_t s, const StepOpts& o = StepOpts()) {
    StepProf* const prof = o.prof;
    std::vector<PfJob>* const rec = o.rec;
    const int only = o.only;
    auto launch_id = [&](size_t l, int k) { return (unsigned)(o.salt >= 0 ? 1 + (2 * o.salt + k) % 254 : 2 * (int)l + 1 + k); };
    const StepModes m = modes_of(g);
    auto gemv = [&](const GemvArgs& a, unsigned cls) {
        ZG_TRY(emit_gemv(g, a, gemv_plan(a, g->wt), s, rec, cls));
        return prof_mark(prof, (int)cls, s);
    };
    ZG_TRY(prof_mark(prof, -1, s));
    if (rec) rec->push_back(PfJob{});
    else if (only < 0 || only == 0) {
        EmbedArgs e = embed_args(g, only == 0 ? 3 : 0);  // main.zig:179-183
        ZG_TRY(launch_embed_step(e, s));
        ZG_TRY(tap_class(g, o.taps, 0, 0, 0, s));
    }
    ZG_TRY(prof_mark(prof, 0, s));
    for (size_t l = (only < 0 ? 0 : o.only_layer); l < (only < 0 ? g->cfg.n_layer : o.only_layer + 1); ++l) {
        const zg_layer& y = g->layers[l];
        // one sequence: classes 1 and 2 as one launch (attn_qkv.hip), timed as class 1; the prefetcher's table keeps both entries
        const bool fused = g->fused_on && !rec && 2 * l + 2 <= 255;
        ZG_TRY(tap_class(g, o.taps, -1, l, 0, s));
        if (fused && (only < 0 || only == 1)) {
            const GemvArgs a = c_attn_args(g, y, t_hi, m);
            AttnArgs at = attn_args(g, y, t_hi);
            at.launch_id = launch_id(l, 0);
            at.fault = g->fault;
            at.spin_limit = g->spin_limit;
            ZG_TRY(launch_attn_qkv(a, gemv_plan(a, g->wt), g->wt, at, g->epoch, g->qkv_tag, s));
            ZG_TRY(prof_mark(prof, 1, s));
            ZG_TRY(prof_mark(prof, 2, s));
            ZG_TRY(tap_class(g, o.taps, 1, l, ZG_TAP_FUSED, s));
            ZG_TRY(tap_class(g, o.taps, 2, l, ZG_TAP_FUSED, s));
        }
        if (!fused && (only < 0 || only == 1)) {
            ZG_TRY(gemv(c_attn_args(g, y, t_hi, m), 1));
            ZG_TRY(tap_class(g, o.taps, 1, l, 0, s));
        }
        if ((!fused && only < 0) || only == 2) {   // scaled_dot_product_attention over the cache: ops.zig:160 -> :249-307
            AttnArgs a = attn_args(g, y, t_hi);
            if (g->pl_on) {
                a.pl_out = g->ap;
                a.merge_cnt = g->attn_cnt;
                if (g->tags_on && 2 * l + 2 <= 255) {
                    a.epoch = g->epoch;
                    a.launch_id = launch_id(l, 0);
                    a.part_tag = g->part_tag;
                    a.fault = g->fault;
                    a.spin_limit = g->spin_limit;
                }
            }
            if (rec) {  // the K and V rows of earlier positions, laid out for this grid
                PfJob j{};
                j.kind = PF_KV;
                j.cls = 2;
                j.base = reinterpret_cast<const char*>(y.k_cache);
                j.base2 = reinterpret_cast<const char*>(y.v_cache);
                j.n_heads = (unsigned)g->cfg.n_heads;
                j.ctx = (unsigned)g->cfg.context_size;
                j.batch = (unsigned)g->batch;
                j.row_bytes = g->kv_mode ? 128u : 256u;  // (B24: the bf16 plane; its byte plane is left to the kernel)
                rec->push_back(j);
            } else
                ZG_TRY(launch_attn_decode(a, s));
            ZG_TRY(prof_mark(prof, 2, s));
            ZG_TRY(tap_class(g, o.taps, 2, l, 0, s));
        }
        if (only < 0 || only == 3) {
            ZG_TRY(gemv(c_proj_args(g, y, t_hi, m), 3));
            ZG_TRY(tap_class(g, o.taps, 3, l, 0, s));
        }
        if (only < 0 || only == 4) {
            ZG_TRY(gemv(c_fc_args(g, y, t_hi, m), 4));
            ZG_TRY(tap_class(g, o.taps, 4, l, 0, s));
        }
        if (only < 0 || only == 5) {
            GemvArgs a = mlp_proj_args(g, l, t_hi, m);
            if (a.sk_tag) a.launch_id = launch_id(l, 1);
            ZG_TRY(gemv(a, 5));
            ZG_TRY(tap_class(g, o.taps, 5, l, 0, s));
        }
    }
    if (with_logits && (only < 0 || only == 6)) {
        ZG_TRY(enqueue_lm_head(g, s, rec));
        ZG_TRY(prof_mark(prof, 6, s));
        ZG_TRY(tap_class(g, o.taps, 6, 0, 0, s));
    }
    // GPT.sample's tail (main.zig:200-206) on the logits of this step: the next step's embed kernel feeds what it draws (mode 2)
    // the log-probability stage reads the row the sampler read and the token the next step's embed kernel will record
    auto logprobs = [&](const int* tokens) {
        return launch_logprob(g->logits, (int)g->batch, (int)g->cfg.vocab_size, g->part_val, g->part_idx, g->lm_grid, g->lm_grid, g->lp_top, g->lp_ws,
                              tokens, g->ctrl, g->prompt_len, g->lp_rec, s);
    };
    // the stop stage, last: it learns the pick of its own step the way the log-probability stage does
    auto stop = [&](const int* picks) {
        StopArgs a{};
        a.conds = g->stop;
        a.tokens = g->out_tokens;
        a.stride = (int)g->cfg.context_size;
        a.prompt_len = g->prompt_len;
        a.batch = (int)g->batch;
        a.vocab = (int)g->cfg.vocab_size;
        a.ctrl = g->ctrl;
        a.col = -1;
        a.picks = picks;
        a.part_val = g->part_val;
        a.part_idx = g->part_idx;
        a.n_part = a.part_stride = g->lm_grid;
        a.finish_col = g->stop_fin;
        a.reason = g->stop_reason;
        a.host = &g->h_stop->host;
        return launch_stop(a, s);
    };
    const StepTail tail = o.tail;
    if (!with_logits || only >= 0 || rec) return ZG_OK;
    const int* const picks = tail.sampler == GREEDY ? nullptr : g->sampled;  // (the greedy graphs have no sampler node)
    ZG_TRY(emit_sampler_chain(handle_chain(g, true), tail, s));
    if (tail.lp) ZG_TRY(logprobs(picks));
    if (tail.stop) ZG_TRY(stop(picks));
    return ZG_OK;
}

// The epoch of the next stream-K launch (gemm_s4.hip SK: the producer stores it into sk_flags, the consumer waits until its flag
// word equals it).  One per layer per pass in 32 bits: days of continuous prefill wrap it.  0 is what every flag word holds that no
// launch has written, and behind the wrap a small value is what a word may still hold from the handle's first launches — a
// consumer would take a half tile nobody produced, with no fault raised.  So 0 is never handed out, and where the count begins
// again the flag words are zeroed on the stream in front of the launch (as note_steps does for the decode tags): every word then
// holds 0, and from there on every epoch handed out is larger than every word written before it.
int next_sk_epoch(zg_gpt* g, hipStream_t s, unsigned* out) {
    if (++g->sk_epoch == 0u) {
        ZG_HIP(hipMemsetAsync(g->sk_flags, 0, kSkFlagWords * sizeof(unsigned), s));
        g->sk_epoch = 1u;
        ++g->sk_restarts;
    }
    *out = g->sk_epoch;
    return ZG_OK;
}

// Whole-prompt forward of positions 0..P-1 of every sequence (tokens in g->prompt): fills the KV caches
// exactly as P calls of GPT.forward would (main.zig:331-334) and leaves the residual stream of all rows in
// pf_x.  With `last_block_full` false the last Block stops after its cache append: nothing downstream of
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
int enqueue_prefill(zg_gpt* g, size_t pos0, size_t P, bool last_block_full, hipStream_t s, StepTaps* taps = nullptr) {
    const bool f32w = g->wt != WT_BF16;
    const int np = f32w ? kWeightPlanes : (g->flags & ZG_GPT_PREFILL_2PLANE) ? 2 : kSplit;
    const size_t E = g->cfg.n_embed, L = g->cfg.n_layer, H = g->cfg.n_heads, C = g->cfg.context_size;
    const int B = (int)g->batch, M = (int)(g->batch * P), iE = (int)E;
    const size_t Mz = (size_t)M, T_tap = std::min(C, pos0 + P + kPassTapRowsBehind);
    PrefillGemmPlan plan{};
    PrefillGemmPlan* const plan_out = taps ? &plan : nullptr;
    auto tap_x = [&](int cls, size_t l) { return taps ? tap_put(taps, cls, l, ZG_TAP_X, ZG_TAP_F32, 0, g->pf_x, 1, Mz * E * 4, Mz * E * 4, s) : ZG_OK; };
    auto tap_a = [&](int cls, size_t l, unsigned f) {
        return taps ? tap_put(taps, cls, l, ZG_TAP_A, ZG_TAP_BF16, f, g->pf_a, 1, Mz * kSplit * E * 2, Mz * kSplit * E * 2, s) : ZG_OK;
    };
    auto tap_plan = [&](int cls, size_t l) {
        if (!taps) return (int)ZG_OK;
        int v[ZG_PREFILL_PLAN_INTS];
        prefill_plan_ints(plan, v);
        return tap_words(taps, cls, l, ZG_TAP_PLAN, v, ZG_PREFILL_PLAN_INTS);
    };
    ZG_TRY(launch_embed_prefill(g->prompt, (int)C, B, (int)P, g->wte, g->wpe, g->wt, iE, g->pf_x, s, (int)pos0));
    ZG_TRY(tap_x(0, 0));
    ZG_TRY(launch_ln_split(g->pf_x, M, iE, g->layers[0].ln_1_g, g->layers[0].ln_1_b, 1e-5f, g->pf_a, s));
    ZG_TRY(tap_a(1, 0, 0));
    for (size_t l = 0; l < L; ++l) {
        const zg_layer& y = g->layers[l];
        // pf_a holds split(ln_1(x)) here: from the line above or from the tail of the previous Block's last GEMM
        // c_attn with the cache append of ops.zig:152-157 in its epilogue
        PrefillQkv qa{(int)P, iE, (int)H, (int)C, g->kv_mode, y.k_cache, y.v_cache, g->batch * C * E * 2};
        qa.pos0 = (int)pos0;
        if (!f32w && g->sk_flags != nullptr) {  // (the persistent GEMM may hand half tiles over between workgroups: gemm_s4.hip SK)
            qa.sk_ws = g->pf_ws;
            qa.sk_ws_bytes = g->pf_ws_floats * 4;
            qa.sk_flags = g->sk_flags;
            qa.sk_flags_words = (unsigned)kSkFlagWords;
            ZG_TRY(next_sk_epoch(g, s, &qa.sk_epoch));
            g->sk_used = true;
        }
        if (taps) ZG_TRY(tap_caches(g, taps, -1, l, 0, T_tap, s));
        ZG_TRY(launch_prefill_gemm(g->pf_a, f32w ? y.c_attn_p : (const bf16_t*)y.c_attn_w, y.c_attn_b, g->pf_qkv, M, 3 * iE, iE, 3 * iE, PF_QKV,
                                   g->pf_ws, g->pf_ws_floats, nullptr, s, &qa, np, nullptr, plan_out));
        if (taps) {  // q, then the k | v columns: the persistent kernel leaves those to an fp32 cache (gemm_s4.hip S4_QKV)
            const unsigned kv_cols = plan.family == PFF_S4 && g->kv_mode == 0 ? ZG_TAP_NOT_WRITTEN : 0u;
            ZG_TRY(tap_plan(2, l));
            ZG_TRY(tap_put(taps, 2, l, ZG_TAP_Q, ZG_TAP_F32, 0, g->pf_qkv, Mz, E * 4, 3 * E * 4, s));
            ZG_TRY(tap_put(taps, 2, l, ZG_TAP_QKV_KV, ZG_TAP_F32, kv_cols, g->pf_qkv + E, Mz, 2 * E * 4, 3 * E * 4, s));
            ZG_TRY(tap_caches(g, taps, 2, l, 0, T_tap, s));
        }
        if (l + 1 == L && !last_block_full) break;
        // K and V: the caches — except a whole prompt on an fp16 / B24 cache, which reads the unrounded k / v columns of qkv (an fp32
        // cache is read directly: the c_attn epilogue then need not store those columns)
        PrefillKv kv;
        if (pos0 > 0 || g->kv_mode == 0) kv = PrefillKv{y.k_cache, y.v_cache, g->kv_mode, g->batch * C * E * 2, (int)C};
        int ran[3] = {0, 0, 0};
        ZG_TRY(launch_attn_prefill(g->pf_qkv, g->pf_a, B, (int)pos0, (int)P, iE, (int)H, g->pf_ws, g->pf_ws_floats, kv, s, 0, taps ? ran : nullptr));
        if (taps) ZG_TRY(tap_words(taps, 3, l, ZG_TAP_GEO, ran, 3));
        ZG_TRY(tap_a(3, l, 0));
        const PrefillLn ln2{y.ln_2_g, y.ln_2_b, 1e-5f, g->pf_a};
        ZG_TRY(launch_prefill_gemm(g->pf_a, f32w ? y.c_proj_p : (const bf16_t*)y.c_proj_w, y.c_proj_b, g->pf_x, M, iE, iE, iE, PF_RESID, g->pf_ws,
                                   g->pf_ws_floats, &ln2, s, nullptr, np, nullptr, plan_out));
        ZG_TRY(tap_plan(4, l));
        ZG_TRY(tap_x(4, l));
        ZG_TRY(tap_a(4, l, 0));
        ZG_TRY(launch_prefill_gemm(g->pf_a, f32w ? y.c_fc_p : (const bf16_t*)y.c_fc_w, y.c_fc_b, g->pf_h, M, 4 * iE, iE, 0, PF_GELU_SPLIT, g->pf_ws,
                                   g->pf_ws_floats, nullptr, s, nullptr, np, nullptr, plan_out));
        ZG_TRY(tap_plan(5, l));
        if (taps) ZG_TRY(tap_put(taps, 5, l, ZG_TAP_HP, ZG_TAP_BF16, 0, g->pf_h, 1, Mz * kSplit * 4 * E * 2, Mz * kSplit * 4 * E * 2, s));
        const bool more = l + 1 < L;
        const PrefillLn ln1{more ? g->layers[l + 1].ln_1_g : nullptr, more ? g->layers[l + 1].ln_1_b : nullptr, 1e-5f, g->pf_a};
        ZG_TRY(launch_prefill_gemm(g->pf_h, f32w ? y.mlp_proj_p : (const bf16_t*)y.mlp_proj_w, y.mlp_proj_b, g->pf_x, M, iE, 4 * iE, iE, PF_RESID, g->pf_ws,
                                   g->pf_ws_floats, more ? &ln1 : nullptr, s, nullptr, np, nullptr, plan_out));
        ZG_TRY(tap_plan(6, l));
        ZG_TRY(tap_x(6, l));
        ZG_TRY(tap_a(6, l, more ? 0u : ZG_TAP_NOT_WRITTEN));
    }
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
    if (g->sk_used) {  // a whole-prompt pass may have handed half tiles over inside gemm_s4: did a consumer give up waiting?
        g->sk_used = false;
        ZG_TRY(gemm_s4_fault(&sk));
    }
    if (g->tags_on || g->fused_on) {
        volatile unsigned* f = g->fault;
        tag = *f;
        if (tag) *f = 0;
    }
    if (sk) {
        set_error("a half-tile hand-over of the whole-prompt c_attn GEMM timed out%s: results discarded", tag ? " (and a tagged hand-over of the decode step)" : "");
        return ZG_ERR_HIP;
    }
    if (tag) {
        set_error("a tagged hand-over of the decode step timed out (a workgroup waited %u polls for its writers): results discarded", g->spin_limit);
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
    if (!g->tags_on && !g->fused_on) return ZG_OK;
    g->epochs_since_clear += n;
    g->steps_counted += n;
    if (g->epochs_since_clear < ((size_t)1 << 23)) return ZG_OK;
    g->epochs_since_clear = n;
    ++g->tag_clears;
    ZG_HIP(hipMemsetAsync(g->sk_tag, 0, g->sk_tag_bytes, s));
    ZG_HIP(hipMemsetAsync(g->part_tag, 0, g->part_tag_bytes, s));
    ZG_HIP(hipMemsetAsync(g->qkv_tag, 0, g->qkv_tag_bytes, s));
    return ZG_OK;
}

// Side-stream prefetcher (prefetch.hip): job table, control block, low-priority stream.  Called from zg_gpt_create
// BEFORE the graphs are captured (the decode kernels get the progress counter as an argument).
int setup_prefetcher(zg_gpt* g) {
    // Default: only where it was measured to pay — one sequence and Linears of a few MB (GPT-2 124M: 241 -> 224 us per
    // token; GPT-2 XL's 20 MB matrices cannot be fetched a launch ahead, 8 prompts gain < 1 %).  ZGPT2_PREFETCH=1 / 0 forces.
    // (not beside co-running handles: a handle with a private stream is one of several chains on the chip — §3.3 of DESIGN.md — and
    // the prefetcher's per-XCD placement follows ONE queue's block order; each would also park 96 polling workgroups)
    const bool small = g->stream == nullptr && g->batch == 1 && 4 * g->cfg.n_embed * g->cfg.n_embed * g->wbytes <= ((size_t)6 << 20);
    const int want = env_int("ZGPT2_PREFETCH", small ? 1 : 0);
    if ((g->flags & ZG_GPT_NO_PREFETCH) || !want || gs(g) == nullptr) return ZG_OK;
    if (g->pf_njobs > 255) return ZG_OK;  // the progress word counts launches in 8 bits (n_layer >= 51): no prefetcher, not an error
    std::vector<PfJob> jobs;
    StepOpts describe;
    describe.rec = &jobs;
    ZG_TRY(enqueue_step(g, true, (int)g->cfg.context_size, nullptr, describe));
    ZG_REQUIRE((int)jobs.size() == g->pf_njobs, ZG_ERR_ARG, "prefetcher: %zu launches per step", jobs.size());
    ZG_HIP(hipMemcpy(g->pf_jobs, jobs.data(), jobs.size() * sizeof(PfJob), hipMemcpyHostToDevice));
    int least = 0, greatest = 0;
    ZG_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    ZG_HIP(hipStreamCreateWithPriority(&g->pf_stream, hipStreamNonBlocking, least));
    ZG_HIP(hipEventCreateWithFlags(&g->pf_ev_main, hipEventDisableTiming));
    ZG_HIP(hipEventCreateWithFlags(&g->pf_ev_side, hipEventDisableTiming));
    g->pf_on = true;
    return ZG_OK;
}

void drop_prefetcher(zg_gpt* g) {
    if (g->pf_stream) {
        (void)hipStreamSynchronize(g->pf_stream);
        (void)hipStreamDestroy(g->pf_stream);
    }
    if (g->pf_ev_main) (void)hipEventDestroy(g->pf_ev_main);
    if (g->pf_ev_side) (void)hipEventDestroy(g->pf_ev_side);
    g->pf_stream = nullptr;
    g->pf_ev_main = g->pf_ev_side = nullptr;
    g->pf_on = false;
}

// Start the prefetcher for a run of decode steps ending at sequence length last_T: the control block is cleared on
// the side stream (behind the previous run's prefetcher), the decode stream waits for that, and the prefetcher
// starts once the decode stream reaches this point.  pf_stop() goes behind the last step.
int pf_start(zg_gpt* g, size_t last_T, hipStream_t s) {
    if (!g->pf_on || s == nullptr) return ZG_OK;
    if (g->pf_ran) {  // how did the previous one leave?  (the decode stream was synchronised by the caller)
        ZG_HIP(hipStreamSynchronize(g->pf_stream));
        unsigned why[8];
        ZG_HIP(hipMemcpy(why, g->pf_ctl->exit_reason, sizeof(why), hipMemcpyDeviceToHost));
        bool idle_exit = false;
        for (unsigned w : why) idle_exit |= w == 2u;
        g->pf_ran = false;
        if (idle_exit) {  // a strike, not a verdict: one slow host moment inside a generate loop produces the same exit
            g->pf_stalled = true;
            ++g->pf_strikes;
            g->pf_sit_out = 8;  // generate calls without it before the next try
        }
    }
    if (g->pf_stalled) {
        if (g->pf_strikes >= 3 || g->pf_sit_out-- > 0) return ZG_OK;
        g->pf_stalled = false;  // try again
    }
    ZG_HIP(hipMemsetAsync(g->pf_ctl, 0, sizeof(PfCtl), g->pf_stream));
    ZG_HIP(hipEventRecord(g->pf_ev_side, g->pf_stream));
    ZG_HIP(hipStreamWaitEvent(s, g->pf_ev_side, 0));
    ZG_HIP(hipEventRecord(g->pf_ev_main, s));
    ZG_HIP(hipStreamWaitEvent(g->pf_stream, g->pf_ev_main, 0));
    PfArgs a{};
    a.ctl = g->pf_ctl;
    a.jobs = g->pf_jobs;
    a.njobs = g->pf_njobs;
    // the measured optimum of the round-2 / round-3 sweeps (profiles/NOTEBOOK.md), constants since round 5
    a.lead = 2;    // launches ahead of the running one
    a.nsub = 12;   // prefetcher workgroups per XCD
    a.max_T = (int)last_T;
    a.idle_limit = (unsigned)env_int("ZGPT2_PF_IDLE", 100000);  // polls without progress (~0.1 s) before it gives up (0: the test of that exit)
    a.sleep = 1;
    a.cls_mask = 0x3e;  // every class but lm_head (its head start measured a net loss)
    a.line_shift = 7;   // one touch per 128-byte line
    a.cap_bytes = 0;
    g->pf_ran = true;
    return launch_prefetcher(a, g->pf_stream);
}

int pf_stop(zg_gpt* g, hipStream_t s) {
    if (!g->pf_on || s == nullptr) return ZG_OK;
    ZG_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&g->pf_ctl->progress), (int)PF_STOP, 1, s));
    return ZG_OK;
}

size_t prefill_min() { return 4; }  // shorter prompts go through the decode chain (measured: the whole-prompt pass pays from 4 tokens up)

// The decode graphs of a handle, per 64-position bucket of the sequence length, keyed by what the graph contains:
//   with_logits  lm_head behind the Blocks (a step that only feeds a prompt token has none)
//   multi        graph_steps consecutive steps (all with lm_head, all in one bucket) as ONE graph: the position lives in device
//                memory, so the same kernels simply repeat; saves the gap between graph launches in the generate loop
//   tail         what follows lm_head (StepTail, normalized; the option values are read on the device)
// The table has a slot for every combination of the fields, indexed by them as mixed-radix digits; the slots of combinations
// that cannot occur (multi or a tail without lm_head, penalties or edits in front of a greedy pick) simply stay null.
struct StepKey {
    bool with_logits, multi;
    StepTail tail;
};
constexpr size_t kStepShapes = 2 * 2 * kSamplerModes * 2 * 2 * 2 * 2;  // the radices of step_index
size_t step_index(StepKey k) {
    return ((((((size_t)k.with_logits * 2 + k.multi) * kSamplerModes + k.tail.sampler) * 2 + k.tail.pen) * 2 + k.tail.lp) * 2 + k.tail.stop) * 2 + k.tail.edit;
}

size_t bucket_of(size_t seq_len) { return (seq_len + 63) / 64 - 1; }

void drop_graphs(zg_gpt* g) {
    for (auto& e : g->graphs)
        if (e) {
            (void)hipGraphExecDestroy(e);
            e = nullptr;
        }
}

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

// The graph of (step shape k, bucket b) for stream s (the stream of g->graph_stream: capture_all), captured on first use.
int graph_exec(zg_gpt* g, StepKey k, size_t b, hipStream_t s, hipGraphExec_t* out) {
    hipGraphExec_t& e = g->graphs[step_index(k) * g->n_buckets + b];
    if (!e) {
        const int t_hi = bucket_t_hi(g, (b + 1) * 64);  // any length of the bucket: only its upper bound is baked in
        const size_t n_steps = k.multi ? g->graph_steps : 1;
        StepOpts o;
        o.tail = k.tail;
        ZG_TRY(capture_graph(s, &e, [&] {
            int st = ZG_OK;
            for (size_t i = 0; i < n_steps && st == ZG_OK; ++i) st = enqueue_step(g, k.with_logits, t_hi, s, o);
            return st;
        }));
    }
    *out = e;
    return ZG_OK;
}

// The single-step and (where the handle has them) multi-step graphs of a tail, buckets b0 .. b1
int capture_tail(zg_gpt* g, StepTail tail, size_t b0, size_t b1, hipStream_t s) {
    hipGraphExec_t e;
    for (size_t b = b0; b <= b1 && b < g->n_buckets; ++b) {
        ZG_TRY(graph_exec(g, {true, false, tail}, b, s, &e));
        if (g->graph_steps > 1) ZG_TRY(graph_exec(g, {true, true, tail}, b, s, &e));
    }
    return ZG_OK;
}

// The tails whose graphs zg_gpt_create captures besides the default one, by the handle's flags: each *_GENERATE flag names the
// samplers it is for, ZG_GPT_LOGPROBS_GENERATE the twins with the log-probability stage of the default tail and of those, and
// ZG_GPT_STOP_GENERATE the twins with the stop stage of all of these
std::vector<StepTail> tails_of_flags(unsigned flags) {
    std::vector<StepTail> t;
    if (flags & ZG_GPT_SAMPLED_GENERATE) t.push_back({PLAIN, false, false});
    if (flags & ZG_GPT_TRUNCATED_GENERATE)
        for (SamplerMode m : {ONE_FILTER, TWO_FILTERS}) t.push_back({m, false, false});
    if (flags & ZG_GPT_PENALIZED_GENERATE)
        for (SamplerMode m : {PLAIN, ONE_FILTER, TWO_FILTERS}) t.push_back({m, true, false});
    if (flags & ZG_GPT_EDITED_GENERATE) {  // min-p alone, and the edit stage in front of every sampler form (unpenalised)
        t.push_back({MINP_ONLY, false, false});
        for (SamplerMode m : {PLAIN, ONE_FILTER, TWO_FILTERS, MINP_ONLY}) t.push_back({m, false, false, false, true});
    }
    if (flags & ZG_GPT_LOGPROBS_GENERATE) {
        const size_t n = t.size();
        t.push_back({GREEDY, false, true});
        for (size_t i = 0; i < n; ++i) t.push_back({t[i].sampler, t[i].pen, true, false, t[i].edit});
    }
    if (flags & ZG_GPT_STOP_GENERATE) {  // the stop twins of the default tail and of everything above
        const size_t n = t.size();
        t.push_back({GREEDY, false, false, true});
        for (size_t i = 0; i < n; ++i) t.push_back({t[i].sampler, t[i].pen, t[i].lp, true, t[i].edit});
    }
    return t;
}

// All decode graphs of a handle for stream s.  Called from zg_gpt_create — the State.init moment (main.zig:46-64) — so that
// no forward allocates; a later zg_set_stream re-captures them on the first call that sees the new stream.  A generation whose
// tail create did not capture adds that tail's graphs when it begins (gen_begin).
int capture_all(zg_gpt* g, hipStream_t s) {
    if ((g->flags & ZG_GPT_NO_GRAPH) || s == nullptr) return ZG_OK;
    if (g->graph_stream != s) {
        drop_graphs(g);
        g->graph_stream = s;
    }
    hipGraphExec_t e;
    for (size_t b = 0; b < g->n_buckets; ++b) ZG_TRY(graph_exec(g, {false, false, StepTail{}}, b, s, &e));
    ZG_TRY(capture_tail(g, StepTail{}, 0, g->n_buckets - 1, s));
    for (const StepTail& t : tails_of_flags(g->flags)) ZG_TRY(capture_tail(g, t, 0, g->n_buckets - 1, s));
    return ZG_OK;
}

// Run one decode step at sequence length seq_len: replay the graph of its bucket, or launch eagerly when graphs
// are disabled / the stream cannot be captured.
int run_step(zg_gpt* g, bool with_logits, size_t seq_len, hipStream_t s, StepTail tail = StepTail{}) {
    ZG_TRY(ensure_ln_folded(g, s));
    tail = normalized(tail, with_logits);
    if ((g->flags & ZG_GPT_NO_GRAPH) || s == nullptr) {
        StepOpts o;
        o.tail = tail;
        return enqueue_step(g, with_logits, bucket_t_hi(g, seq_len), s, o);
    }
    if (g->graph_stream != s) ZG_TRY(capture_all(g, s));  // the caller switched streams after zg_gpt_create
    hipGraphExec_t e;
    ZG_TRY(graph_exec(g, {with_logits, false, tail}, bucket_of(seq_len), s, &e));
    ZG_HIP(hipGraphLaunch(e, s));
    return ZG_OK;
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
        const size_t cap = c.stage_cap / 4;
        ZG_REQUIRE(cap > 0, ZG_ERR_STAGING, "no staging arena");
        for (size_t o = 0; o < n; o += cap) {
            const size_t m = (n - o < cap) ? (n - o) : cap;
            ZG_HIP(hipMemcpyAsync(c.stage, src + o, m * 4, hipMemcpyHostToDevice, s));
            ZG_TRY(launch_f32_to_bf16(reinterpret_cast<const float*>(c.stage), reinterpret_cast<bf16_t*>(dst) + o, m, s));
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
    const size_t rows = n / K, cap_rows = c.stage_cap / (4 * K);
    ZG_REQUIRE(cap_rows > 0, ZG_ERR_STAGING, "no staging arena for a %zu-float row", K);
    const hipMemcpyKind kind = is_device_ptr(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    for (size_t r = 0; r < rows; r += cap_rows) {
        const size_t m = rows - r < cap_rows ? rows - r : cap_rows;
        ZG_HIP(hipMemcpyAsync(c.stage, src + r * K, m * K * 4, kind, s));
        ZG_TRY(launch_f32_to_b24(reinterpret_cast<const float*>(c.stage), m, (int)K, reinterpret_cast<char*>(dst) + r * 3 * K, s));
        ZG_HIP(hipStreamSynchronize(s));
    }
    if (planes) {
        ZG_TRY(launch_b24_split3(dst, rows, (int)K, planes, s));
        ZG_HIP(hipStreamSynchronize(s));
    }
    return ZG_OK;
}

// The control block of the steps enqueued next, through its pinned mirror (n_partials is always the lm_head grid).
int stage_ctrl(zg_gpt* g, size_t step, size_t seq_len, int mode, hipStream_t s) {
    g->h_ctrl->step = (int)step;
    g->h_ctrl->seq_len = (int)seq_len;
    g->h_ctrl->mode = mode;
    g->h_ctrl->n_partials = g->lm_grid;
    ZG_HIP(hipMemcpyAsync(g->ctrl, g->h_ctrl, sizeof(StepCtrl), hipMemcpyHostToDevice, s));
    return ZG_OK;
}

// n floats from device memory to a caller's pointer, which may be host or device.
int copy_out_f32(float* dst, const float* src, size_t n, hipStream_t s) {
    ZG_HIP(hipMemcpyAsync(dst, src, n * sizeof(float), is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
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
    if (g->h_lp) (void)hipHostFree(g->h_lp);
    if (g->h_stop) (void)hipHostFree(g->h_stop);
    if (g->h_edit) (void)hipHostFree(g->h_edit);
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
    // The decode modes, each decided from the plans (gemv_plan) of the launches enqueue_step would make with the mode on.
    const zg_layer& y = g->layers[0];
    const int off = decode_paths_off();
    g->lm_grid = gemv_plan(lm_head_args(g), g->wt).grid;
    // the widest input of a Block (mlp c_proj: 4 E floats per sequence) must fit the batched kernels' LDS
    ZG_REQUIRE(gemv_plan(mlp_proj_args(g, 0, 0, StepModes{}), g->wt).supported, ZG_ERR_UNSUPPORTED,
               "batch %zu with n_embed %zu: %zu input rows of 4*n_embed floats do not fit the LDS (use a smaller batch)", batch, c.n_embed, batch);
    if (g->wt == WT_BF16 && batch >= 2 && !(off & kOffPlanes) && c.n_embed % 32 == 0) {
        const StepModes cand{true, false, false};  // activation planes between the kernels
        const GemvPlan lin[4] = {gemv_plan(c_attn_args(g, y, 0, cand), g->wt), gemv_plan(c_proj_args(g, y, 0, cand), g->wt),
                                 gemv_plan(c_fc_args(g, y, 0, cand), g->wt), gemv_plan(mlp_proj_args(g, 0, 0, cand), g->wt)};
        auto every_linear = [&](bool GemvPlan::*f) { return lin[0].*f && lin[1].*f && lin[2].*f && lin[3].*f; };
        g->pl_on = every_linear(&GemvPlan::can_take_planes);  // all plane-fed Linears on the matrix-core path?
        // LayerNorm statistics by tile: every producer and consumer of x must be the four-wave kernel (the statistics' only
        // part in a plan is the bound on n_embed / 16 asked here)
        g->st_on = g->pl_on && !(off & kOffTileStats) && c.n_embed % 16 == 0 && c.n_embed / 16 <= 128 && every_linear(&GemvPlan::pl4_with_planes);
    }
    g->tags_on = g->pl_on && !(off & kOffTags);
    g->spin_limit = (unsigned)env_int("ZGPT2_TAG_SPIN_LIMIT", 1 << 20);
    g->tail_off = (unsigned)off & kStepPathsAtCreate;
    // one sequence on the fp32 cache: ln_1 + c_attn and the attention as one launch where c_attn runs on the LayerNorm-folding
    // kernel (ZGPT2_DECODE_PATHS_OFF kOffFusedAttn: two launches)
    if (batch == 1 && !(off & kOffFusedAttn) && c.n_layer <= 127) {
        const GemvArgs ca = c_attn_args(g, y, 0, modes_of(g));
        g->fused_on = attn_qkv_ok(ca, gemv_plan(ca, g->wt), attn_args(g, y, (int)c.context_size));
    }
    ZG_REQUIRE(g->lm_grid <= 4096, ZG_ERR_UNSUPPORTED, "lm_head grid %d exceeds the argmax partial buffer", g->lm_grid);
    // (the control mirror and, 256 bytes behind it, the fault word of the tagged hand-overs: pinned, written by the kernels)
    e = hipHostMalloc(reinterpret_cast<void**>(&g->h_ctrl), sizeof(StepCtrl) + 512, hipHostMallocDefault);
    // (h_ints, and behind it the staging of the penalties' prior / history: the same shape)
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&g->h_ints), 2 * (batch * c.context_size + batch) * sizeof(int), hipHostMallocDefault);
    // (the mirror of the log-probability record: a fetch copies its columns through it)
    if (e == hipSuccess)
        e = hipHostMalloc(reinterpret_cast<void**>(&g->h_lp), batch * c.context_size * (1 + 2 * ZG_LOGPROBS_TOP_MAX) * sizeof(float), hipHostMallocDefault);
    // (the stop stage's block: a few hundred bytes, always there)
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&g->h_stop), sizeof(*g->h_stop), hipHostMallocDefault);
    // (the edit stage's mirror: the bias table and the keep bitmap)
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&g->h_edit), edit_block_bytes(c.vocab_size), hipHostMallocDefault);
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc(control mirrors)", __FILE__, __LINE__);
    g->edit_build.assign(edit_block_bytes(c.vocab_size), 0);
    memset(g->h_stop, 0, sizeof(*g->h_stop));
    static_assert(sizeof(StepCtrl) + sizeof(SampleParams) <= 256, "the fault word sits 256 bytes behind the control mirror");
    g->h_samp = reinterpret_cast<SampleParams*>(reinterpret_cast<char*>(g->h_ctrl) + 128);  // (same pinned block)
    g->fault = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(g->h_ctrl) + 256);
    *g->fault = 0;
    g->h_pen = reinterpret_cast<PenParams*>(reinterpret_cast<char*>(g->h_ctrl) + 384);  // (behind zg_gpt_sample's uniforms at 320)
    g->h_prior = g->h_ints + batch * c.context_size + batch;
    g->h_lp_top = reinterpret_cast<int*>(reinterpret_cast<char*>(g->h_ctrl) + 416);  // (behind h_pen)
    ZG_REQUIRE(!(g->flags & ZG_GPT_PENALIZED_GENERATE) || c.context_size <= (size_t)kPenMaxHistory, ZG_ERR_UNSUPPORTED,
               "ZG_GPT_PENALIZED_GENERATE: context_size %zu beyond the %d tokens the penalty kernel's LDS table holds", c.context_size, kPenMaxHistory);
    {   // decode steps per graph in the generate loop: a graph launch costs ~7 us of idle queue (124M: 224.8 us per token
        // with 1 step per graph, 220.4 with 2 / 4, 218.3 with 8, 219.5 with 16)
        const int k = env_int("ZGPT2_GRAPH_STEPS", 8);
        g->graph_steps = (k == 2 || k == 4 || k == 8 || k == 16 || k == 32 || k == 64) ? (size_t)k : 1;
    }
    g->n_buckets = (c.context_size + 63) / 64;
    g->graphs.assign(kStepShapes * g->n_buckets, nullptr);
    // every decode graph is captured and instantiated here, not on the first forward that needs it
    ZG_TRY(setup_prefetcher(g));
    ZG_TRY(capture_all(g, gs(g)));
    if (parent) {
        ++parent->n_children;
        g->counted = true;
    }
    return ZG_OK;
}

}  // namespace

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

// A new sequence starts (position 1 of the token-at-a-time loop, a whole-prompt pass, a generation): the caches are cleared.  The
// decode attention loads the rows of its whole 64-position bucket and gives the ones at or behind the sequence length a
// probability of exactly 0 — which silences any finite leftover of an earlier sequence, but 0 x NaN is NaN: once a sequence had
// overflowed (or a checkpoint held a NaN) every later sequence on the handle came out NaN as well, repaired weights or not
// (tools/fuzz_errors_gpt.py).  124M, one sequence: 75 MB, ~20 us per generation of 217 ms.
// from_row > 0 (a whole-prompt pass writes rows 0 .. from_row - 1 itself): only the rows behind it, strip by strip — eight
// 1023-token prompts would otherwise pay a 600 MB memset (0.12 ms of a 5.4 ms pass) for one stale row per head.
// keep_head (a continuation: rows below from_row are the session): never the memset of the whole region.
static int clear_kv(zg_gpt* g, hipStream_t s, size_t from_row = 0, bool keep_head = false) {
    if (g->kv_region_bytes == 0 || g->arena == nullptr) return ZG_OK;
    const size_t C = g->cfg.context_size, E = g->cfg.n_embed, B = g->batch, L = g->cfg.n_layer;
    if (keep_head && from_row >= C) return ZG_OK;
    if (!keep_head && (from_row == 0 || from_row * 2 < C)) {
        ZG_HIP(hipMemsetAsync(g->layers[0].k_cache, 0, g->kv_region_bytes, s));
        return ZG_OK;
    }
    const size_t elems = B * C * E, kvb = kv_elem_bytes(g);
    const size_t stride = L > 1 ? (size_t)(reinterpret_cast<char*>(g->layers[1].k_cache) - reinterpret_cast<char*>(g->layers[0].k_cache)) / 2
                                : (size_t)(reinterpret_cast<char*>(g->layers[0].v_cache) - reinterpret_cast<char*>(g->layers[0].k_cache));
    ZG_REQUIRE(stride >= elems * kvb && reinterpret_cast<char*>(g->layers[0].v_cache) - reinterpret_cast<char*>(g->layers[0].k_cache) == (ptrdiff_t)stride,
               ZG_ERR_UNSUPPORTED, "kv clear: cache stride");
    const int strips = (int)(B * g->cfg.n_heads);
    ZG_TRY(launch_kv_clear_tail(g->layers[0].k_cache, (int)(2 * L), stride, 0, g->kv_mode == 0 ? 256 : 128, strips, (int)C, (int)from_row, s));
    if (g->kv_mode == 2) ZG_TRY(launch_kv_clear_tail(g->layers[0].k_cache, (int)(2 * L), stride, elems * 2, 64, strips, (int)C, (int)from_row, s));
    return ZG_OK;
}

// The cache policy of a whole-prompt pass over rows past .. end - 1.  past == 0, a new sequence: everything behind the pass is
// cleared (clear_kv).  A continuation: the rows behind it are cleared if anything was written there since they were last clean (a
// rollback, or zg_gpt_forward calls out of order) — the decode attention reads its whole 64-position bucket, and what a
// discarded row holds (a NaN, say) must not come back.  Rows below past are never touched.
static int clear_for_pass(zg_gpt* g, hipStream_t s, size_t past, size_t end) {
    if (past == 0) ZG_TRY(clear_kv(g, s, end));
    else if (g->kv_dirty_hi > end) ZG_TRY(clear_kv(g, s, end, true));
    g->kv_dirty_hi = end;
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

// GPT.forward enqueued on the handle's stream, nothing drained (zg_gpt_forward drains; zg_gpt_sample puts its sampler behind it first)
// taps (zg_debug_gpt_step_taps): the same step launched eagerly, with copies of what each launch class wrote behind it
static int forward_enqueue(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, int compute_logits, float* logits_out, size_t logits_len,
                           StepTaps* taps = nullptr) {
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
    if (taps) {
        StepOpts o;
        o.taps = taps;
        ZG_TRY(enqueue_step(g, compute_logits != 0, bucket_t_hi(g, seq_len), s, o));
    } else
        ZG_TRY(run_step(g, compute_logits != 0, seq_len, s));
    if (logits_out) ZG_TRY(copy_out_f32(logits_out, g->logits, g->batch * V, s));
    return ZG_OK;
}

int zg_gpt_forward(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, int compute_logits,
                   float* logits_out, size_t logits_len) {
    ZG_TRY(forward_enqueue(g, seq_len, tokens, n_tokens, compute_logits, logits_out, logits_len));
    // h_ints / h_ctrl are reused by the next call: drain before returning.
    ZG_HIP(hipStreamSynchronize(gs(g)));
    return check_fault(g);
}

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
        const int v[ZG_TAP_INFO_INTS] = {g->pl_on, g->st_on, g->tags_on, g->fused_on, g->max_splits, g->lm_grid, bucket_t_hi(g, seq_len), g->kv_mode, g->wt};
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

// How many alternatives a log-probability record may be asked for: the one check of every entry point that takes a top_n
static int check_top_n(size_t top_n, size_t vocab, const char* who) {
    ZG_REQUIRE(top_n <= (size_t)ZG_LOGPROBS_TOP_MAX && top_n <= vocab, ZG_ERR_ARG, "%s: top_n %zu outside 0..%zu", who, top_n,
               std::min((size_t)ZG_LOGPROBS_TOP_MAX, vocab));
    return ZG_OK;
}

// top_n of the record the call in flight writes, through its pinned word into the arena: from here on a fetch finds that record
static int stage_top_n(zg_gpt* g, size_t top_n, hipStream_t s) {
    g->lp_valid = true;
    g->lp_top_n = top_n;
    *g->h_lp_top = (int)top_n;
    ZG_HIP(hipMemcpyAsync(g->lp_top, g->h_lp_top, sizeof(int), hipMemcpyHostToDevice, s));
    return ZG_OK;
}

// `rows` records [ZG_LOGPROBS_TOP_MAX] of ids and values (host) into the packed [rows][top_n] arrays (host) a caller receives
static void unpack_top(const int* ids, const float* vals, size_t rows, size_t top_n, size_t* ids_out, float* vals_out) {
    for (size_t i = 0; i < rows; ++i)
        for (size_t j = 0; j < top_n; ++j) {
            ids_out[i * top_n + j] = (size_t)ids[i * ZG_LOGPROBS_TOP_MAX + j];
            vals_out[i * top_n + j] = vals[i * ZG_LOGPROBS_TOP_MAX + j];
        }
}

// The whole-prompt pass: n tokens of every sequence go to positions past_len .. past_len + n - 1 behind the cached
// ones — the prompt loop of generate (main.zig:331-334) at an offset — and, on request, ln_f + lm_head of each sequence's last new
// position run through the decode kernels.  Everything is checked before the handle or its staging is touched.
// sc (zg_gpt_score): behind the pass, the scoring stage over all of its rows.
struct ScoreCall {
    size_t top_n;
    float* logits_out;  // [batch][n][vocab], host or device, or null
    size_t logits_len;
};

// The scoring stage of a pass of n new positions per sequence behind `past` cached ones, whose residual stream of every row is
// in pf_x: ln_f of all rows once (pf_a is free: the pass is over), then block by block of kScoreRows rows the lm_head on the
// matrix cores into sc_logits, the two statistics launches, and on request the block's logits to the caller.
// taps (zg_debug_gpt_pass_taps): class 7 — the ln_f planes, then per block (the table's layer field) each GEMM's plan and the block's rows of sc_logits.
static int enqueue_score(zg_gpt* g, size_t past, size_t n, float* logits_out, hipStream_t s, StepTaps* taps = nullptr) {
    const size_t E = g->cfg.n_embed, V = g->cfg.vocab_size, C = g->cfg.context_size, V64 = g->sc_v64, head = V / 64 * 64, M = g->batch * n;
    const int iE = (int)E, ld = (int)V64;
    const int np = (g->flags & ZG_GPT_PREFILL_2PLANE) ? 2 : kSplit;
    ZG_TRY(ensure_score_weights(g, s));
    ZG_TRY(launch_ln_split(g->pf_x, (int)M, iE, g->ln_f_g, g->ln_f_b, 1e-5f, g->pf_a, s));
    PrefillGemmPlan plan{};
    PrefillGemmPlan* const plan_out = taps ? &plan : nullptr;
    auto tap_plan = [&](size_t block) {
        if (!taps) return (int)ZG_OK;
        int v[ZG_PREFILL_PLAN_INTS];
        prefill_plan_ints(plan, v);
        return tap_words(taps, 7, block, ZG_TAP_PLAN, v, ZG_PREFILL_PLAN_INTS);
    };
    if (taps) ZG_TRY(tap_put(taps, 7, 0, ZG_TAP_A, ZG_TAP_BF16, 0, g->pf_a, 1, M * kSplit * E * 2, M * kSplit * E * 2, s));
    for (size_t r0 = 0; r0 < M; r0 += kScoreRows) {
        const int rows = (int)std::min(kScoreRows, M - r0);
        const bf16_t* A = g->pf_a + r0 * kSplit * E;
        if (g->wt != WT_BF16) {  // the planes hold zero rows up to V64: one launch
            ZG_TRY(launch_prefill_gemm(A, g->sc_planes, nullptr, g->sc_logits, rows, ld, iE, ld, PF_F32, g->sc_gemm_ws, g->sc_gemm_ws_floats, nullptr, s, nullptr,
                                       kWeightPlanes, nullptr, plan_out));
            ZG_TRY(tap_plan(r0 / kScoreRows));
        } else {  // the whole 64-row groups of wte where they lie, then the strip: no row behind V - 1 of wte is read
            if (head) {
                ZG_TRY(launch_prefill_gemm(A, reinterpret_cast<const bf16_t*>(g->wte), nullptr, g->sc_logits, rows, (int)head, iE, ld, PF_F32, g->pf_ws,
                                           g->pf_ws_floats, nullptr, s, nullptr, np, nullptr, plan_out));
                ZG_TRY(tap_plan(r0 / kScoreRows));
            }
            if (g->sc_tail) {
                ZG_TRY(launch_prefill_gemm(A, g->sc_tail, nullptr, g->sc_logits + head, rows, 64, iE, ld, PF_F32, g->pf_ws, g->pf_ws_floats, nullptr, s, nullptr, np,
                                           nullptr, plan_out));
                ZG_TRY(tap_plan(r0 / kScoreRows));
            }
        }
        if (taps) ZG_TRY(tap_put(taps, 7, r0 / kScoreRows, ZG_TAP_LOGITS, ZG_TAP_F32, 0, g->sc_logits, 1, (size_t)rows * V64 * 4, (size_t)rows * V64 * 4, s));
        const ScoreTargets tg{g->prompt, (int)C, (int)n, (int)past, (int)r0};
        ZG_TRY(launch_score(g->sc_logits, rows, (int)V, ld, g->lp_top, g->sc_ws, tg, g->lp_rec, s));
        if (logits_out)
            ZG_HIP(hipMemcpy2DAsync(logits_out + r0 * V, V * 4, g->sc_logits, V64 * 4, V * 4, (size_t)rows,
                                    is_device_ptr(logits_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    }
    return ZG_OK;
}

static int pass_impl(zg_gpt* g, size_t past_len, const size_t* tokens, size_t stride, size_t n, int compute_logits, float* logits_out, size_t logits_len,
                     const char* who, const ScoreCall* sc = nullptr, StepTaps* taps = nullptr) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && tokens, ZG_ERR_ARG, "%s: null argument", who);
    ZG_REQUIRE(g->pf_x != nullptr, ZG_ERR_UNSUPPORTED, "%s: the handle was created with ZG_GPT_NO_PREFILL", who);
    const size_t C = g->cfg.context_size, V = g->cfg.vocab_size, B = g->batch, E = g->cfg.n_embed;
    if (sc) {
        ZG_REQUIRE(g->sc_logits != nullptr, ZG_ERR_UNSUPPORTED, "%s: the handle was created without ZG_GPT_SCORE", who);
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
        ZG_HIP(hipMemcpy2DAsync(g->x, E * 4, g->pf_x + (n - 1) * E, n * E * 4, E * 4, B, hipMemcpyDeviceToDevice, s));
        ZG_TRY(stage_ctrl(g, end - 1, end, 1, s));
        ZG_TRY(enqueue_lm_head(g, s));
        if (logits_out) ZG_TRY(copy_out_f32(logits_out, g->logits, B * V, s));
    }
    if (sc) {  // a log-probability generation with this top_n: the record continues behind it (generate_from) and leaves through the same fetch
        ZG_TRY(stage_top_n(g, sc->top_n, s));
        // column past_len: its predicting row is not part of the pass (NaN: every byte 0xff)
        ZG_HIP(hipMemset2DAsync(g->lp_rec.logprob + past_len, C * sizeof(float), 0xff, sizeof(float), B, s));
        ZG_TRY(enqueue_score(g, past_len, n, sc->logits_out, s, taps));
    }
    ZG_HIP(hipStreamSynchronize(s));
    return check_fault(g);
}

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

// zg_gpt_prefill / zg_gpt_extend / zg_gpt_score with every launch of the pass tapped (tests; include/zgpt2.h).  arena_out == nullptr:
// nothing runs; an upper bound of what a call needs is reported.  Allocates its device arena per call.
int zg_debug_gpt_pass_taps(zg_gpt* g, size_t past_len, const size_t* tokens, size_t token_stride, size_t n_tokens, int compute_logits, int score, size_t top_n,
                           float* logits_out, size_t logits_len, void* arena_out, size_t arena_bytes, size_t* arena_used, zg_tap_entry* table_out,
                           size_t table_len, size_t* n_entries, int* info, size_t n_info) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && tokens && arena_used && n_entries, ZG_ERR_ARG, "debug_gpt_pass_taps: null argument");
    ZG_REQUIRE(g->pf_x != nullptr, ZG_ERR_UNSUPPORTED, "debug_gpt_pass_taps: the handle was created with ZG_GPT_NO_PREFILL");
    const size_t C = g->cfg.context_size, E = g->cfg.n_embed, L = g->cfg.n_layer, B = g->batch;
    ZG_REQUIRE(n_tokens >= 1 && past_len + n_tokens <= C, ZG_ERR_SHAPE, "debug_gpt_pass_taps: %zu tokens behind %zu positions (context %zu)", n_tokens, past_len, C);
    ZG_REQUIRE(!score || g->sc_logits != nullptr, ZG_ERR_UNSUPPORTED, "debug_gpt_pass_taps: the handle was created without ZG_GPT_SCORE");
    // an upper bound of the pass's taps: per layer two cache taps of K and V (at most 4 bytes an element, and the B24 byte plane
    // within that), x twice, pf_a four times, qkv, pf_h, three plans and the geometry; class 0 and 1 once; the score stage
    const size_t M = B * n_tokens, T = std::min(C, past_len + n_tokens + kPassTapRowsBehind), blocks = (M + kScoreRows - 1) / kScoreRows;
    const size_t per_layer = 4 * B * E * T * 4 + 2 * M * E * 4 + 4 * M * kSplit * E * 2 + M * 3 * E * 4 + M * kSplit * 4 * E * 2;
    const size_t entries = 2 + L * 24 + (score ? 1 + 3 * blocks : 0);
    const size_t cap = L * per_layer + M * E * 4 + M * kSplit * E * 2 + (score ? M * kSplit * E * 2 + M * g->sc_v64 * 4 : 0) + 256 * (entries + 1);
    *arena_used = cap;
    *n_entries = entries;
    if (info && n_info >= ZG_PASS_INFO_INTS) {
        const bool f32w = g->wt != WT_BF16;
        const int v[ZG_PASS_INFO_INTS] = {f32w ? kSplit : (g->flags & ZG_GPT_PREFILL_2PLANE) ? 2 : kSplit, g->kv_mode, g->wt,
                                          (int)std::min(g->pf_ws_floats, (size_t)INT_MAX), !f32w && g->sk_flags != nullptr, (int)g->sc_v64, (int)kScoreRows};
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

int zg_gpt_cached_len(zg_gpt* g, size_t* len_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && len_out, ZG_ERR_ARG, "gpt_cached_len: null argument");
    *len_out = g->cached_len;
    return ZG_OK;
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

static inline bool penalties_off(const zg_logit_penalties& p) { return p.repetition == 1.0f && p.presence == 0.0f && p.frequency == 0.0f; }

// ---- Logit edits (include/zgpt2.h zg_logit_edits).  A checked set asks a call for the edit stage (any of the three
// lists: build_edits' stage_on — the set built in the handle's edit_build goes to the device and the edit launch runs) and / or for
// the sampler's min-p threshold
static inline bool edits_off(const zg_logit_edits& e) { return e.n_bias == 0 && e.n_allowed == 0 && e.n_banned == 0 && e.min_p == 0.0f; }

// temp x log(min_p) in double, rounded once: what the sampler adds to the row maximum (min_p 0: -inf, nothing is cut)
static float min_p_offset(float temp, float min_p) { return min_p == 0.0f ? -INFINITY : (float)((double)temp * log((double)min_p)); }

// The refusals of a set of edits over `vocab` logits (include/zgpt2.h), and — where any list is given — the set as the kernel
// reads it, built into `block` (edit_block_bytes(vocab) bytes of plain host memory): the bias pairs sorted by id, then the keep
// bitmap.  Nothing else is touched.
static int build_edits(const zg_logit_edits* e, size_t vocab, const char* who, char* block, bool* stage_on) {
    ZG_REQUIRE(e != nullptr, ZG_ERR_ARG, "%s: edits is null", who);
    ZG_REQUIRE(e->min_p >= 0.0f && e->min_p < 1.0f, ZG_ERR_ARG, "%s: min_p %f outside [0, 1)", who, e->min_p);  // (a NaN fails it)
    ZG_REQUIRE(e->n_bias <= (size_t)ZG_EDIT_MAX_BIAS, ZG_ERR_ARG, "%s: %zu biases above %d", who, e->n_bias, ZG_EDIT_MAX_BIAS);
    ZG_REQUIRE((e->n_bias == 0 || (e->bias_ids && e->bias_values)) && (e->n_allowed == 0 || e->allowed_ids) && (e->n_banned == 0 || e->banned_ids), ZG_ERR_ARG,
               "%s: a null array with a non-zero count", who);
    for (size_t i = 0; i < e->n_bias; ++i) ZG_REQUIRE(e->bias_ids[i] < vocab, ZG_ERR_SHAPE, "%s: bias id %zu >= vocab %zu", who, e->bias_ids[i], vocab);
    for (size_t i = 0; i < e->n_allowed; ++i) ZG_REQUIRE(e->allowed_ids[i] < vocab, ZG_ERR_SHAPE, "%s: allowed id %zu >= vocab %zu", who, e->allowed_ids[i], vocab);
    for (size_t i = 0; i < e->n_banned; ++i) ZG_REQUIRE(e->banned_ids[i] < vocab, ZG_ERR_SHAPE, "%s: banned id %zu >= vocab %zu", who, e->banned_ids[i], vocab);
    std::pair<int, float> pairs[ZG_EDIT_MAX_BIAS];
    for (size_t i = 0; i < e->n_bias; ++i) {
        ZG_REQUIRE(std::isfinite(e->bias_values[i]), ZG_ERR_ARG, "%s: bias %f on token %zu", who, e->bias_values[i], e->bias_ids[i]);
        pairs[i] = {(int)e->bias_ids[i], e->bias_values[i]};
    }
    std::sort(pairs, pairs + e->n_bias, [](const std::pair<int, float>& a, const std::pair<int, float>& b) { return a.first < b.first; });
    for (size_t i = 1; i < e->n_bias; ++i) ZG_REQUIRE(pairs[i].first != pairs[i - 1].first, ZG_ERR_ARG, "%s: token %d is biased twice", who, pairs[i].first);
    *stage_on = e->n_bias != 0 || e->n_allowed != 0 || e->n_banned != 0;
    if (!*stage_on) return ZG_OK;
    EditTable* tab = reinterpret_cast<EditTable*>(block);
    unsigned* keep = reinterpret_cast<unsigned*>(block + sizeof(EditTable));
    const size_t words = (vocab + 31) / 32;
    memset(tab, 0, sizeof(EditTable));
    tab->n_bias = (int)e->n_bias;
    for (size_t i = 0; i < e->n_bias; ++i) {
        tab->ids[i] = pairs[i].first;
        tab->vals[i] = pairs[i].second;
    }
    memset(keep, e->n_allowed ? 0x00 : 0xff, words * 4);
    for (size_t i = 0; i < e->n_allowed; ++i) keep[e->allowed_ids[i] >> 5] |= 1u << (e->allowed_ids[i] & 31);
    for (size_t i = 0; i < e->n_banned; ++i) keep[e->banned_ids[i] >> 5] &= ~(1u << (e->banned_ids[i] & 31));
    if (vocab & 31) keep[words - 1] &= (1u << (vocab & 31)) - 1u;  // (bits behind the vocabulary: never read, not counted)
    size_t kept = 0;
    for (size_t w = 0; w < words; ++w) kept += (size_t)__builtin_popcount(keep[w]);
    // (both lists are the host's: a row of -inf alone never reaches a kernel)
    ZG_REQUIRE(kept >= 1, ZG_ERR_ARG, "%s: the allow and ban lists leave no token", who);
    return ZG_OK;
}

// The set built in edit_build through its pinned mirror into the arena.  PRECONDITION: nothing in flight reads the mirror (every
// edited call drains, or begins by draining).
static int stage_edits(zg_gpt* g, hipStream_t s) {
    const size_t bytes = g->edit_build.size();
    memcpy(g->h_edit, g->edit_build.data(), bytes);
    ZG_HIP(hipMemcpyAsync(g->edit_tab, g->h_edit, bytes, hipMemcpyHostToDevice, s));
    return ZG_OK;
}

int zg_debug_min_p_offset(float temp, float min_p, float* d_out) {
    ZG_REQUIRE(d_out != nullptr && temp > 0.0f && min_p >= 0.0f && min_p < 1.0f, ZG_ERR_ARG, "debug_min_p_offset: temp %f, min_p %f", temp, min_p);
    *d_out = min_p_offset(temp, min_p);
    return ZG_OK;
}

int zg_gpt_hidden(zg_gpt* g, float* x_out, size_t len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && x_out && len >= g->batch * g->cfg.n_embed, ZG_ERR_ARG, "gpt_hidden: bad argument");
    hipStream_t s = gs(g);
    ZG_TRY(copy_out_f32(x_out, g->x, g->batch * g->cfg.n_embed, s));
    ZG_HIP(hipStreamSynchronize(s));
    return check_fault(g);
}

// The options of a sampler call over `vocab` logits into *p, the host image of SampleParams (the caller uploads it); returns the
// sampler they need: the plain one with both filters and min-p off, the threshold-aware tail alone for min-p alone
static SamplerMode fill_sample_params(SampleParams* p, size_t vocab, const zg_sample_options& o, uint64_t seed, float min_p) {
    const bool k_on = o.top_k >= 1 && o.top_k < vocab, p_on = o.top_p < 1.0f;
    p->inv_temp = 1.0f / o.temp;
    p->top_k = k_on ? (unsigned)o.top_k : 0u;
    p->seed = seed;
    p->top_p = p_on ? o.top_p : 1.0f;
    p->min_p_off = min_p_offset(o.temp, min_p);
    return k_on && p_on ? TWO_FILTERS : (k_on || p_on) ? ONE_FILTER : min_p != 0.0f ? MINP_ONLY : PLAIN;
}

static int check_penalties(const zg_logit_penalties* p, const char* who) {
    ZG_REQUIRE(p != nullptr, ZG_ERR_ARG, "%s: penalties is null", who);
    ZG_REQUIRE(p->repetition > 0.0f, ZG_ERR_ARG, "%s: repetition penalty %f (must be > 0)", who, p->repetition);  // (a NaN fails it)
    ZG_REQUIRE(std::isfinite(p->presence) && std::isfinite(p->frequency), ZG_ERR_ARG, "%s: presence %f / frequency %f penalty", who, p->presence,
               p->frequency);
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

// The penalties of the call and its token lists (checked) through their pinned mirrors into the arena.  PRECONDITION: nothing in
// flight reads the mirrors (every penalised call drains, or begins by draining).
static int stage_penalties(zg_gpt* g, const zg_logit_penalties& p, size_t past, const size_t* tokens, size_t stride, const size_t* lens, hipStream_t s) {
    const size_t C = g->cfg.context_size, B = g->batch;
    *g->h_pen = PenParams{p.repetition, p.presence, p.frequency, (int)past};
    int* h_len = g->h_prior + B * C;
    for (size_t b = 0; b < B; ++b) {
        h_len[b] = tokens ? (int)lens[b] : 0;
        for (size_t i = 0; tokens && i < lens[b]; ++i) g->h_prior[b * C + i] = (int)tokens[b * stride + i];
    }
    ZG_HIP(hipMemcpyAsync(g->pen, g->h_pen, sizeof(PenParams), hipMemcpyHostToDevice, s));
    if (tokens) ZG_HIP(hipMemcpyAsync(g->prior, g->h_prior, B * C * sizeof(int), hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(g->prior_len, h_len, B * sizeof(int), hipMemcpyHostToDevice, s));
    return ZG_OK;
}

static int check_sample_options(const zg_sample_options* o, const char* who) {
    ZG_REQUIRE(o != nullptr, ZG_ERR_ARG, "%s: options is null", who);
    ZG_REQUIRE(o->temp > 0.0f, ZG_ERR_ARG, "%s: temperature %f", who, o->temp);
    ZG_REQUIRE(o->top_p > 0.0f && o->top_p <= 1.0f, ZG_ERR_ARG, "%s: top_p %f outside (0, 1]", who, o->top_p);  // (a NaN fails both)
    return ZG_OK;
}

// GPT.sample (main.zig:198-207) behind one forward step: the checked body of the per-token family — zg_gpt_sample_edit's, under the
// name of the entry point that calls it; each entry point keeps in front what it is stricter about.  penalties null: none, the
// history is not read; an entry point without edits passes kNoEdits.  Everything the chain reads is staged first: the chain only launches.
static const zg_logit_edits kNoEdits{};
static int sample_impl(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, const zg_sample_options* opt, const zg_logit_penalties* pen,
                       const size_t* history, size_t history_stride, const size_t* history_lens, const zg_logit_edits* edits, const float* uniforms,
                       uint64_t seed, size_t* tokens_out, float* probs_out, size_t probs_len, const char* who) {
    ZG_TRY(require_init());
    ZG_TRY(check_sample_options(opt, who));
    ZG_REQUIRE(g != nullptr, ZG_ERR_ARG, "%s: null handle", who);
    if (pen) {
        ZG_TRY(check_penalties(pen, who));
        ZG_TRY(check_pen_handle(g, who));
        ZG_TRY(check_history(g, history, history_stride, history_lens, 0, who));
    }
    bool edit_on = false;
    ZG_TRY(build_edits(edits, g->cfg.vocab_size, who, g->edit_build.data(), &edit_on));
    const bool pen_on = pen && !penalties_off(*pen);
    if (pen_on || edit_on) ZG_HIP(hipStreamSynchronize(gs(g)));  // (an enqueued generation may still be reading the pinned mirrors; idle otherwise)
    ZG_REQUIRE(tokens && tokens_out, ZG_ERR_ARG, "gpt_sample: bad argument");
    const size_t V = g->cfg.vocab_size, B = g->batch;
    ZG_REQUIRE(!probs_out || probs_len >= B * V, ZG_ERR_SHAPE, "gpt_sample: probs_out needs %zu elements", B * V);
    for (size_t b = 0; uniforms && b < B; ++b)  // (checked before anything is enqueued)
        ZG_REQUIRE(uniforms[b] >= 0.0f && uniforms[b] < 1.0f, ZG_ERR_ARG, "gpt_sample: uniform %f outside [0,1)", uniforms[b]);
    ZG_TRY(forward_enqueue(g, seq_len, tokens, n_tokens, 1, nullptr, 0));  // main.zig:199 (not drained: the sampler goes behind it)
    hipStream_t s = gs(g);
    if (pen_on) ZG_TRY(stage_penalties(g, *pen, 0, history, history_stride, history_lens, s));
    if (edit_on) ZG_TRY(stage_edits(g, s));
    // (pinned, 320 bytes into the control block: h_ints[0 .. B) is still being read by the forward's token upload)
    float* h_u = reinterpret_cast<float*>(reinterpret_cast<char*>(g->h_ctrl) + 320);
    // (no uniforms: the counter PRNG the device loop's sampler draws from, zg_common.h)
    for (size_t b = 0; b < B; ++b) h_u[b] = uniforms ? uniforms[b] : counter_uniform(seed, seq_len, b);
    SamplerChain c = handle_chain(g, false);
    float* d_u = g->q;  // scratch: q is dead after the forward
    ZG_HIP(hipMemcpyAsync(d_u, h_u, B * sizeof(float), hipMemcpyHostToDevice, s));
    // (h_samp: nothing in flight reads it, forward_enqueue's callers drain; the plain sampler takes its temperature by value)
    const SamplerMode mode = fill_sample_params(g->h_samp, V, *opt, seed, edits->min_p);
    if (threshold_sampler(mode)) ZG_HIP(hipMemcpyAsync(g->samp, g->h_samp, sizeof(SampleParams), hipMemcpyHostToDevice, s));
    c.u = d_u, c.temp = opt->temp, c.write_probs = probs_out != nullptr, c.pick = g->cur_token;
    ZG_TRY(emit_sampler_chain(c, StepTail{mode, pen_on, false, false, edit_on}, s));  // main.zig:200-206
    ZG_HIP(hipMemcpyAsync(g->h_ints + B, g->cur_token, B * sizeof(int), hipMemcpyDeviceToHost, s));
    if (probs_out) ZG_TRY(copy_out_f32(probs_out, g->logits, B * V, s));
    ZG_HIP(hipStreamSynchronize(s));
    ZG_TRY(check_fault(g));
    for (size_t b = 0; b < B; ++b) tokens_out[b] = (size_t)g->h_ints[B + b];
    return ZG_OK;
}

int zg_gpt_sample(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, float temp, const float* uniforms,
                  uint64_t seed, size_t* tokens_out, float* probs_out, size_t probs_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(temp > 0.0f, ZG_ERR_ARG, "gpt_sample: bad argument");
    const zg_sample_options plain{temp, 0, 1.0f};
    return sample_impl(g, seq_len, tokens, n_tokens, &plain, nullptr, nullptr, 0, nullptr, &kNoEdits, uniforms, seed, tokens_out, probs_out, probs_len,
                       "gpt_sample");
}

// zg_gpt_sample behind top-k / nucleus truncation (filters off: exactly zg_gpt_sample's launches)
int zg_gpt_sample_ex(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, const zg_sample_options* opt, const float* uniforms,
                     uint64_t seed, size_t* tokens_out, float* probs_out, size_t probs_len) {
    return sample_impl(g, seq_len, tokens, n_tokens, opt, nullptr, nullptr, 0, nullptr, &kNoEdits, uniforms, seed, tokens_out, probs_out, probs_len,
                       "gpt_sample_ex");
}

// ... with the penalty stage in front, on the caller's history: here the penalties are required
int zg_gpt_sample_pen(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, const zg_sample_options* opt, const zg_logit_penalties* pen,
                      const size_t* history, size_t history_stride, const size_t* history_lens, const float* uniforms, uint64_t seed, size_t* tokens_out,
                      float* probs_out, size_t probs_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(pen != nullptr, ZG_ERR_ARG, "gpt_sample_pen: penalties is null");
    return sample_impl(g, seq_len, tokens, n_tokens, opt, pen, history, history_stride, history_lens, &kNoEdits, uniforms, seed, tokens_out, probs_out,
                       probs_len, "gpt_sample_pen");
}

// ... and with the edit stage behind the penalties and min-p in the sampler: here the edits are required
int zg_gpt_sample_edit(zg_gpt* g, size_t seq_len, const size_t* tokens, size_t n_tokens, const zg_sample_options* opt, const zg_logit_penalties* pen,
                       const size_t* history, size_t history_stride, const size_t* history_lens, const zg_logit_edits* edits, const float* uniforms,
                       uint64_t seed, size_t* tokens_out, float* probs_out, size_t probs_len) {
    return sample_impl(g, seq_len, tokens, n_tokens, opt, pen, history, history_stride, history_lens, edits, uniforms, seed, tokens_out, probs_out,
                       probs_len, "gpt_sample_edit");
}

// A generation in three parts, so that several handles' generations can be fed to their streams side by side
// (zg_gpt_generate_enqueue_many): gen_begin — prompts, cache clearing, the whole-prompt pass, the prefetcher's start;
// gen_pump — ONE graph launch (graph_steps decode steps) or one single step, false when nothing is left; gen_end — the
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
    SamplerMode mode;       // GREEDY (opt unused), or PLAIN: draw with opt — gen_begin raises it to the filters opt switches on
    zg_sample_options opt;
    uint64_t seed;
    // penalties (a sampler only; pen_on false: none, the request is what it was without them) and the caller's prior of every row of
    // the ONE handle such a request goes to: [rows][prior_stride], prior_lens[rows] tokens each, or null
    bool pen_on = false;
    zg_logit_penalties pen{1.0f, 0.0f, 0.0f};
    const size_t* prior = nullptr;
    size_t prior_stride = 0;
    const size_t* prior_lens = nullptr;
    // the log-probability stage behind every pick with top_n alternatives; lp_on false: the request is what it was
    bool lp_on = false;
    size_t top_n = 0;
    // stop conditions, checked (check_stop); stop_on false: the request is what it was
    bool stop_on = false;
    zg_stop_conditions stop{};
    // logit edits, checked, the set built in the ONE handle's edit_build: edit_on — the
    // edit stage runs; min_p — the sampler's threshold (0: off).  Both off: the request is what it was
    bool edit_on = false;
    float min_p = 0.0f;
    GenRequest(const size_t* prompts, size_t stride, const size_t* lens, size_t n_steps, const zg_sample_options* opt_or_null = nullptr, uint64_t seed = 0,
               size_t past = 0)
        : prompts(prompts), stride(stride), lens(lens), n_steps(n_steps), past(past), mode(opt_or_null ? PLAIN : GREEDY),
          opt(opt_or_null ? *opt_or_null : zg_sample_options{1.0f, 0, 1.0f}), seed(seed) {}
};

// Steps the host may be ahead of the stop stage's progress word before it feeds the next piece, where the caller names none:
// the smallest value whose rate is inside the run-to-run spread of an unpaced loop (tools/bench_stop.py)
constexpr size_t kStopLookahead = 16;

// The refusals of a set of stop conditions (include/zgpt2.h), vocab standing for the first token that cannot occur
static int check_stop(const zg_stop_conditions* c, size_t vocab, const char* who) {
    ZG_REQUIRE(c != nullptr, ZG_ERR_ARG, "%s: stop conditions are null", who);
    ZG_REQUIRE(c->n_ids <= ZG_STOP_MAX_IDS && c->n_seqs <= ZG_STOP_MAX_SEQS, ZG_ERR_ARG, "%s: %zu stop tokens / %zu stop sequences above %d / %d", who,
               c->n_ids, c->n_seqs, ZG_STOP_MAX_IDS, ZG_STOP_MAX_SEQS);
    ZG_REQUIRE((c->n_ids == 0 || c->ids) && (c->n_seqs == 0 || (c->seqs && c->seq_lens)), ZG_ERR_ARG, "%s: a null array with a non-zero count", who);
    for (size_t k = 0; k < c->n_seqs; ++k)
        ZG_REQUIRE(c->seq_lens[k] >= 1 && c->seq_lens[k] <= ZG_STOP_MAX_SEQ_LEN && c->seq_lens[k] <= c->seq_stride, ZG_ERR_ARG,
                   "%s: stop sequence %zu has length %zu (1 .. %d, stride %zu)", who, k, c->seq_lens[k], ZG_STOP_MAX_SEQ_LEN, c->seq_stride);
    for (size_t j = 0; j < c->n_ids; ++j) ZG_REQUIRE(c->ids[j] < vocab, ZG_ERR_SHAPE, "%s: stop token %zu >= vocab %zu", who, c->ids[j], vocab);
    for (size_t k = 0; k < c->n_seqs; ++k)
        for (size_t i = 0; i < c->seq_lens[k]; ++i)
            ZG_REQUIRE(c->seqs[k * c->seq_stride + i] < vocab, ZG_ERR_SHAPE, "%s: token %zu of stop sequence %zu >= vocab %zu", who,
                       c->seqs[k * c->seq_stride + i], k, vocab);
    return ZG_OK;
}

// Checked conditions as the kernel reads them
static void fill_stop(StopConds* d, const zg_stop_conditions& c) {
    memset(d, 0, sizeof(*d));
    d->n_ids = (int)c.n_ids;
    d->n_seqs = (int)c.n_seqs;
    for (size_t j = 0; j < c.n_ids; ++j) d->ids[j] = (int)c.ids[j];
    for (size_t k = 0; k < c.n_seqs; ++k) {
        d->seq_len[k] = (int)c.seq_lens[k];
        for (size_t i = 0; i < c.seq_lens[k]; ++i) d->seq[k][i] = (int)c.seqs[k * c.seq_stride + i];
    }
}

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
    if (pen_on) {  // (a row's history, prior and recorded, never exceeds the context: the kernel's table is sized by it)
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
    if (g->pf_x != nullptr && min_prompt >= prefill_min())
        first = min_prompt < n_steps ? min_prompt : n_steps;
    const bool edit_on = r.edit_on && r.mode != GREEDY;
    g->gen_tail = StepTail{r.mode, pen_on, r.lp_on, r.stop_on, edit_on};  // (normalized: pen_on / edit_on only with a sampler, and the steps it is for have lm_head)
    g->stop_valid = false;
    g->gen_stop = r.stop_on;
    if (r.stop_on) {  // the conditions of this call; no row has finished; the stage has seen nothing (the stream is drained: the words are the host's)
        fill_stop(&g->h_stop->conds, r.stop);
        ZG_HIP(hipMemcpyAsync(g->stop, &g->h_stop->conds, sizeof(StopConds), hipMemcpyHostToDevice, s));
        ZG_HIP(hipMemsetAsync(g->stop_fin, 0xff, kStopMaxRows * 4, s));
        ZG_HIP(hipMemsetAsync(g->stop_reason, 0xff, kStopMaxRows * 4, s));
        g->h_stop->host.progress = g->h_stop->host.done_col = 0u;
        g->gen_lookahead = r.stop.lookahead ? std::min(r.stop.lookahead, C) : kStopLookahead;  // (beyond the context: never waits)
    }
    if (r.mode != GREEDY) {
        g->gen_tail.sampler = fill_sample_params(g->h_samp, V, r.opt, r.seed, r.min_p);
        ZG_HIP(hipMemcpyAsync(g->samp, g->h_samp, sizeof(SampleParams), hipMemcpyHostToDevice, s));
    }
    if (pen_on) ZG_TRY(stage_penalties(g, r.pen, past, r.prior, r.prior_stride, r.prior_lens, s));
    if (edit_on) ZG_TRY(stage_edits(g, s));
    g->lp_valid = false;
    if (r.lp_on) {
        ZG_TRY(stage_top_n(g, r.top_n, s));
        // the new columns no step with lm_head reaches (the whole-prompt pass, steps that only feed a prompt token) record prompt
        // tokens: NaN (every byte 0xff); the stage itself writes the NaN of a longer row's prompt columns
        const size_t fed = std::min(min_prompt, n_steps);
        ZG_HIP(hipMemset2DAsync(g->lp_rec.logprob + past, C * sizeof(float), 0xff, fed * sizeof(float), B, s));
    }
    ZG_HIP(hipMemcpyAsync(g->prompt, g->h_ints, B * C * sizeof(int), hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(g->prompt_len, g->h_ints + B * C, B * sizeof(int), hipMemcpyHostToDevice, s));
    ZG_TRY(stage_ctrl(g, past + first, past + first, r.mode != GREEDY ? 2 : 0, s));
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
        if (g->graph_stream != s) ZG_TRY(capture_all(g, s));
        if (!(g->gen_tail == StepTail{}) && min_prompt < n_steps)
            ZG_TRY(capture_tail(g, g->gen_tail, bucket_of(past + std::max(first, min_prompt) + 1), bucket_of(past + n_steps), s));
    }
    ZG_TRY(note_steps(g, n_steps, s));
    ZG_TRY(pf_start(g, past + n_steps, s));
    g->gen_pos = past + first;  // absolute, as gen_n and gen_min_prompt: gen_pump's steps, buckets and graph alignment follow the position
    g->gen_n = past + n_steps;
    g->gen_min_prompt = past + min_prompt;
    g->gen_since_sync = 0;
    g->gen_open = true;
    return ZG_OK;
}

// A stop generation before each piece it feeds: *ended when every row has finished — nothing more is fed —, else
// wait while the host is more than gen_lookahead steps ahead of the stop stage.  The stage counts steps with lm_head only, so the
// steps below gen_min_prompt (the default tail) are not paced over.  progress is read BEFORE done_col and the kernel stores them
// the other way round: a done_col still 0 then means that the finishing step had not announced itself when progress was read, which
// is what bounds `end`.  The wait is bounded by the device's state, not by a count: whenever the word has stood still over 16 polls
// the stream is asked, and a drained or failed stream ends the wait — a faulted device ends the call instead of spinning the host.
static int stop_pace(zg_gpt* g, hipStream_t s, bool* ended) {
    StopHost* const h = &g->h_stop->host;
    *ended = false;
    unsigned seen = ~0u;  // progress at the last look at the stream
    for (unsigned polls = 0;; ++polls) {
        const unsigned p = __atomic_load_n(&h->progress, __ATOMIC_ACQUIRE);
        const unsigned d = __atomic_load_n(&h->done_col, __ATOMIC_ACQUIRE);
        if (d != 0u) {
            *ended = true;
            return ZG_OK;
        }
        if (g->gen_pos <= std::max((size_t)p, g->gen_min_prompt) + g->gen_lookahead) return ZG_OK;
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
    const size_t C = g->cfg.context_size, n_steps = g->gen_n, st = g->gen_pos;
    *more = false;
    if (st >= n_steps) return ZG_OK;
    if (g->gen_stop && st > g->gen_min_prompt) {  // (behind the first step with lm_head: nothing can have finished before)
        bool ended = false;
        ZG_TRY(stop_pace(g, s, &ended));
        if (ended) return ZG_OK;
    }
    const size_t K = ((g->flags & ZG_GPT_NO_GRAPH) || s == nullptr) ? 1 : g->graph_steps;
    // ZGPT2_SYNC_EVERY=n (profiling only): drain the stream every n steps — rocprofv3's counter collection has crashed
    // on this stack when tens of thousands of dispatches were queued ahead of it
    static const int sync_every = env_int("ZGPT2_SYNC_EVERY", 0);
    if (sync_every > 0 && ++g->gen_since_sync >= (size_t)sync_every) {
        g->gen_since_sync = 0;
        (void)hipStreamSynchronize(s);
    }
    if (K > 1 && st >= g->gen_min_prompt && st % K == 0 && st + K <= n_steps && st + K <= C) {
        if (g->graph_stream != s) ZG_TRY(capture_all(g, s));
        hipGraphExec_t e;  // sequence lengths st + 1 .. st + K share a bucket (K divides 64); captured by gen_begin (first use: the backstop)
        ZG_TRY(graph_exec(g, {true, true, g->gen_tail}, bucket_of(st + 1), s, &e));
        ZG_HIP(hipGraphLaunch(e, s));
        g->gen_pos = st + K;
    } else {
        ZG_TRY(run_step(g, st >= g->gen_min_prompt, st + 1, s, g->gen_tail));
        g->gen_pos = st + 1;
    }
    *more = g->gen_pos < n_steps;
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
    g->gen_open = false;
    ZG_TRY(pf_stop(g, s));  // also after a failed launch: the prefetcher must not wait for steps that never come
    ZG_TRY(rs);
    ZG_TRY(launch_embed_step(embed_args(g, 1), s));  // record the pick of the last step
    if (g->gen_stop) {  // the column actually reached: the one place that corrects what gen_begin set up front
        g->gen_n = g->cached_len = g->kv_dirty_hi = g->stop_end = g->gen_pos;
        g->stop_valid = true;
    }
    g->steps_enqueued = g->gen_n;
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
static int generate_request(zg_gpt* const* handles, size_t n_handles, const zg_generate_request& q, const char* who) {
    ZG_TRY(require_init());
    zg_gpt* const g = handles[0];
    ZG_REQUIRE(g != nullptr, ZG_ERR_ARG, "%s: null argument", who);
    if (q.options) ZG_TRY(check_sample_options(q.options, who));
    ZG_REQUIRE(q.options || !q.penalties, ZG_ERR_ARG, "%s: penalties without sampler options (greedy picking with penalties is top_k = 1)", who);
    GenRequest r(q.prompts, q.prompt_stride, q.prompt_lens, q.n_steps, q.options, q.seed, q.past_len);
    if (q.logprobs) {
        r.lp_on = true;
        r.top_n = q.top_n;
    }
    if (q.penalties) {
        ZG_TRY(check_penalties(q.penalties, who));
        if (!penalties_off(*q.penalties)) {
            r.pen_on = true;
            r.pen = *q.penalties;
            r.prior = q.prior;
            r.prior_stride = q.prior_stride;
            r.prior_lens = q.prior_lens;
        } else {  // all off: the request stays what it was without them, but the lists are still the caller's to get right
            ZG_TRY(check_pen_handle(g, who));
            ZG_TRY(check_history(g, q.prior, q.prior_stride, q.prior_lens, 0, who));
        }
    }
    if (q.stop && (q.stop->n_ids || q.stop->n_seqs)) {
        ZG_REQUIRE(g->batch <= (size_t)kStopMaxRows, ZG_ERR_UNSUPPORTED, "%s: batch %zu above %d", who, g->batch, kStopMaxRows);
        ZG_TRY(check_stop(q.stop, g->cfg.vocab_size, who));
        r.stop_on = true;
        r.stop = *q.stop;
    }
    if (q.edits) {
        ZG_TRY(build_edits(q.edits, g->cfg.vocab_size, who, g->edit_build.data(), &r.edit_on));
        ZG_REQUIRE(q.options || edits_off(*q.edits), ZG_ERR_ARG, "%s: edits without sampler options (greedy picking with edits is top_k = 1)", who);
        r.min_p = q.edits->min_p;
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

int zg_gpt_generate_stop_result(zg_gpt* g, size_t* end_out, size_t* finish_cols_out, int* reasons_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && end_out && finish_cols_out && reasons_out, ZG_ERR_ARG, "generate_stop_result: null argument");
    ZG_REQUIRE(g->stop_valid, ZG_ERR_ARG, "generate_stop_result: the last generation had no stop conditions");
    hipStream_t s = gs(g);
    ZG_HIP(hipMemcpyAsync(g->h_stop->fin, g->stop_fin, g->batch * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipMemcpyAsync(g->h_stop->reason, g->stop_reason, g->batch * 4, hipMemcpyDeviceToHost, s));
    ZG_HIP(hipStreamSynchronize(s));
    ZG_TRY(check_fault(g));
    *end_out = g->stop_end;
    for (size_t b = 0; b < g->batch; ++b) {
        const int f = g->h_stop->fin[b];
        finish_cols_out[b] = f < 0 ? ZG_STOP_NONE : (size_t)f;
        reasons_out[b] = f < 0 ? -1 : g->h_stop->reason[b];
    }
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

int zg_gpt_generate_fetch_logprobs(zg_gpt* g, size_t first, size_t n, size_t top_n, float* logprobs_out, size_t logprobs_len, size_t* top_ids_out,
                                   float* top_logprobs_out, size_t top_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && logprobs_out, ZG_ERR_ARG, "generate_fetch_logprobs: null argument");
    const size_t C = g->cfg.context_size, B = g->batch, K = ZG_LOGPROBS_TOP_MAX;
    ZG_REQUIRE(g->lp_valid, ZG_ERR_ARG, "generate_fetch_logprobs: the last generation recorded no log-probabilities");
    ZG_REQUIRE(top_n <= g->lp_top_n, ZG_ERR_ARG, "generate_fetch_logprobs: top_n %zu above the %zu the generation recorded", top_n, g->lp_top_n);
    ZG_REQUIRE(top_n == 0 || (top_ids_out && top_logprobs_out), ZG_ERR_ARG, "generate_fetch_logprobs: top_n %zu without its outputs", top_n);
    ZG_REQUIRE(first <= C && n <= C - first && logprobs_len >= B * n && (top_n == 0 || top_len >= B * n * top_n), ZG_ERR_SHAPE,
               "generate_fetch_logprobs: positions %zu .. %zu of %zu, %zu and %zu elements", first, first + n, C, logprobs_len, top_len);
    if (n == 0) return ZG_OK;
    hipStream_t s = gs(g);
    float* h_lp = g->h_lp;
    int* h_ids = reinterpret_cast<int*>(g->h_lp + B * C);
    float* h_top = g->h_lp + B * C * (1 + K);
    // the columns asked for, packed [batch][n] and [batch][n][20]
    ZG_HIP(hipMemcpy2DAsync(h_lp, n * 4, g->lp_rec.logprob + first, C * 4, n * 4, B, hipMemcpyDeviceToHost, s));
    if (top_n) {
        ZG_HIP(hipMemcpy2DAsync(h_ids, n * K * 4, g->lp_rec.top_ids + first * K, C * K * 4, n * K * 4, B, hipMemcpyDeviceToHost, s));
        ZG_HIP(hipMemcpy2DAsync(h_top, n * K * 4, g->lp_rec.top_logprobs + first * K, C * K * 4, n * K * 4, B, hipMemcpyDeviceToHost, s));
    }
    ZG_HIP(hipStreamSynchronize(s));
    ZG_TRY(check_fault(g));
    memcpy(logprobs_out, h_lp, B * n * sizeof(float));
    unpack_top(h_ids, h_top, B * n, top_n, top_ids_out, top_logprobs_out);
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

// The sampler chain on the caller's rows (tests), a small kernel standing in for lm_head's row-maximum partials: the body of
// zg_debug_edit_rows, and with edits null — no edit stage, no min-p — of zg_debug_sample_rows.  Allocates its workspace per call.
static int debug_sample_rows(const float* logits, size_t batch, size_t vocab, const zg_sample_options* opt, const zg_logit_edits* edits, const float* uniforms,
                             float* edited_out, size_t* tokens_out, float* probs_out, float* thresholds_out, const char* who) {
    ZG_TRY(check_sample_options(opt, who));
    ZG_REQUIRE(logits && uniforms && tokens_out && batch >= 1 && batch <= 64 && vocab >= 1 && vocab <= (size_t)64 * 4096, ZG_ERR_ARG, "%s: bad argument", who);
    std::vector<char> block(edits ? edit_block_bytes(vocab) : 0);
    bool stage_on = false;
    if (edits) ZG_TRY(build_edits(edits, vocab, who, block.data(), &stage_on));
    const int B = (int)batch, V = (int)vocab, n_part = std::min(64, (V + 255) / 256);
    SampleParams hp{};
    const SamplerMode mode = fill_sample_params(&hp, vocab, *opt, 0, edits ? edits->min_p : 0.0f);
    hipStream_t s = ctx().stream;
    DevScratch ds;
    char *d_filt, *d_edit;
    SampleParams* d_par;
    float* d_u;
    SamplerChain c{};
    c.batch = B, c.vocab = V, c.n_part = n_part, c.temp = opt->temp, c.write_probs = probs_out != nullptr;
    ZG_TRY(ds.carve([&] {
        d_filt = ds.take<char>(filter_workspace_bytes(B));
        c.filt = filter_workspace(d_filt, B);
        c.logits = ds.take<float>(batch * vocab * 4);
        c.seg_ws = ds.take<float>(sample_workspace_floats(B) * 4);
        c.part_val = ds.take<float>((size_t)B * n_part * 4);
        c.part_idx = ds.take<int>((size_t)B * n_part * 4);
        c.params = d_par = ds.take<SampleParams>(sizeof(SampleParams));
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
    ZG_HIP(hipMemcpyAsync(d_par, &hp, sizeof(hp), hipMemcpyHostToDevice, s));
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
    return debug_sample_rows(logits, batch, vocab, opt, nullptr, uniforms, nullptr, tokens_out, probs_out, thresholds_out, "debug_sample_rows");
}

// ... with the edit stage in front of the sampler and min-p in it; here the edits are required.  Everything off: zg_debug_sample_rows.
int zg_debug_edit_rows(const float* logits, size_t batch, size_t vocab, const zg_sample_options* opt, const zg_logit_edits* edits, const float* uniforms,
                       float* edited_out, size_t* tokens_out, float* probs_out, float* thresholds_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(edits != nullptr, ZG_ERR_ARG, "debug_edit_rows: edits is null");
    return debug_sample_rows(logits, batch, vocab, opt, edits, uniforms, edited_out, tokens_out, probs_out, thresholds_out, "debug_edit_rows");
}

// The penalty kernels on the caller's rows (tests): the launches of the penalised step, in place on a copy.  Allocates per call.
int zg_debug_penalize_rows(const float* logits, size_t batch, size_t vocab, const zg_logit_penalties* pen, const size_t* history, size_t history_stride,
                           const size_t* history_lens, float* logits_out, unsigned* counts_out) {
    ZG_TRY(require_init());
    ZG_TRY(check_penalties(pen, "debug_penalize_rows"));
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
        c.pen = d_par = ds.take<PenParams>(sizeof(PenParams));
    }));
    std::vector<int> h_hist(batch * stride, 0), h_len(batch);
    for (size_t b = 0; b < batch; ++b) {
        h_len[b] = (int)history_lens[b];
        for (size_t i = 0; i < history_lens[b]; ++i) h_hist[b * stride + i] = (int)history[b * history_stride + i];
    }
    const PenParams hp{pen->repetition, pen->presence, pen->frequency, 0};
    ZG_HIP(hipMemcpyAsync(d_logits, logits, batch * vocab * 4, hipMemcpyDefault, s));
    ZG_HIP(hipMemsetAsync(d_counts, 0, batch * vocab * 4, s));
    ZG_HIP(hipMemcpyAsync(d_hist, h_hist.data(), batch * stride * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_len, h_len.data(), batch * 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d_par, &hp, sizeof(hp), hipMemcpyHostToDevice, s));
    c.hist.prior = d_hist;
    c.hist.prior_len = d_len;
    c.hist.prior_stride = (int)stride;
    c.hist.max_hist = (int)longest;
    ZG_TRY(emit_sampler_chain(c, StepTail{GREEDY, true}, s));
    // all penalties off: the call is the identity on the rows (the counts are still the history's)
    ZG_HIP(hipMemcpyAsync(logits_out, penalties_off(*pen) ? logits : d_logits, batch * vocab * 4, hipMemcpyDefault, s));
    if (counts_out) ZG_HIP(hipMemcpyAsync(counts_out, d_counts, batch * vocab * 4, hipMemcpyDefault, s));
    ZG_HIP(hipStreamSynchronize(s));
    return ZG_OK;
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

int zg_gpt_profile_step(zg_gpt* g, size_t seq_len, int iters, float* us_out, size_t n_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && us_out && n_out >= 8 && iters > 0, ZG_ERR_ARG, "profile_step: bad argument");
    ZG_REQUIRE(seq_len >= 1 && seq_len + (size_t)iters - 1 <= g->cfg.context_size, ZG_ERR_SHAPE,
               "profile_step: positions %zu..%zu outside the context", seq_len, seq_len + iters - 1);
    hipStream_t s = gs(g);
    ZG_HIP(hipStreamSynchronize(s));
    ZG_TRY(ensure_ln_folded(g, s));
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
        if ((g->tags_on || g->fused_on) && which != 0) st = launch_epoch_bump(g->epoch, s);
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
    if (set_sk_epoch) g->sk_epoch = sk_epoch;
    if (!g->tags_on && !g->fused_on) return ZG_OK;
    hipStream_t s = gs(g);
    ZG_TRY(note_steps(g, n_steps, s));
    return launch_epoch_add(g->epoch, (unsigned)n_steps, s);
}

int zg_debug_gpt_age_state(zg_gpt* g, unsigned long long* out, size_t n_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && out && n_out >= ZG_AGE_STATE_WORDS, ZG_ERR_ARG, "debug_gpt_age_state: need %d words", ZG_AGE_STATE_WORDS);
    ZG_HIP(hipStreamSynchronize(gs(g)));
    unsigned epoch = 0;
    ZG_HIP(hipMemcpy(&epoch, g->epoch, sizeof(unsigned), hipMemcpyDeviceToHost));
    out[0] = epoch;
    out[1] = g->epochs_since_clear;
    out[2] = g->steps_counted;
    out[3] = g->tag_clears;
    out[4] = g->sk_epoch;
    out[5] = g->sk_restarts;
    return ZG_OK;
}

int zg_debug_gpt_tag_census(zg_gpt* g, unsigned epoch24, unsigned sk_flag_value, size_t* counts, size_t n_counts) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && counts && n_counts >= 4 && epoch24 < (1u << 24), ZG_ERR_ARG, "debug_gpt_tag_census: need 4 counts and a 24-bit epoch");
    ZG_HIP(hipStreamSynchronize(gs(g)));
    const unsigned long long* const words[3] = {g->sk_tag, g->part_tag, g->qkv_tag};
    const size_t bytes[3] = {g->sk_tag_bytes, g->part_tag_bytes, g->qkv_tag_bytes};
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
    if (g->sk_flags != nullptr) {
        unsigned f[kSkFlagWords];
        ZG_HIP(hipMemcpy(f, g->sk_flags, sizeof(f), hipMemcpyDeviceToHost));
        for (const unsigned w : f) counts[3] += w == sk_flag_value;
    }
    return ZG_OK;
}

int zg_debug_prefetch_stats(zg_gpt* g, unsigned* out, size_t n_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(g && out && n_out >= 25, ZG_ERR_ARG, "prefetch_stats: need 25 words");
    memset(out, 0, n_out * sizeof(unsigned));
    out[0] = g->pf_on ? (g->pf_stalled ? 2u : 1u) : 0u;
    if (!g->pf_on) return ZG_OK;
    ZG_HIP(hipStreamSynchronize(gs(g)));
    ZG_HIP(hipStreamSynchronize(g->pf_stream));
    PfCtl h;
    ZG_HIP(hipMemcpy(&h, g->pf_ctl, sizeof(PfCtl), hipMemcpyDeviceToHost));
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
