// api_gpt_step.hip — model tier of the C ABI: what a decode step launches and which graph replays it.  The shape of a decode step
// exists once, as StepKey {with_logits, multi, StepTail}: what enqueue_step launches and which graph replays it (the sampler chain
// behind lm_head is emitted by emit_sampler_chain for every user: sampler_chain.hip).  What follows
// lm_head — which sampler, penalties or not, log-probabilities or not — travels as ONE value, StepTail, from the request to the
// launches: a generation holds one (zg_gpt::gen.tail), a step is told one (StepOpts::tail), a graph is keyed by one, and the graph
// table is indexed by its fields as mixed-radix digits (step_index).  ONE rule says which graphs exist when: create captures the
// default tail's and those of the tails its flags name (tails_of_flags), and a generation whose tail is another one captures that
// tail's graphs for the buckets it will touch when it begins (gen_begin), before its steps are counted and the prefetcher starts.
#include <vector>

#include "api_gpt.h"

using namespace zg;

namespace {  // this unit only

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
    a.progress = g->prefetch.on ? &g->prefetch.ctl->progress : nullptr;
    return a;
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

// The history the penalty stage of a handle reads: the prior buffer alone (zg_gpt_sample_pen: the caller's explicit history), or
// followed by the generate loop's own record from PenParams.past_len on
PenHistory pen_history(const zg_gpt* g, bool loop) {
    PenHistory h{};
    h.prior = g->pen.prior;
    h.prior_len = g->pen.prior_len;
    h.prior_stride = (int)g->cfg.context_size;
    if (loop) {
        h.rec = g->out_tokens;
        h.rec_stride = (int)g->cfg.context_size;
        h.ctrl = g->ctrl;
    }
    h.max_hist = (int)g->cfg.context_size;  // (the entry points hold prior + recorded tokens to the context)
    return h;
}

size_t step_index(StepKey k) {
    return (((((((((size_t)k.with_logits * 2 + k.multi) * kSamplerModes + k.tail.sampler) * 2 + k.tail.pen) * 2 + k.tail.lp) * 2 + k.tail.stop) * 2 + k.tail.edit) * 2 + k.tail.guide) * 2 + k.tail.ban) * 2 + k.tail.beam;
}

// The tails whose graphs zg_gpt_create captures besides the default one, by the handle's flags: each *_GENERATE flag names the
// samplers it is for, ZG_GPT_LOGPROBS_GENERATE the twins with the log-probability stage of the default tail and of those, and
// ZG_GPT_GUIDED_GENERATE the guided twins of the sampler tails, ZG_GPT_BANNED_GENERATE their banned twins, ZG_GPT_STOP_GENERATE the twins with the stop stage of all of these
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
    if (flags & ZG_GPT_GUIDED_GENERATE) {  // the guided twin of every sampler tail above (a greedy pick has none)
        const size_t n = t.size();
        for (size_t i = 0; i < n; ++i) t.push_back({t[i].sampler, t[i].pen, false, false, t[i].edit, true});
    }
    if (flags & ZG_GPT_BANNED_GENERATE) {  // the banned twin of every unguided sampler tail above (no greedy, no guided + banned twin)
        const size_t n = t.size();
        for (size_t i = 0; i < n; ++i)
            if (!t[i].guide) t.push_back({t[i].sampler, t[i].pen, false, false, t[i].edit, false, true});
    }
    if (flags & ZG_GPT_LOGPROBS_GENERATE) {
        const size_t n = t.size();
        t.push_back({GREEDY, false, true});
        for (size_t i = 0; i < n; ++i) t.push_back({t[i].sampler, t[i].pen, true, false, t[i].edit, t[i].guide, t[i].ban});
    }
    if (flags & ZG_GPT_STOP_GENERATE) {  // the stop twins of the default tail and of everything above
        const size_t n = t.size();
        t.push_back({GREEDY, false, false, true});
        for (size_t i = 0; i < n; ++i) t.push_back({t[i].sampler, t[i].pen, t[i].lp, true, t[i].edit, t[i].guide, t[i].ban});
    }
    if (flags & ZG_GPT_BEAM_GENERATE) t.push_back(normalized({GREEDY, false, true, false, false, false, false, true}, true));  // the one beam tail: it has no twins
    return t;
}

// The arguments of the decode launches of a Block and of lm_head, one builder per launch class: enqueue_step launches what they
// return, and decide_step_modes plans (gemv_plan) the very same arguments.  The decode modes they lay the arguments out for are
// passed in: the handle's own (zg_gpt::modes) for a step, a candidate while decide_step_modes decides them.

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
    a.progress = g->prefetch.on ? &g->prefetch.ctl->progress : nullptr;
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
            a.epoch = g->hand.epoch;
            a.sk_tag = g->hand.sk_tag;
            a.fault = g->hand.fault;
            a.spin_limit = g->hand.spin_limit;
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

}  // namespace

namespace zg {  // offered to the other units: api_gpt.h declares them

int bucket_t_hi(const zg_gpt* g, size_t seq_len) {
    const size_t hi = ((seq_len + 63) / 64) * 64;
    return (int)(hi < g->cfg.context_size ? hi : g->cfg.context_size);
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
    e.pl_out = g->modes.pl ? g->xp : nullptr;
    e.pl_g = g->layers[0].ln_1_g;
    e.epoch = (((g->modes.pl && g->modes.tags) || g->modes.fused) && finish_only != 1 && finish_only != 2) ? g->hand.epoch : nullptr;
    e.st_out = g->modes.st ? g->xst : nullptr;
    e.finish_only = finish_only;
    e.progress = g->prefetch.on ? &g->prefetch.ctl->progress : nullptr;
    e.sampled = g->samp.sampled;
    return e;
}

int prof_mark(StepProf* p, int cls, hipStream_t s) {
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

int enqueue_lm_head(zg_gpt* g, hipStream_t s, std::vector<PfJob>* rec) {
    const GemvArgs a = lm_head_args(g);
    const GemvPlan p = gemv_plan(a, g->wt);
    ZG_REQUIRE(p.grid == g->lm_grid, ZG_ERR_ARG, "lm_head grid changed");
    return emit_gemv(g, a, p, s, rec, 6);
}

// The chain of a handle: the loop's (draws by its control block into `sampled`, history = prior + its own record), or that of a
// per-token call, whose draw source and destination are the caller's to add
SamplerChain handle_chain(const zg_gpt* g, bool loop) {
    SamplerChain c{};
    c.logits = g->logits, c.batch = (int)g->batch, c.vocab = (int)g->cfg.vocab_size;
    c.part_val = g->part_val, c.part_idx = g->part_idx, c.n_part = g->lm_grid;
    c.pen = g->pen.params, c.hist = pen_history(g, loop);
    c.edit_tab = g->edit.tab, c.edit_keep = g->edit.keep;
    c.guide = GuideArgs{g->guide.next, g->guide.keep, g->guide.n_states, g->guide.state, g->guide.rec, (int)g->cfg.context_size, loop ? g->ctrl : nullptr,
                        g->prompt_len};
    c.ban = BanArgs{g->ban.rules, g->prompt_len, nullptr};
    c.params = g->samp.params, c.seg_ws = g->samp.ws, c.filt = g->samp.filt;
    if (loop) c.ctrl = g->ctrl, c.pick = g->samp.sampled;
    return c;
}

// The decode modes of a handle (zg_gpt_create, once the arena is carved), each decided from the plans (gemv_plan) of the launches
// enqueue_step would make with the mode on; with them lm_grid, tail_off and the spin limit of the tagged hand-overs.
int decide_step_modes(zg_gpt* g) {
    const zg_gpt_config& c = g->cfg;
    const size_t batch = g->batch;
    const zg_layer& y = g->layers[0];
    const int off = decode_paths_off();
    StepModes& m = g->modes;
    g->lm_grid = gemv_plan(lm_head_args(g), g->wt).grid;
    // the widest input of a Block (mlp c_proj: 4 E floats per sequence) must fit the batched kernels' LDS
    ZG_REQUIRE(gemv_plan(mlp_proj_args(g, 0, 0, StepModes{}), g->wt).supported, ZG_ERR_UNSUPPORTED,
               "batch %zu with n_embed %zu: %zu input rows of 4*n_embed floats do not fit the LDS (use a smaller batch)", batch, c.n_embed, batch);
    if (g->wt == WT_BF16 && batch >= 2 && !(off & kOffPlanes) && c.n_embed % 32 == 0) {
        const StepModes cand{true, false, false};  // activation planes between the kernels
        const GemvPlan lin[4] = {gemv_plan(c_attn_args(g, y, 0, cand), g->wt), gemv_plan(c_proj_args(g, y, 0, cand), g->wt),
                                 gemv_plan(c_fc_args(g, y, 0, cand), g->wt), gemv_plan(mlp_proj_args(g, 0, 0, cand), g->wt)};
        auto every_linear = [&](bool GemvPlan::*f) { return lin[0].*f && lin[1].*f && lin[2].*f && lin[3].*f; };
        m.pl = every_linear(&GemvPlan::can_take_planes);  // all plane-fed Linears on the matrix-core path?
        // LayerNorm statistics by tile: every producer and consumer of x must be the four-wave kernel (the statistics' only
        // part in a plan is the bound on n_embed / 16 asked here)
        m.st = m.pl && !(off & kOffTileStats) && c.n_embed % 16 == 0 && c.n_embed / 16 <= 128 && every_linear(&GemvPlan::pl4_with_planes);
    }
    m.tags = m.pl && !(off & kOffTags);
    g->hand.spin_limit = (unsigned)env_int("ZGPT2_TAG_SPIN_LIMIT", 1 << 20);
    g->tail_off = (unsigned)off & kStepPathsAtCreate;
    // one sequence on the fp32 cache: ln_1 + c_attn and the attention as one launch where c_attn runs on the LayerNorm-folding
    // kernel (ZGPT2_DECODE_PATHS_OFF kOffFusedAttn: two launches)
    if (batch == 1 && !(off & kOffFusedAttn) && c.n_layer <= 127) {
        const GemvArgs ca = c_attn_args(g, y, 0, m);
        m.fused = attn_qkv_ok(ca, gemv_plan(ca, g->wt), attn_args(g, y, (int)c.context_size));
    }
    ZG_REQUIRE(g->lm_grid <= 4096, ZG_ERR_UNSUPPORTED, "lm_head grid %d exceeds the argmax partial buffer", g->lm_grid);
    return ZG_OK;
}

// One decode step = GPT.forward (main.zig:178-195) for all sequences.
int enqueue_step(zg_gpt* g, bool with_logits, int t_hi, hipStream_t s, const StepOpts& o) {
    StepProf* const prof = o.prof;
    std::vector<PfJob>* const rec = o.rec;
    const int only = o.only;
    auto launch_id = [&](size_t l, int k) { return (unsigned)(o.salt >= 0 ? 1 + (2 * o.salt + k) % 254 : 2 * (int)l + 1 + k); };
    const StepModes& m = g->modes;
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
        const bool fused = g->modes.fused && !rec && 2 * l + 2 <= 255;
        ZG_TRY(tap_class(g, o.taps, -1, l, 0, s));
        if (fused && (only < 0 || only == 1)) {
            const GemvArgs a = c_attn_args(g, y, t_hi, m);
            AttnArgs at = attn_args(g, y, t_hi);
            at.launch_id = launch_id(l, 0);
            at.fault = g->hand.fault;
            at.spin_limit = g->hand.spin_limit;
            ZG_TRY(launch_attn_qkv(a, gemv_plan(a, g->wt), g->wt, at, g->hand.epoch, g->hand.qkv_tag, s));
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
            if (g->modes.pl) {
                a.pl_out = g->ap;
                a.merge_cnt = g->attn_cnt;
                if (g->modes.tags && 2 * l + 2 <= 255) {
                    a.epoch = g->hand.epoch;
                    a.launch_id = launch_id(l, 0);
                    a.part_tag = g->hand.part_tag;
                    a.fault = g->hand.fault;
                    a.spin_limit = g->hand.spin_limit;
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
        return launch_logprob(g->logits, (int)g->batch, (int)g->cfg.vocab_size, g->part_val, g->part_idx, g->lm_grid, g->lm_grid, g->lp.top, g->lp.ws,
                              tokens, g->ctrl, g->prompt_len, g->lp.rec, s);
    };
    // the stop stage, last: it learns the pick of its own step the way the log-probability stage does
    auto stop = [&](const int* picks) {
        StopArgs a{};
        a.conds = g->stop.conds;
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
        a.finish_col = g->stop.fin;
        a.reason = g->stop.reason;
        a.host = &g->stop.pinned->host;
        return launch_stop(a, s);
    };
    const StepTail tail = o.tail;
    if (!with_logits || only >= 0 || rec) return ZG_OK;
    const int* const picks = tail.sampler == GREEDY ? nullptr : g->samp.sampled;  // (the greedy graphs have no sampler node)
    ZG_TRY(emit_sampler_chain(handle_chain(g, true), tail, s));
    if (tail.lp) ZG_TRY(logprobs(picks));
    // beam search: the next beams from the lists the stage above has just recorded, into `sampled` (the next step's
    // embed kernel runs in mode 2), then every slot's cache becomes its parent's over the positions this step has filled
    if (tail.beam) {
        BeamArgs a{};
        a.st = g->beam.state;
        a.lenpow = g->beam.lenpow;
        a.n_lenpow = (int)g->cfg.context_size + 1;
        a.batch = (int)g->batch;
        a.vocab = (int)g->cfg.vocab_size;
        a.top_ids = g->lp.rec.top_ids;
        a.top_logprobs = g->lp.rec.top_logprobs;
        a.stride = (int)g->cfg.context_size;
        a.ctrl = g->ctrl;
        a.col = -1;
        a.sampled = g->samp.sampled;
        a.parent = g->beam.parent;
        a.score = g->beam.score;
        a.logprob = g->lp.rec.logprob;
        a.host = &g->stop.pinned->host;
        ZG_TRY(launch_beam(a, s));
        ZG_TRY(enqueue_kv_fork(g, t_hi, g->beam.state->src, &g->ctrl->seq_len, 0u, 0, s));
    }
    // the guide's advance: the state record of this column, then the transition of the pick (a guided tail has a sampler)
    if (tail.guide) ZG_TRY(launch_guide_advance(handle_chain(g, true).guide, picks, (int)g->batch, (int)g->cfg.vocab_size, s));
    if (tail.stop) ZG_TRY(stop(picks));
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
    if (g->prefetch.njobs > 255) return ZG_OK;  // the progress word counts launches in 8 bits (n_layer >= 51): no prefetcher, not an error
    std::vector<PfJob> jobs;
    StepOpts describe;
    describe.rec = &jobs;
    ZG_TRY(enqueue_step(g, true, (int)g->cfg.context_size, nullptr, describe));
    ZG_REQUIRE((int)jobs.size() == g->prefetch.njobs, ZG_ERR_ARG, "prefetcher: %zu launches per step", jobs.size());
    ZG_HIP(hipMemcpy(g->prefetch.jobs, jobs.data(), jobs.size() * sizeof(PfJob), hipMemcpyHostToDevice));
    int least = 0, greatest = 0;
    ZG_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    ZG_HIP(hipStreamCreateWithPriority(&g->prefetch.stream, hipStreamNonBlocking, least));
    ZG_HIP(hipEventCreateWithFlags(&g->prefetch.ev_main, hipEventDisableTiming));
    ZG_HIP(hipEventCreateWithFlags(&g->prefetch.ev_side, hipEventDisableTiming));
    g->prefetch.on = true;
    return ZG_OK;
}

void drop_prefetcher(zg_gpt* g) {
    if (g->prefetch.stream) {
        (void)hipStreamSynchronize(g->prefetch.stream);
        (void)hipStreamDestroy(g->prefetch.stream);
    }
    if (g->prefetch.ev_main) (void)hipEventDestroy(g->prefetch.ev_main);
    if (g->prefetch.ev_side) (void)hipEventDestroy(g->prefetch.ev_side);
    g->prefetch.stream = nullptr;
    g->prefetch.ev_main = g->prefetch.ev_side = nullptr;
    g->prefetch.on = false;
}

// Start the prefetcher for a run of decode steps ending at sequence length last_T: the control block is cleared on
// the side stream (behind the previous run's prefetcher), the decode stream waits for that, and the prefetcher
// starts once the decode stream reaches this point.  pf_stop() goes behind the last step.
int pf_start(zg_gpt* g, size_t last_T, hipStream_t s) {
    if (!g->prefetch.on || s == nullptr) return ZG_OK;
    if (g->prefetch.ran) {  // how did the previous one leave?  (the decode stream was synchronised by the caller)
        ZG_HIP(hipStreamSynchronize(g->prefetch.stream));
        unsigned why[8];
        ZG_HIP(hipMemcpy(why, g->prefetch.ctl->exit_reason, sizeof(why), hipMemcpyDeviceToHost));
        bool idle_exit = false;
        for (unsigned w : why) idle_exit |= w == 2u;
        g->prefetch.ran = false;
        if (idle_exit) {  // a strike, not a verdict: one slow host moment inside a generate loop produces the same exit
            g->prefetch.stalled = true;
            ++g->prefetch.strikes;
            g->prefetch.sit_out = 8;  // generate calls without it before the next try
        }
    }
    if (g->prefetch.stalled) {
        if (g->prefetch.strikes >= 3 || g->prefetch.sit_out-- > 0) return ZG_OK;
        g->prefetch.stalled = false;  // try again
    }
    ZG_HIP(hipMemsetAsync(g->prefetch.ctl, 0, sizeof(PfCtl), g->prefetch.stream));
    ZG_HIP(hipEventRecord(g->prefetch.ev_side, g->prefetch.stream));
    ZG_HIP(hipStreamWaitEvent(s, g->prefetch.ev_side, 0));
    ZG_HIP(hipEventRecord(g->prefetch.ev_main, s));
    ZG_HIP(hipStreamWaitEvent(g->prefetch.stream, g->prefetch.ev_main, 0));
    PfArgs a{};
    a.ctl = g->prefetch.ctl;
    a.jobs = g->prefetch.jobs;
    a.njobs = g->prefetch.njobs;
    // the measured optimum of the round-2 / round-3 sweeps (profiles/NOTEBOOK.md), constants since round 5
    a.lead = 2;    // launches ahead of the running one
    a.nsub = 12;   // prefetcher workgroups per XCD
    a.max_T = (int)last_T;
    a.idle_limit = (unsigned)env_int("ZGPT2_PF_IDLE", 100000);  // polls without progress (~0.1 s) before it gives up (0: the test of that exit)
    a.sleep = 1;
    a.cls_mask = 0x3e;  // every class but lm_head (its head start measured a net loss)
    a.line_shift = 7;   // one touch per 128-byte line
    a.cap_bytes = 0;
    g->prefetch.ran = true;
    return launch_prefetcher(a, g->prefetch.stream);
}

int pf_stop(zg_gpt* g, hipStream_t s) {
    if (!g->prefetch.on || s == nullptr) return ZG_OK;
    ZG_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&g->prefetch.ctl->progress), (int)PF_STOP, 1, s));
    return ZG_OK;
}

size_t bucket_of(size_t seq_len) { return (seq_len + 63) / 64 - 1; }

void drop_graphs(zg_gpt* g) {
    for (auto& e : g->graph.execs)
        if (e) {
            (void)hipGraphExecDestroy(e);
            e = nullptr;
        }
}

// The graph of (step shape k, bucket b) for stream s (the stream of g->graph.stream: capture_all), captured on first use.
int graph_exec(zg_gpt* g, StepKey k, size_t b, hipStream_t s, hipGraphExec_t* out) {
    hipGraphExec_t& e = g->graph.execs[step_index(k) * g->graph.n_buckets + b];
    if (!e) {
        const int t_hi = bucket_t_hi(g, (b + 1) * 64);  // any length of the bucket: only its upper bound is baked in
        const size_t n_steps = k.multi ? g->graph.steps : 1;
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
    for (size_t b = b0; b <= b1 && b < g->graph.n_buckets; ++b) {
        ZG_TRY(graph_exec(g, {true, false, tail}, b, s, &e));
        if (g->graph.steps > 1) ZG_TRY(graph_exec(g, {true, true, tail}, b, s, &e));
    }
    return ZG_OK;
}

// All decode graphs of a handle for stream s.  Called from zg_gpt_create — the State.init moment (main.zig:46-64) — so that
// no forward allocates; a later zg_set_stream re-captures them on the first call that sees the new stream.  A generation whose
// tail create did not capture adds that tail's graphs when it begins (gen_begin).
int capture_all(zg_gpt* g, hipStream_t s) {
    if ((g->flags & ZG_GPT_NO_GRAPH) || s == nullptr) return ZG_OK;
    if (g->graph.stream != s) {
        drop_graphs(g);
        g->graph.stream = s;
    }
    hipGraphExec_t e;
    for (size_t b = 0; b < g->graph.n_buckets; ++b) ZG_TRY(graph_exec(g, {false, false, StepTail{}}, b, s, &e));
    ZG_TRY(capture_tail(g, StepTail{}, 0, g->graph.n_buckets - 1, s));
    for (const StepTail& t : tails_of_flags(g->flags)) ZG_TRY(capture_tail(g, t, 0, g->graph.n_buckets - 1, s));
    return ZG_OK;
}

// Run one decode step at sequence length seq_len: replay the graph of its bucket, or launch eagerly when graphs
// are disabled / the stream cannot be captured.
int run_step(zg_gpt* g, bool with_logits, size_t seq_len, hipStream_t s, StepTail tail) {
    ZG_TRY(ensure_ln_folded(g, s));
    g->hidden.src = HID_X;
    tail = normalized(tail, with_logits);
    if ((g->flags & ZG_GPT_NO_GRAPH) || s == nullptr) {
        StepOpts o;
        o.tail = tail;
        return enqueue_step(g, with_logits, bucket_t_hi(g, seq_len), s, o);
    }
    if (g->graph.stream != s) ZG_TRY(capture_all(g, s));  // the caller switched streams after zg_gpt_create
    hipGraphExec_t e;
    ZG_TRY(graph_exec(g, {with_logits, false, tail}, bucket_of(seq_len), s, &e));
    ZG_HIP(hipGraphLaunch(e, s));
    return ZG_OK;
}

}  // namespace zg
