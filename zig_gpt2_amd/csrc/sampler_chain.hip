// sampler_chain.hip — the handle-free host side of the sampler: the sampler chain behind lm_head, emitted by emit_sampler_chain for
// every user, and the checks and fills of what a sampler call is given (options, penalties, edits, stop conditions, top_n, a guide).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "sampler_chain.h"

using namespace zg;

namespace {  // this unit only

// temp x log(min_p) in double, rounded once: what the sampler adds to the row maximum (min_p 0: -inf, nothing is cut)
static float min_p_offset(float temp, float min_p) { return min_p == 0.0f ? -INFINITY : (float)((double)temp * log((double)min_p)); }

}  // namespace

namespace zg {  // offered to the model tier: sampler_chain.h declares them

// the edit stage's block: the bias table, then the keep bitmap of `vocab` bits
size_t edit_block_bytes(size_t vocab) { return sizeof(EditTable) + (vocab + 31) / 32 * 4; }

// The launches of tail t behind lm_head, up to the pick: GPT.sample's tail (main.zig:200-206) behind the stages that rewrite the
// row.  Launches only — what they read is staged by the caller (enqueue_step runs under capture).  A GREEDY tail has no sampler
// launch: the partials are the pick.
int emit_sampler_chain(const SamplerChain& c, StepTail t, hipStream_t s) {
    // the penalties act on the raw logits, the edits on the row the penalties leave (HF's processor order); the row-maximum
    // partials every sampler starts from are rebuilt only behind the LAST stage that rewrites the row — the edit launch does it itself
    // and the guide's mask IS the edit launch where both are on: one launch rewrites the row for both and rebuilds
    // the ban stage sits between the two and only stores -inf: behind it the partials are rebuilt by the edit (or mask)
    // launch where one follows, else by the rebuild launch alone
    const bool rewritten_later = t.edit || t.guide;
    if (t.pen) ZG_TRY(launch_penalize(c.logits, c.batch, c.vocab, c.pen, c.hist, c.part_val, c.part_idx, c.n_part, c.counts, s, !t.ban && !rewritten_later));
    if (t.ban) {
        ZG_TRY(launch_ban(c.logits, c.batch, c.vocab, c.ban, c.hist, s));
        if (!rewritten_later) ZG_TRY(launch_row_argmax_partials(c.logits, c.batch, c.vocab, c.part_val, c.part_idx, c.n_part, s));
    }
    if (t.guide)
        ZG_TRY(launch_guide_mask(c.logits, c.batch, c.vocab, t.edit ? c.edit_tab : nullptr, t.edit ? c.edit_keep : nullptr, c.guide, c.part_val, c.part_idx,
                                 c.n_part, s));
    else if (t.edit) ZG_TRY(launch_logit_edit(c.logits, c.batch, c.vocab, c.edit_tab, c.edit_keep, c.part_val, c.part_idx, c.n_part, s));
    if (t.sampler == GREEDY) return ZG_OK;
    if (threshold_sampler(t.sampler))  // a filter or min-p: the selection launches, then the tail kernels that read tau
        return launch_sample_filtered(c.logits, c.batch, c.vocab, c.params, filter_launches(t.sampler), c.u, c.ctrl, c.part_val, c.n_part, c.n_part, c.seg_ws,
                                      c.filt, c.pick, c.write_probs, s);
    if (c.ctrl) return launch_sample_step(c.logits, c.batch, c.vocab, c.params, c.ctrl, c.part_val, c.n_part, c.n_part, c.seg_ws, c.pick, s);
    return launch_sample(c.logits, c.batch, c.vocab, c.per_row ? c.params : nullptr, c.temp, c.u, c.part_val, c.n_part, c.n_part, c.seg_ws, c.pick, c.write_probs, s);
}

// How many alternatives a log-probability record may be asked for: the one check of every entry point that takes a top_n
int check_top_n(size_t top_n, size_t vocab, const char* who) {
    ZG_REQUIRE(top_n <= (size_t)ZG_LOGPROBS_TOP_MAX && top_n <= vocab, ZG_ERR_ARG, "%s: top_n %zu outside 0..%zu", who, top_n,
               std::min((size_t)ZG_LOGPROBS_TOP_MAX, vocab));
    return ZG_OK;
}

// `rows` records [ZG_LOGPROBS_TOP_MAX] of ids and values (host) into the packed [rows][top_n] arrays (host) a caller receives
void unpack_top(const int* ids, const float* vals, size_t rows, size_t top_n, size_t* ids_out, float* vals_out) {
    for (size_t i = 0; i < rows; ++i)
        for (size_t j = 0; j < top_n; ++j) {
            ids_out[i * top_n + j] = (size_t)ids[i * ZG_LOGPROBS_TOP_MAX + j];
            vals_out[i * top_n + j] = vals[i * ZG_LOGPROBS_TOP_MAX + j];
        }
}

bool penalties_off(const zg_logit_penalties& p) { return p.repetition == 1.0f && p.presence == 0.0f && p.frequency == 0.0f; }

// ---- Logit edits (include/zgpt2.h zg_logit_edits).  A checked set asks a call for the edit stage (any of the three
// lists: build_edits' stage_on — the set built in the handle's edit.build goes to the device and the edit launch runs) and / or for
// the sampler's min-p threshold
bool edits_off(const zg_logit_edits& e) { return e.n_bias == 0 && e.n_allowed == 0 && e.n_banned == 0 && e.min_p == 0.0f; }

// The refusals of a set of edits over `vocab` logits (include/zgpt2.h), and — where any list is given — the set as the kernel
// reads it, built into `block` (edit_block_bytes(vocab) bytes of plain host memory): the bias pairs sorted by id, then the keep
// bitmap.  Nothing else is touched.
int build_edits(const zg_logit_edits* e, size_t vocab, const char* who, char* block, bool* stage_on) {
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

// ---- Guided decoding (include/zgpt2.h zg_guide).  The one place that checks a table and builds what the mask reads
size_t guide_keep_words(size_t vocab) { return (vocab + 31) / 32; }

// The refusals of a table over `vocab` tokens, and the keep bitmap of every state into keep [n_states][guide_keep_words(vocab)]
// (plain host memory of ZG_GUIDE_MAX_STATES rows): bit i of row s set iff next[s][i] is a state.  Bits behind the vocabulary stay
// clear.  Nothing else is touched.
int build_guide(const zg_guide* gd, size_t vocab, const char* who, unsigned* keep) {
    ZG_REQUIRE(gd != nullptr && gd->next != nullptr, ZG_ERR_ARG, "%s: the guide or its table is null", who);
    ZG_REQUIRE(gd->n_states >= 1 && gd->n_states <= (size_t)ZG_GUIDE_MAX_STATES, ZG_ERR_ARG, "%s: %zu states outside 1..%d", who, gd->n_states,
               ZG_GUIDE_MAX_STATES);
    const size_t words = guide_keep_words(vocab);
    memset(keep, 0, gd->n_states * words * 4);
    for (size_t st = 0; st < gd->n_states; ++st) {
        const uint16_t* row = gd->next + st * vocab;
        unsigned* k = keep + st * words;
        size_t kept = 0;
        for (size_t i = 0; i < vocab; ++i) {
            if (row[i] == ZG_GUIDE_DEAD) continue;
            ZG_REQUIRE(row[i] < gd->n_states, ZG_ERR_ARG, "%s: state %zu goes to state %u of %zu on token %zu", who, st, (unsigned)row[i], gd->n_states, i);
            k[i >> 5] |= 1u << (i & 31);
            ++kept;
        }
        ZG_REQUIRE(kept >= 1, ZG_ERR_ARG, "%s: state %zu allows no token", who, st);
    }
    return ZG_OK;
}

// The refusals of a guided call: start_states [n] against the loaded table (guide_keep null: none is loaded), its keep bitmaps
// against the call's own keep set (call_keep null: the call has no lists) — EVERY state of the table must keep a token, a popcount of
// the AND per state —, and greedy picking beside a guided row.  states_out [n] (optional): the states as the device holds them, -1
// for ZG_GUIDE_NONE; *any_out: some row is guided.  With no guided row nothing of the table is asked.
int check_guide_call(const unsigned* guide_keep, size_t n_states, size_t vocab, const unsigned* call_keep, const size_t* start_states, size_t n, bool greedy,
                     const char* who, int* states_out, bool* any_out) {
    ZG_REQUIRE(start_states != nullptr, ZG_ERR_ARG, "%s: start_states is null", who);
    bool any = false;
    for (size_t b = 0; b < n; ++b) {
        const bool none = start_states[b] == ZG_GUIDE_NONE;
        any = any || !none;
        if (!none) {
            ZG_REQUIRE(guide_keep != nullptr, ZG_ERR_ARG, "%s: row %zu starts in state %zu but no guide is loaded", who, b, start_states[b]);
            ZG_REQUIRE(start_states[b] < n_states, ZG_ERR_ARG, "%s: row %zu starts in state %zu of %zu", who, b, start_states[b], n_states);
        }
        if (states_out) states_out[b] = none ? -1 : (int)start_states[b];
    }
    *any_out = any;
    if (!any) return ZG_OK;
    ZG_REQUIRE(!greedy, ZG_ERR_ARG, "%s: a guide without sampler options (greedy picking with a guide is top_k = 1)", who);
    const size_t words = guide_keep_words(vocab);
    for (size_t st = 0; call_keep && st < n_states; ++st) {
        size_t kept = 0;
        for (size_t w = 0; w < words; ++w) kept += (size_t)__builtin_popcount(guide_keep[st * words + w] & call_keep[w]);
        ZG_REQUIRE(kept >= 1, ZG_ERR_ARG, "%s: the allow and ban lists leave state %zu no token", who, st);
    }
    return ZG_OK;
}

// ---- History-dependent bans (include/zgpt2.h zg_ban_rules).  The one place that checks a rule set and lays it out

// the size of a call's static keep set: the popcount of the keep bitmap behind the bias table of a built edit block (build_edits
// with the stage on), or the whole vocabulary without one
size_t edits_kept(const char* block, size_t vocab) {
    if (!block) return vocab;
    const unsigned* keep = reinterpret_cast<const unsigned*>(block + sizeof(EditTable));
    size_t kept = 0;
    for (size_t w = 0; w < (vocab + 31) / 32; ++w) kept += (size_t)__builtin_popcount(keep[w]);
    return kept;
}

// The refusals of a rule set for a call of `batch` rows over `vocab` tokens on a handle of `context` positions, whose static keep
// set holds `kept` tokens, which runs n_steps steps behind priors of prior_lens[b] tokens (null: none), picks greedily (greedy) or
// has a guided row (guided).  r null: no rules.  *on_out: some rule is on — off, the call is the one without rules and nothing but
// the arguments' own validity is asked.
int check_bans(const zg_ban_rules* r, size_t batch, size_t vocab, size_t context, size_t kept, size_t n_steps, const size_t* prior_lens, bool greedy,
               bool guided, const char* who, bool* on_out) {
    *on_out = false;
    if (!r) return ZG_OK;
    ZG_REQUIRE(r->size == sizeof(zg_ban_rules), ZG_ERR_ARG, "%s: the size field of the ban rules is %zu, not sizeof(zg_ban_rules)", who, r->size);
    ZG_REQUIRE(batch >= 1 && batch <= (size_t)kBanMaxRows, ZG_ERR_ARG, "%s: ban rules for %zu rows (1 .. %d)", who, batch, kBanMaxRows);
    ZG_REQUIRE((r->n_words == 0 || (r->words && r->word_lens)) && (r->n_suppress == 0 || r->suppress_ids), ZG_ERR_ARG,
               "%s: ban rules: a null array with a non-zero count", who);
    ZG_REQUIRE(r->n_words <= (size_t)ZG_BAN_MAX_WORDS && r->n_suppress <= (size_t)ZG_BAN_MAX_SUPPRESS, ZG_ERR_ARG,
               "%s: %zu bad words / %zu suppress ids above %d / %d", who, r->n_words, r->n_suppress, ZG_BAN_MAX_WORDS, ZG_BAN_MAX_SUPPRESS);
    bool on = r->n_words != 0;
    for (size_t b = 0; r->no_repeat_ngram && b < batch; ++b) {
        ZG_REQUIRE(r->no_repeat_ngram[b] <= (size_t)ZG_BAN_MAX_NGRAM, ZG_ERR_ARG, "%s: row %zu: no_repeat_ngram %zu above %d", who, b, r->no_repeat_ngram[b],
                   ZG_BAN_MAX_NGRAM);
        on = on || r->no_repeat_ngram[b] != 0;
    }
    for (size_t b = 0; r->min_tokens && b < batch; ++b) on = on || (r->min_tokens[b] != 0 && r->n_suppress != 0);
    for (size_t k = 0; k < r->n_words; ++k)
        ZG_REQUIRE(r->word_lens[k] >= 1 && r->word_lens[k] <= (size_t)ZG_BAN_MAX_WORD_LEN && r->word_lens[k] <= r->word_stride, ZG_ERR_ARG,
                   "%s: bad word %zu has length %zu (1 .. %d, stride %zu)", who, k, r->word_lens[k], ZG_BAN_MAX_WORD_LEN, r->word_stride);
    for (size_t k = 0; k < r->n_words; ++k)
        for (size_t i = 0; i < r->word_lens[k]; ++i)
            ZG_REQUIRE(r->words[k * r->word_stride + i] < vocab, ZG_ERR_SHAPE, "%s: token %zu of bad word %zu >= vocab %zu", who, r->words[k * r->word_stride + i], k,
                       vocab);
    for (size_t j = 0; j < r->n_suppress; ++j)
        ZG_REQUIRE(r->suppress_ids[j] < vocab, ZG_ERR_SHAPE, "%s: suppress id %zu >= vocab %zu", who, r->suppress_ids[j], vocab);
    if (!on) return ZG_OK;
    ZG_REQUIRE(context <= (size_t)kPenMaxHistory, ZG_ERR_UNSUPPORTED, "%s: context_size %zu beyond the %d tokens of history the ban kernel's LDS holds", who,
               context, kPenMaxHistory);
    ZG_REQUIRE(!greedy, ZG_ERR_ARG, "%s: ban rules without sampler options (greedy picking with bans is top_k = 1)", who);
    ZG_REQUIRE(!guided, ZG_ERR_ARG, "%s: ban rules beside a guided row (a grammar compiles its bad words into the table)", who);
    // a row of -inf alone never reaches a kernel: the most the rules can ban in any row, at any step, leaves a token of the keep set
    for (size_t b = 0; b < batch; ++b) {
        const size_t n = r->no_repeat_ngram ? r->no_repeat_ngram[b] : 0, mt = r->min_tokens ? r->min_tokens[b] : 0;
        const size_t hist = std::min((prior_lens ? prior_lens[b] : 0) + n_steps, vocab);
        const size_t d = (n > 0 ? hist : 0) + r->n_words + (mt > 0 ? r->n_suppress : 0);
        ZG_REQUIRE(kept >= 1 + d, ZG_ERR_ARG, "%s: row %zu: the ban rules could forbid %zu tokens of the %zu the call keeps (no token would be left)", who, b, d,
                   kept);
    }
    *on_out = true;
    return ZG_OK;
}

// Checked rules as the kernel reads them (a null array: all off)
void fill_bans(BanRules* d, const zg_ban_rules& r, size_t batch, size_t past_len) {
    memset(d, 0, sizeof(*d));
    d->n_words = (int)r.n_words;
    d->n_suppress = (int)r.n_suppress;
    d->past_len = (int)past_len;
    for (size_t b = 0; b < batch; ++b) {
        d->ngram[b] = r.no_repeat_ngram ? (int)r.no_repeat_ngram[b] : 0;
        d->min_tokens[b] = r.min_tokens ? (int)std::min(r.min_tokens[b], (size_t)INT32_MAX) : 0;
    }
    for (size_t j = 0; j < r.n_suppress; ++j) d->suppress[j] = (int)r.suppress_ids[j];
    for (size_t k = 0; k < r.n_words; ++k) {
        d->word_len[k] = (int)r.word_lens[k];
        for (size_t i = 0; i < r.word_lens[k]; ++i) d->words[k][i] = (int)r.words[k * r.word_stride + i];
    }
}

// The options of a sampler call over `vocab` logits into *p, the host image of SampleParams (the caller uploads it); returns the
// sampler they need: the plain one with both filters and min-p off, the threshold-aware tail alone for min-p alone
SamplerMode fill_sample_params(SampleParams* p, size_t vocab, const zg_sample_options& o, uint64_t seed, float min_p) {
    const bool k_on = o.top_k >= 1 && o.top_k < vocab, p_on = o.top_p < 1.0f;
    p->inv_temp = 1.0f / o.temp;
    p->top_k = k_on ? (unsigned)o.top_k : 0u;
    p->seed = seed;
    p->top_p = p_on ? o.top_p : 1.0f;
    p->min_p_off = min_p_offset(o.temp, min_p);
    return k_on && p_on ? TWO_FILTERS : (k_on || p_on) ? ONE_FILTER : min_p != 0.0f ? MINP_ONLY : PLAIN;
}

// A table of one zg_row_sampling per row, checked (the message names the row) and laid out as the kernels read it: sp[b] / pp[b],
// the host images of SampleParams / PenParams (either may be null: nothing is filled there), forms[b] = the sampler form row b has
// by its own parameters — exactly fill_sample_params' —, and *tail = what the chain is launched as, the union of the rows' needs:
// the levels of the row that needs most, the threshold-aware tail if any row has a filter or min-p, the penalty stage if any row
// is penalised.  The one place a row's parameters become a launch; every sampler call, uniform ones included, comes through here.
int plan_rows(const zg_row_sampling* rows, size_t n_rows, size_t vocab, size_t past_len, const char* who, SampleParams* sp, PenParams* pp, int* forms,
              StepTail* tail) {
    ZG_REQUIRE(rows != nullptr && n_rows >= 1, ZG_ERR_ARG, "%s: rows is null or empty", who);
    SamplerMode u = PLAIN;
    bool pen = false;
    for (size_t b = 0; b < n_rows; ++b) {
        char row[96];
        snprintf(row, sizeof row, "%s: row %zu", who, b);
        const zg_row_sampling& r = rows[b];
        ZG_TRY(check_sample_options(&r.options, row));
        ZG_REQUIRE(r.min_p >= 0.0f && r.min_p < 1.0f, ZG_ERR_ARG, "%s: min_p %f outside [0, 1)", row, r.min_p);  // (a NaN fails it)
        ZG_TRY(check_penalties(&r.penalties, row));
        SampleParams one;
        const SamplerMode m = fill_sample_params(sp ? &sp[b] : &one, vocab, r.options, r.seed, r.min_p);
        if (pp) pp[b] = PenParams{r.penalties.repetition, r.penalties.presence, r.penalties.frequency, (int)past_len};
        if (forms) forms[b] = (int)m;
        // (PLAIN < MINP_ONLY < ONE_FILTER < TWO_FILTERS by what is launched: the tail kernels, then three levels, then six)
        if (filter_launches(m) > filter_launches(u) || (u == PLAIN && m == MINP_ONLY)) u = m;
        pen = pen || !penalties_off(r.penalties);
    }
    *tail = StepTail{u, pen};
    return ZG_OK;
}

// the table of a uniform call: n_rows equal entries
void uniform_rows(zg_row_sampling* rows, size_t n_rows, const zg_sample_options& o, float min_p, const zg_logit_penalties* pen_or_null, uint64_t seed) {
    for (size_t b = 0; b < n_rows; ++b) rows[b] = zg_row_sampling{o, min_p, pen_or_null ? *pen_or_null : zg_logit_penalties{1.0f, 0.0f, 0.0f}, seed};
}

int check_penalties(const zg_logit_penalties* p, const char* who) {
    ZG_REQUIRE(p != nullptr, ZG_ERR_ARG, "%s: penalties is null", who);
    ZG_REQUIRE(p->repetition > 0.0f, ZG_ERR_ARG, "%s: repetition penalty %f (must be > 0)", who, p->repetition);  // (a NaN fails it)
    ZG_REQUIRE(std::isfinite(p->presence) && std::isfinite(p->frequency), ZG_ERR_ARG, "%s: presence %f / frequency %f penalty", who, p->presence,
               p->frequency);
    return ZG_OK;
}

int check_sample_options(const zg_sample_options* o, const char* who) {
    ZG_REQUIRE(o != nullptr, ZG_ERR_ARG, "%s: options is null", who);
    ZG_REQUIRE(o->temp > 0.0f, ZG_ERR_ARG, "%s: temperature %f", who, o->temp);
    ZG_REQUIRE(o->top_p > 0.0f && o->top_p <= 1.0f, ZG_ERR_ARG, "%s: top_p %f outside (0, 1]", who, o->top_p);  // (a NaN fails both)
    return ZG_OK;
}

// The refusals of a set of stop conditions (include/zgpt2.h), vocab standing for the first token that cannot occur
int check_stop(const zg_stop_conditions* c, size_t vocab, const char* who) {
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
void fill_stop(StopConds* d, const zg_stop_conditions& c) {
    memset(d, 0, sizeof(*d));
    d->n_ids = (int)c.n_ids;
    d->n_seqs = (int)c.n_seqs;
    for (size_t j = 0; j < c.n_ids; ++j) d->ids[j] = (int)c.ids[j];
    for (size_t k = 0; k < c.n_seqs; ++k) {
        d->seq_len[k] = (int)c.seq_lens[k];
        for (size_t i = 0; i < c.seq_lens[k]; ++i) d->seq[k][i] = (int)c.seqs[k * c.seq_stride + i];
    }
}

// The refusals of a beam generation (include/zgpt2.h zg_beam_options), on what the handle is: its rows, vocabulary, context and
// cached positions.  The prompts are judged as far as the beam rules need them (equal lengths, equal within a group); their
// tokens and the room in the context are the generation's own checks.
int check_beam(const zg_generate_request* q, const zg_beam_options* o, size_t batch, size_t vocab, size_t context, size_t cached_len, const char* who) {
    ZG_REQUIRE(q != nullptr && q->size == sizeof(zg_generate_request), ZG_ERR_ARG, "%s: null request, or its size field is not sizeof(zg_generate_request)", who);
    ZG_REQUIRE(o != nullptr && o->size == sizeof(zg_beam_options), ZG_ERR_ARG, "%s: null options, or their size field is not sizeof(zg_beam_options)", who);
    ZG_REQUIRE(!q->options && !q->penalties && !q->prior && !q->prior_stride && !q->prior_lens && !q->logprobs && !q->top_n && !q->stop && !q->edits, ZG_ERR_ARG,
               "%s: options, penalties, prior, logprobs, stop and edits must be NULL / 0 (beams over such a distribution are not offered)", who);
    const size_t W = o->num_beams;
    ZG_REQUIRE(W >= 1 && W <= ZG_BEAM_MAX, ZG_ERR_ARG, "%s: num_beams %zu outside 1..%d", who, W, ZG_BEAM_MAX);
    ZG_REQUIRE(batch >= 1 && batch <= (size_t)kBeamRows && batch % W == 0, ZG_ERR_ARG, "%s: a batch of %zu is no multiple of num_beams %zu", who, batch, W);
    ZG_REQUIRE(2 * W <= vocab, ZG_ERR_ARG, "%s: 2 x num_beams %zu above the vocabulary of %zu", who, W, vocab);
    ZG_REQUIRE(std::isfinite(o->length_penalty), ZG_ERR_ARG, "%s: length_penalty is not finite", who);
    ZG_REQUIRE(o->eos_id == ZG_BEAM_NO_EOS || o->eos_id < vocab, ZG_ERR_SHAPE, "%s: eos_id %zu >= vocab %zu", who, o->eos_id, vocab);
    ZG_REQUIRE(q->prompts && q->prompt_lens, ZG_ERR_ARG, "%s: null prompts", who);
    ZG_REQUIRE(q->past_len <= cached_len && q->past_len <= context, ZG_ERR_ARG, "%s: past_len %zu beyond the %zu cached positions", who, q->past_len, cached_len);
    const size_t np = q->prompt_lens[0];
    for (size_t b = 1; b < batch; ++b)
        ZG_REQUIRE(q->prompt_lens[b] == np, ZG_ERR_ARG, "%s: prompt %zu has %zu tokens, prompt 0 has %zu (beam rows run in lock step)", who, b, q->prompt_lens[b], np);
    ZG_REQUIRE(np >= 1 && np <= q->prompt_stride, ZG_ERR_SHAPE, "%s: prompts of %zu tokens in rows of %zu", who, np, q->prompt_stride);
    ZG_REQUIRE(q->n_steps > np, ZG_ERR_ARG, "%s: n_steps %zu picks nothing behind prompts of %zu tokens", who, q->n_steps, np);
    for (size_t b = 0; b < batch; ++b)
        for (size_t i = 0; i < np; ++i)
            ZG_REQUIRE(q->prompts[b * q->prompt_stride + i] == q->prompts[(b / W) * W * q->prompt_stride + i], ZG_ERR_ARG,
                       "%s: prompt %zu differs from prompt %zu of its group at token %zu", who, b, (b / W) * W, i);
    return ZG_OK;
}

// The state a beam generation starts from (sample_beam.h): the options, slot g W of every group live with score 0, empty pools
void fill_beam_state(BeamState* d, const zg_beam_options& o, size_t c0) {
    memset(d, 0, sizeof(*d));
    d->W = (int)o.num_beams;
    d->eos = o.eos_id == ZG_BEAM_NO_EOS ? -1 : (int)o.eos_id;
    d->early = o.early_stopping != 0;
    d->c0 = (int)c0;
    for (int s = 0; s < kBeamRows; ++s) {
        d->score[s] = s % d->W == 0 ? 0.0f : -INFINITY;
        d->src[s] = s;
        d->done_col[s] = -1;
    }
}

// lenpow[L] = (float)pow((double)L, (double)length_penalty), L = 0 .. n - 1
void fill_lenpow(float* d, size_t n, float length_penalty) {
    for (size_t L = 0; L < n; ++L) d[L] = (float)pow((double)L, (double)length_penalty);
}

}  // namespace zg

extern "C" {

// check_beam's face (tests; no GPU, no zg_init)
int zg_debug_beam_check(const zg_generate_request* r, const zg_beam_options* beam, size_t batch, size_t vocab, size_t context, size_t cached_len) {
    return check_beam(r, beam, batch, vocab, context, cached_len, "debug_beam_check");
}

// plan_rows' face (tests; no GPU, no zg_init): out[0] the sampler form the chain is launched in, out[1] whether the penalty stage
// runs, out[2 + b] the form of row b
int zg_debug_each_plan(const zg_row_sampling* rows, size_t n_rows, size_t vocab, int* out, size_t n_out) {
    ZG_REQUIRE(out != nullptr && vocab >= 1 && n_rows <= 64 && n_out >= 2 + n_rows, ZG_ERR_ARG, "debug_each_plan: %zu rows, vocab %zu, %zu outputs", n_rows, vocab,
               n_out);
    StepTail t;
    ZG_TRY(plan_rows(rows, n_rows, vocab, 0, "debug_each_plan", nullptr, nullptr, out + 2, &t));
    out[0] = (int)t.sampler;
    out[1] = t.pen ? 1 : 0;
    return ZG_OK;
}

// build_guide's and check_guide_call's face (tests, and the Python builders; no GPU, no zg_init): a load of `guide`, then a call
int zg_debug_guide_check(const zg_guide* guide, size_t vocab, const zg_logit_edits* edits, const size_t* start_states, size_t n, int greedy) {
    ZG_REQUIRE(vocab >= 1 && vocab <= (size_t)64 * 4096 && n <= 64, ZG_ERR_ARG, "debug_guide_check: vocab %zu, %zu rows", vocab, n);
    std::vector<unsigned> keep((size_t)ZG_GUIDE_MAX_STATES * guide_keep_words(vocab));
    ZG_TRY(build_guide(guide, vocab, "debug_guide_check", keep.data()));
    if (n == 0) return ZG_OK;
    std::vector<char> block(edit_block_bytes(vocab));
    bool stage_on = false, any = false;
    if (edits) ZG_TRY(build_edits(edits, vocab, "debug_guide_check", block.data(), &stage_on));
    return check_guide_call(keep.data(), guide->n_states, vocab, stage_on ? reinterpret_cast<const unsigned*>(block.data() + sizeof(EditTable)) : nullptr,
                            start_states, n, greedy != 0, "debug_guide_check", nullptr, &any);
}

// check_bans' face (tests; no GPU, no zg_init): the refusal of a banned call with these rules, the edits' own refusals included
int zg_debug_ban_check(const zg_ban_rules* bans, size_t batch, size_t vocab, size_t context, const zg_logit_edits* edits, size_t n_steps,
                       const size_t* prior_lens, int greedy, int guided) {
    ZG_REQUIRE(vocab >= 1 && vocab <= (size_t)64 * 4096 && batch >= 1 && batch <= (size_t)kBanMaxRows, ZG_ERR_ARG, "debug_ban_check: vocab %zu, %zu rows", vocab,
               batch);
    std::vector<char> block(edit_block_bytes(vocab));
    bool stage_on = false, on = false;
    if (edits) ZG_TRY(build_edits(edits, vocab, "debug_ban_check", block.data(), &stage_on));
    return check_bans(bans, batch, vocab, context, edits_kept(stage_on ? block.data() : nullptr, vocab), n_steps, prior_lens, greedy != 0, guided != 0,
                      "debug_ban_check", &on);
}

int zg_debug_min_p_offset(float temp, float min_p, float* d_out) {
    ZG_REQUIRE(d_out != nullptr && temp > 0.0f && min_p >= 0.0f && min_p < 1.0f, ZG_ERR_ARG, "debug_min_p_offset: temp %f, min_p %f", temp, min_p);
    *d_out = min_p_offset(temp, min_p);
    return ZG_OK;
}

}  // extern "C"
