"""Python mirror of the model side of the reference (src/main.zig) over the C ABI.

`GPT` wraps the device-resident model tier (zg_gpt_*): State.init + load_gpt become the
constructor and `load_weights`, GPT.forward keeps its (seq_len, token, compute_logits) meaning,
`generate` is the reference decode loop with greedy argmax in place of the sampler.
`HostGPT` is the op-tier composition: main.zig's State/MLP/Block/GPT written against ops.py
exactly as main.zig is written against ops.zig (used to test the drop-in boundary).
"""
import ctypes as C

import numpy as np

from . import _lib, ops
from ._lib import check, ptr
from .synth import GPTConfig


def _pack_prompts(prompts, rows):
    """`rows` prompts of any lengths -> (tokens [rows, stride] padded with zeros, lengths [rows], stride)."""
    prompts = [np.atleast_1d(np.asarray(p, dtype=np.uint64)) for p in prompts]
    assert len(prompts) == rows
    stride = max(len(p) for p in prompts)
    mat = np.zeros((rows, stride), np.uint64)
    lens = np.zeros(rows, np.uint64)
    for b, p in enumerate(prompts):
        mat[b, : len(p)] = p
        lens[b] = len(p)
    return mat, lens, stride


class GPT:
    def __init__(self, config: GPTConfig, batch=1, weights_f32=False, use_graph=True, kv_f16=False, prefill=True,
                 prefill_planes=3, prefetch=True, kv_b24=False, share_weights_with=None, own_stream=False, stream_priority=0,
                 sampled_generate=False, weights_b24=False, truncated_generate=False, penalized_generate=False, logprobs_generate=False,
                 score=False, stop_generate=False, edited_generate=False, guided=False, banned_generate=False, beam_generate=False):
        """share_weights_with / own_stream / stream_priority: zg_gpt_options of zg_gpt_create_ex (a handle of an independent
        prompt group on the same GPU: private stream, weight region borrowed from another GPT of the same config).
        weights_b24: matrices stored as 24-bit floats (ZG_GPT_WEIGHTS_B24: each fp32 weight rounded to 16 mantissa bits, 3/4 of
        fp32's bytes); excludes weights_f32.  truncated_generate: the graphs of generate_sample(top_k=..., top_p=...) are captured
        at create (ZG_GPT_TRUNCATED_GENERATE) instead of when the first such generation begins; penalized_generate: the same for
        the graphs of generations with repetition / presence / frequency penalties (ZG_GPT_PENALIZED_GENERATE);
        logprobs_generate: the same for the log-probability twins of every graph create captures (ZG_GPT_LOGPROBS_GENERATE).
        score: carve what `score` / `loglikelihood` need (ZG_GPT_SCORE); without it they raise ZG_ERR_UNSUPPORTED.
        stop_generate: the stop twins of every graph create captures (ZG_GPT_STOP_GENERATE), as the other *_generate flags.
        edited_generate: the graphs of generations with logit edits or min-p (ZG_GPT_EDITED_GENERATE), as the other *_generate flags.
        guided: guided decoding (ZG_GPT_GUIDED_GENERATE) — carve the automaton's table, bitmaps, states and record, and
        capture the guided twins of the sampler graphs create captures; without it `load_guide` and guide_states raise ZG_ERR_UNSUPPORTED.
        banned_generate: the banned twins (no_repeat_ngram_size / bad_words_ids / min_tokens; ZG_GPT_BANNED_GENERATE) of the
        sampler graphs create captures, as the other *_generate flags; without it such a generation captures its graphs when it begins.
        beam_generate: the graphs of `beam_search` (ZG_GPT_BEAM_GENERATE) at create instead of when the first one begins."""
        self.config, self.batch = config, batch
        self._kv_bytes = 2 if kv_f16 else 3 if kv_b24 else 4  # bytes of a cache element (kv_rows)
        L = _lib.load()
        flags = (_lib.GPT_WEIGHTS_F32 if weights_f32 else 0) | (0 if use_graph else _lib.GPT_NO_GRAPH)
        flags |= _lib.GPT_KV_F16 if kv_f16 else 0
        flags |= _lib.GPT_KV_B24 if kv_b24 else 0
        flags |= 0 if prefill else _lib.GPT_NO_PREFILL
        flags |= _lib.GPT_PREFILL_2PLANE if prefill_planes == 2 else 0
        flags |= 0 if prefetch else _lib.GPT_NO_PREFETCH
        flags |= _lib.GPT_SAMPLED_GENERATE if sampled_generate else 0
        flags |= _lib.GPT_WEIGHTS_B24 if weights_b24 else 0
        flags |= _lib.GPT_TRUNCATED_GENERATE if truncated_generate else 0
        flags |= _lib.GPT_PENALIZED_GENERATE if penalized_generate else 0
        flags |= _lib.GPT_LOGPROBS_GENERATE if logprobs_generate else 0
        flags |= _lib.GPT_SCORE if score else 0
        flags |= _lib.GPT_STOP_GENERATE if stop_generate else 0
        flags |= _lib.GPT_EDITED_GENERATE if edited_generate else 0
        flags |= _lib.GPT_GUIDED_GENERATE if guided else 0
        flags |= _lib.GPT_BANNED_GENERATE if banned_generate else 0
        flags |= _lib.GPT_BEAM_GENERATE if beam_generate else 0
        cfg = _lib.GptConfig(config.vocab_size, config.context_size, config.n_layer, config.n_heads, config.n_embed)
        h = C.c_void_p()
        if share_weights_with is None and not own_stream:
            check(L.zg_gpt_create(C.byref(h), C.byref(cfg), batch, flags))
        else:
            opt = _lib.GptOptions(share_weights_with.h if share_weights_with is not None else None, int(bool(own_stream)), int(stream_priority))
            check(L.zg_gpt_create_ex(C.byref(h), C.byref(cfg), batch, flags, C.byref(opt)))
        self._weight_owner = share_weights_with  # keeps the owner alive: it must be destroyed last
        self.h = h
        self._L = L

    @classmethod
    def from_raw_dir(cls, path, config: GPTConfig, weights_b24=False, **kw):
        """load_gpt (src/main.zig:304-314) from a reference-format weight directory.  The matrices keep the reference's fp32
        unless every one of them is bf16-representable (weights_io.flags_for_checkpoint: bf16 storage of an ordinary fp32
        checkpoint is 6e-3 of the logit scale away from the fp32 result, outside the 1e-3 bound).  weights_b24=True: such a
        checkpoint is stored as 24-bit floats instead of fp32 (ZG_GPT_WEIGHTS_B24, 3/4 of the weight bytes)."""
        from . import weights_io

        w = weights_io.load_raw_dir(path, config)
        flags = weights_io.flags_for_checkpoint(w, allow_b24=weights_b24)
        flags.update(kw)
        m = cls(config, **flags)
        m.load_weights(w)
        return m

    def close(self):
        if getattr(self, "h", None):
            self._L.zg_gpt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def load_weights(self, weights):
        """weights: dict name -> fp32 array (numpy or torch), names as synth.tensor_specs."""
        L = self._L
        for s, name in enumerate(_lib.TOP_SLOTS):
            w = weights[name]
            check(L.zg_gpt_load_tensor(self.h, s, ptr(w), ops._n(w)))
        for l in range(self.config.n_layer):
            for s, name in enumerate(_lib.BLOCK_SLOTS):
                w = weights[f"h{l}.{name}"]
                check(L.zg_gpt_load_block_tensor(self.h, l, s, ptr(w), ops._n(w)))

    def weight_arena(self):
        p, n = C.c_void_p(), C.c_size_t()
        check(self._L.zg_gpt_weight_arena(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def step_bytes(self, seq_len):
        w, kv = C.c_size_t(), C.c_size_t()
        check(self._L.zg_gpt_step_bytes(self.h, seq_len, C.byref(w), C.byref(kv)))
        return w.value, kv.value

    # ------------------------------------------------------------------ GPT.forward / sample
    def _logits_buf(self, compute_logits, want_logits):
        return np.empty((self.batch, self.config.vocab_size), np.float32) if compute_logits and want_logits else None

    def forward(self, seq_len, tokens, compute_logits=True, want_logits=True):
        """GPT.forward (src/main.zig:178-195) for `batch` sequences; returns logits [batch, V] or None."""
        tokens = np.ascontiguousarray(np.atleast_1d(tokens), dtype=np.uint64)
        logits = self._logits_buf(compute_logits, want_logits)
        check(self._L.zg_gpt_forward(self.h, seq_len, ptr(tokens), tokens.size, int(compute_logits), ptr(logits),
                                     ops._n(logits)))
        return logits

    def prefill(self, tokens, compute_logits=True, want_logits=True):
        """The prompt loop of generate (src/main.zig:331-334) as one pass: tokens [batch, n] are positions
        0..n-1; returns the logits of position n-1 ([batch, V]) or None."""
        tokens = np.ascontiguousarray(np.atleast_2d(tokens), dtype=np.uint64)
        assert tokens.shape[0] == self.batch
        logits = self._logits_buf(compute_logits, want_logits)
        check(self._L.zg_gpt_prefill(self.h, ptr(tokens), tokens.shape[1], tokens.shape[1], int(compute_logits),
                                     ptr(logits), ops._n(logits)))
        return logits

    def step_taps(self, seq_len, tokens):
        """zg_debug_gpt_step_taps: forward(seq_len, tokens) as an eager step with every launch class tapped.  Returns (taps, info):
        taps is a list of dicts {cls, layer, name, flags, data} in launch order, data the raw buffer as a numpy array of its storage
        type (bf16 planes as uint16); info the handle's decode modes by name (_lib.TAP_INFO)."""
        tokens = np.ascontiguousarray(np.atleast_1d(tokens), dtype=np.uint64)
        used, n = C.c_size_t(), C.c_size_t()
        info = np.zeros(len(_lib.TAP_INFO), np.int32)
        check(self._L.zg_debug_gpt_step_taps(self.h, seq_len, ptr(tokens), tokens.size, None, 0, C.byref(used), None, 0, C.byref(n), ptr(info), info.size))
        arena = np.zeros(used.value, np.uint8)
        table = (_lib.TapEntry * n.value)()
        check(self._L.zg_debug_gpt_step_taps(self.h, seq_len, ptr(tokens), tokens.size, ptr(arena), arena.size, C.byref(used), C.addressof(table), n.value,
                                             C.byref(n), ptr(info), info.size))
        return self._tap_list(arena, table, n.value), dict(zip(_lib.TAP_INFO, (int(v) for v in info)))

    @staticmethod
    def _tap_list(arena, table, n):
        taps = []
        for e in table[:n]:
            dt = np.dtype(_lib.TAP_DTYPES[e.type])
            data = arena[e.offset: e.offset + e.count * dt.itemsize].view(dt).copy()
            taps.append({"cls": e.cls, "layer": e.layer, "name": _lib.TAP_BUFFERS[e.buffer], "flags": e.flags, "data": data})
        return taps

    def pass_taps(self, tokens, past_len=0, compute_logits=True, score=False, top_n=0):
        """zg_debug_gpt_pass_taps: extend(past_len, tokens, compute_logits) — or, with score, score(tokens, past_len, top_n,
        want_logits=True) without the fetch of the records — with every launch of the pass tapped.  Returns (taps, info, logits):
        taps as step_taps (in launch order; include/zgpt2.h lists the classes), info by name (_lib.PASS_INFO), logits [batch, V] of
        the last new position (None without compute_logits), or [batch, n, V] of every position for score."""
        tokens = np.ascontiguousarray(np.atleast_2d(tokens), dtype=np.uint64)
        assert tokens.shape[0] == self.batch
        n_tok = tokens.shape[1]
        logits = np.empty((self.batch, n_tok, self.config.vocab_size), np.float32) if score else self._logits_buf(compute_logits, True)
        used, n = C.c_size_t(), C.c_size_t()
        info = np.zeros(len(_lib.PASS_INFO), np.int32)
        head = (self.h, past_len, ptr(tokens), n_tok, n_tok, int(compute_logits), int(score), int(top_n), ptr(logits), ops._n(logits))
        check(self._L.zg_debug_gpt_pass_taps(*head, None, 0, C.byref(used), None, 0, C.byref(n), ptr(info), info.size))
        arena = np.zeros(used.value, np.uint8)
        table = (_lib.TapEntry * n.value)()
        check(self._L.zg_debug_gpt_pass_taps(*head, ptr(arena), arena.size, C.byref(used), C.addressof(table), n.value, C.byref(n), ptr(info), info.size))
        return self._tap_list(arena, table, n.value), dict(zip(_lib.PASS_INFO, (int(v) for v in info))), logits

    def age(self, n_steps=0, sk_epoch=None):
        """zg_debug_gpt_age: as if n_steps decode steps that wrote no tagged slot had been enqueued and run (nothing on a handle
        without tagged hand-overs); sk_epoch: the epoch the next stream-K launch of the whole-prompt pass continues from."""
        check(self._L.zg_debug_gpt_age(self.h, int(n_steps), int(sk_epoch is not None), int(sk_epoch or 0) & 0xFFFFFFFF))

    def age_state(self):
        """zg_debug_gpt_age_state (drains the stream): dict by _lib.AGE_STATE."""
        out = np.zeros(len(_lib.AGE_STATE), np.uint64)
        check(self._L.zg_debug_gpt_age_state(self.h, ptr(out), out.size))
        return dict(zip(_lib.AGE_STATE, (int(v) for v in out)))

    def tag_census(self, epoch24, sk_flag_value=0):
        """zg_debug_gpt_tag_census: how many tagged words carry epoch24 in their tag's epoch field, by array, and how many stream-K
        flag words equal sk_flag_value: dict by _lib.TAG_CENSUS."""
        out = np.zeros(len(_lib.TAG_CENSUS), np.uintp)
        check(self._L.zg_debug_gpt_tag_census(self.h, int(epoch24), int(sk_flag_value), ptr(out), out.size))
        return dict(zip(_lib.TAG_CENSUS, (int(v) for v in out)))

    def cached_len(self):
        """Positions the handle's caches hold (zg_gpt_cached_len)."""
        n = C.c_size_t()
        check(self._L.zg_gpt_cached_len(self.h, C.byref(n)))
        return n.value

    def extend(self, past_len, tokens, compute_logits=True, want_logits=True):
        """prefill at an offset (zg_gpt_extend): tokens [batch, n] go to positions past_len .. past_len + n - 1 behind the cached
        ones in one pass; returns the logits of the last new position ([batch, V]) or None.  past_len below cached_len() rolls back."""
        tokens = np.ascontiguousarray(np.atleast_2d(tokens), dtype=np.uint64)
        assert tokens.shape[0] == self.batch
        logits = self._logits_buf(compute_logits, want_logits)
        check(self._L.zg_gpt_extend(self.h, past_len, ptr(tokens), max(tokens.shape[1], 1), tokens.shape[1], int(compute_logits), ptr(logits),
                                    ops._n(logits)))
        return logits

    def score(self, tokens, past_len=0, top_n=0, want_logits=False):
        """zg_gpt_score: the pass of extend(past_len, tokens) which also records how likely every token it feeds was.
        tokens [batch, n].  Returns (logprobs [batch, n] float32, top_ids [batch, n, top_n] uint64, top_logprobs [batch, n, top_n]
        float32) of columns past_len .. past_len + n - 1 — column j holds log P(tokens[:, j] | everything before it) and the top_n
        alternatives there; the first column is NaN (its predicting row is not part of the pass) — and, with want_logits, the
        logits of every position [batch, n, V] as the pass computed them."""
        tokens = np.ascontiguousarray(np.atleast_2d(tokens), dtype=np.uint64)
        assert tokens.shape[0] == self.batch
        n = tokens.shape[1]
        logits = np.empty((self.batch, n, self.config.vocab_size), np.float32) if want_logits else None
        check(self._L.zg_gpt_score(self.h, past_len, ptr(tokens), max(n, 1), n, int(top_n), ptr(logits), ops._n(logits)))
        out = self.generate_fetch_logprobs(past_len, n, int(top_n))
        return out + (logits,) if want_logits else out

    def loglikelihood(self, contexts, continuations):
        """The `loglikelihood(context, continuation)` request of evaluation harnesses for `batch` rows in ONE call of `score`:
        contexts and continuations are lists of token lists, one pair per row (a context of at least one token).  Returns a list of
        (sum of the continuation's log-probabilities, is_greedy) per row — is_greedy: every continuation token was the most likely
        one.  Rows are padded at the end to the longest; causality keeps the padding from reaching a row's own columns, which are
        the only ones read."""
        assert len(contexts) == self.batch and len(continuations) == self.batch
        rows = [np.r_[np.asarray(c, np.uint64), np.asarray(k, np.uint64)] for c, k in zip(contexts, continuations)]
        assert all(len(c) >= 1 for c in contexts), "a continuation's first token needs a token in front of it"
        mat, _, _ = _pack_prompts(rows, self.batch)
        lp, ids, _ = self.score(mat, top_n=1)
        out = []
        for b, (c, k) in enumerate(zip(contexts, continuations)):
            cols = slice(len(c), len(c) + len(k))
            out.append((float(lp[b, cols].astype(np.float64).sum()), bool(np.array_equal(ids[b, cols, 0], mat[b, cols]))))
        return out

    def _sampled(self, name, suffix, head, temp, top_k, top_p, tail):
        """zg_gpt_<name><suffix>(h, *head, temp, *tail) while no filter is on (the defaults take the plain entry point itself),
        else its _ex twin with zg_sample_options in temp's place."""
        if top_k == 0 and top_p == 1.0:
            check(getattr(self._L, f"zg_gpt_{name}{suffix}")(self.h, *head, temp, *tail))
        else:
            opt = _lib.SampleOptions(temp, top_k, top_p)
            check(getattr(self._L, f"zg_gpt_{name}_ex{suffix}")(self.h, *head, C.addressof(opt), *tail))

    @staticmethod
    def _penalties(repetition_penalty, presence_penalty, frequency_penalty):
        """zg_logit_penalties, or None while all three are off (the call is then today's, through today's entry point)."""
        if repetition_penalty == 1.0 and presence_penalty == 0.0 and frequency_penalty == 0.0:
            return None
        return _lib.LogitPenalties(repetition_penalty, presence_penalty, frequency_penalty)

    @staticmethod
    def _edits(logit_bias, allowed_token_ids, banned_token_ids, min_p):
        """(zg_logit_edits, its arrays), or None while everything is off (the call is then today's, through today's entry point).
        An allow-list that is given but empty is not "off": it reaches the library, which refuses it."""
        if not logit_bias and allowed_token_ids is None and not len(banned_token_ids if banned_token_ids is not None else ()) and min_p == 0.0:
            return None
        if allowed_token_ids is not None and len(allowed_token_ids) == 0:
            raise ValueError("allowed_token_ids is empty: no token could be picked")
        return _lib.logit_edits(logit_bias, allowed_token_ids, banned_token_ids, min_p)

    def _bans(self, no_repeat_ngram_size, bad_words_ids, min_tokens, suppress_token_ids, stop_token_ids=None):
        """(zg_ban_rules, its arrays), or None while every rule is off (the call is then today's, through today's entry point).
        no_repeat_ngram_size / min_tokens: one value for every row, or one per row.  suppress_token_ids None: the call's stop_token_ids."""
        if suppress_token_ids is None:
            suppress_token_ids = stop_token_ids
        n_on = bool(np.any(np.asarray(no_repeat_ngram_size) != 0))
        min_on = bool(np.any(np.asarray(min_tokens) != 0)) and suppress_token_ids is not None and len(suppress_token_ids) > 0
        if not n_on and not bad_words_ids and not min_on:
            return None
        return _lib.ban_rules(self.batch, no_repeat_ngram_size, bad_words_ids, min_tokens, suppress_token_ids)

    def _request_enqueue(self, past, mat, stride, lens, n_steps, temp, seed, top_k, top_p, pen, prior, logprobs, conds, edits, guide_states=None, bans=None):
        """zg_gpt_generate_request_enqueue: the one call every generation with penalties, log-probabilities, stop conditions or
        edits goes through.  conds: a zg_stop_conditions or None; edits: `_edits(...)`.  guide_states (one start state per row, None
        for a row without a guide): the same request through zg_gpt_generate_guided_enqueue.  bans (`_bans(...)`): through
        zg_gpt_generate_banned_enqueue."""
        if (pen is not None or edits is not None or bans is not None) and temp is None:
            raise ValueError("penalties, edits and bans need a sampler: greedy picking with them is temp=1.0, top_k=1")
        if bans is not None and guide_states is not None:
            raise ValueError("ban rules and a guide cannot be combined: a grammar compiles its bad words into the table")
        opt = None if temp is None else _lib.SampleOptions(temp, top_k, top_p)
        pp, pstride, plens, keep = self._token_lists(prior if pen is not None or bans is not None else None)
        r = _lib.generate_request(past_len=past, prompts=ptr(mat), prompt_stride=stride, prompt_lens=ptr(lens), n_steps=n_steps,
                                  options=None if opt is None else C.addressof(opt), penalties=None if pen is None else C.addressof(pen), prior=pp,
                                  prior_stride=pstride, prior_lens=plens, seed=seed, logprobs=int(logprobs is not None), top_n=int(logprobs or 0),
                                  stop=None if conds is None else C.addressof(conds), edits=None if edits is None else C.addressof(edits[0]))
        if bans is not None:
            check(self._L.zg_gpt_generate_banned_enqueue(self.h, C.addressof(r), None, 0, C.addressof(bans[0])))
        elif guide_states is None:
            check(self._L.zg_gpt_generate_request_enqueue(self.h, C.addressof(r)))
        else:
            states = self._guide_states(guide_states)
            check(self._L.zg_gpt_generate_guided_enqueue(self.h, C.addressof(r), None, 0, ptr(states)))
        del keep

    # ------------------------------------------------------------------ guided decoding
    def load_guide(self, guide):
        """zg_gpt_guide_load: the automaton (a guide.Guide) later generations' guide_states refer to; None unloads.  The one slow
        call of the feature: once per grammar, not per request."""
        if guide is None:
            check(self._L.zg_gpt_guide_load(self.h, None))
        else:
            g = guide.c_struct()
            check(self._L.zg_gpt_guide_load(self.h, C.addressof(g)))

    def _guide_states(self, guide_states):
        states = np.array([_lib.GUIDE_NONE if st is None else int(st) for st in guide_states], np.uint64)
        if states.size != self.batch:
            raise ValueError(f"guide_states: {states.size} start states for a batch of {self.batch}")
        return states

    def generate_fetch_guide_states(self, first, n):
        """zg_gpt_generate_fetch_guide_states of columns first .. first + n - 1: [batch, n] uint64, the state each column's pick was
        drawn in, or guide.NONE for a prompt column and for an unguided row.  A second turn starts a row in
        guide.step(state of its last picked column, the token there)."""
        out = np.zeros((self.batch, n), np.uint64)
        check(self._L.zg_gpt_generate_fetch_guide_states(self.h, first, n, ptr(out), out.size))
        return out

    def _token_lists(self, lists):
        """One token list per row (None: none) -> (ptr or None, stride, ptr to lengths or None), with the arrays kept alive."""
        if lists is None:
            return None, 0, None, ()
        mat, lens, stride = _pack_prompts([np.zeros(0, np.uint64) if h is None else h for h in lists], self.batch)
        if mat.shape[1] == 0:
            mat, stride = np.zeros((self.batch, 1), np.uint64), 1
        return ptr(mat), stride, ptr(lens), (mat, lens)

    def _generate_stop(self, past_len, prompts, n_steps, temp, seed, top_k, top_p, pen, prior, logprobs, stop_token_ids, stop, lookahead, edits=None,
                       guide_states=None, bans=None):
        """A generation with stop conditions (the request call): what `_generate` returns, cut at `end` —
        columns past_len .. end - 1.  `stop_result()` tells where every row finished and why."""
        past = past_len or 0
        mat, lens, stride = self._prompts(prompts)
        conds, keep_conds = _lib.stop_conditions(stop_token_ids, stop, lookahead)
        self._request_enqueue(past, mat, stride, lens, n_steps, temp, seed, top_k, top_p, pen, prior, logprobs, conds, edits, guide_states, bans)
        del keep_conds
        n = self.stop_result()[0] - past if conds.n_ids or conds.n_seqs else n_steps  # (no conditions: the plain call ran)
        out = self.generate_fetch_range(past, n)
        return out if logprobs is None else (out,) + self.generate_fetch_logprobs(past, n, logprobs)

    def stop_result(self):
        """zg_gpt_generate_stop_result of the last generation with stop conditions: (end, finish_cols, reasons) — `end` the absolute
        column the generation ended at (exclusive), per row the absolute column it finished at (None: it never did) and the index
        of the condition that matched there (stop tokens first, then the sequences; -1: none)."""
        end = C.c_size_t()
        cols = np.zeros(self.batch, np.uint64)
        reasons = np.zeros(self.batch, np.int32)
        check(self._L.zg_gpt_generate_stop_result(self.h, C.byref(end), ptr(cols), ptr(reasons)))
        return end.value, [None if int(c) == _lib.STOP_NONE else int(c) for c in cols], [int(r) for r in reasons]

    def _generate(self, past_len, prompts, n_steps, temp, seed, top_k, top_p, pen, prior, logprobs, fetch=True, edits=None, guide_states=None, bans=None):
        """Every generation of this class: enqueue through the entry point its arguments ask for, then (fetch) return what the
        public method returns.  past_len None: not a continuation.  temp None: greedy.  pen: `_penalties(...)`.  logprobs: top_n or
        None.  edits: `_edits(...)`.  With penalties, log-probabilities and edits off the plain entry points run
        (zg_gpt_generate_greedy / _enqueue, zg_gpt_generate_sample[_ex][_enqueue], zg_gpt_generate_from_enqueue), else the request
        call (zg_gpt_generate_request_enqueue)."""
        if (pen is not None or edits is not None or bans is not None) and temp is None:
            raise ValueError("penalties, edits and bans need a sampler: greedy picking with them is temp=1.0, top_k=1")
        mat, lens, stride = self._prompts(prompts)
        head = (ptr(mat), stride, ptr(lens), n_steps)
        opt = None if temp is None else _lib.SampleOptions(temp, top_k, top_p)
        opt_p = None if opt is None else C.addressof(opt)
        out = None
        if logprobs is not None or pen is not None or edits is not None or guide_states is not None or bans is not None:
            self._request_enqueue(past_len or 0, mat, stride, lens, n_steps, temp, seed, top_k, top_p, pen, prior, logprobs, None, edits, guide_states, bans)
        elif past_len is not None:
            check(self._L.zg_gpt_generate_from_enqueue(self.h, past_len, *head, opt_p, seed))
        elif fetch:  # the calls that enqueue and fetch in one
            out = np.zeros((self.batch, n_steps), np.uint64)
            if temp is None:
                check(self._L.zg_gpt_generate_greedy(self.h, *head, ptr(out), out.size))
            else:
                self._sampled("generate_sample", "", head, temp, top_k, top_p, (seed, ptr(out), out.size))
        elif temp is None:
            check(self._L.zg_gpt_generate_enqueue(self.h, *head))
        else:
            self._sampled("generate_sample", "_enqueue", head, temp, top_k, top_p, (seed,))
        if not fetch:
            return None
        if out is None:
            out = self.generate_fetch(n_steps) if past_len is None else self.generate_fetch_range(past_len, n_steps)
        return out if logprobs is None else (out,) + self.generate_fetch_logprobs(past_len or 0, n_steps, logprobs)

    def generate_fetch_logprobs(self, first, n, top_n):
        """zg_gpt_generate_fetch_logprobs of columns first .. first + n - 1: (logprobs [batch, n] float32 — NaN where the column
        records a prompt token —, top_ids [batch, n, top_n] uint64, top_logprobs [batch, n, top_n] float32)."""
        lp = np.zeros((self.batch, n), np.float32)
        ids = np.zeros((self.batch, n, top_n), np.uint64)
        top = np.zeros((self.batch, n, top_n), np.float32)
        check(self._L.zg_gpt_generate_fetch_logprobs(self.h, first, n, top_n, ptr(lp), lp.size, ptr(ids) if top_n else None,
                                                     ptr(top) if top_n else None, ids.size))
        return lp, ids, top

    def sample(self, seq_len, tokens, temp, uniforms=None, seed=0, want_probs=False, top_k=0, top_p=1.0, repetition_penalty=1.0,
               presence_penalty=0.0, frequency_penalty=0.0, history=None, logit_bias=None, allowed_token_ids=None, banned_token_ids=None, min_p=0.0):
        """GPT.sample (src/main.zig:198-207) with reproducible uniforms; returns tokens [batch] (and probs).  top_k / top_p:
        truncation in front of the draw (zg_sample_options; the defaults are off and take zg_gpt_sample itself).
        repetition_penalty / presence_penalty / frequency_penalty: zg_logit_penalties on the tokens of `history` (one list per row),
        applied to the raw logits first (zg_gpt_sample_pen; the defaults are off and take today's call).  logit_bias ({id: value}) /
        allowed_token_ids / banned_token_ids: edits of the row behind the penalties; min_p: the sampler's min-p truncation
        (zg_logit_edits; zg_gpt_sample_edit; the defaults are off and take today's call)."""
        tokens = np.ascontiguousarray(np.atleast_1d(tokens), dtype=np.uint64)
        u = None if uniforms is None else np.ascontiguousarray(np.atleast_1d(uniforms), dtype=np.float32)
        out = np.zeros(self.batch, np.uint64)
        probs = np.empty((self.batch, self.config.vocab_size), np.float32) if want_probs else None
        pen = self._penalties(repetition_penalty, presence_penalty, frequency_penalty)
        edits = self._edits(logit_bias, allowed_token_ids, banned_token_ids, min_p)
        if edits is not None:
            opt = _lib.SampleOptions(temp, top_k, top_p)
            hp, hstride, hlens, keep = self._token_lists((history if history is not None else [None] * self.batch) if pen is not None else None)
            check(self._L.zg_gpt_sample_edit(self.h, seq_len, ptr(tokens), tokens.size, C.addressof(opt), None if pen is None else C.addressof(pen), hp, hstride,
                                             hlens, C.addressof(edits[0]), ptr(u), seed, ptr(out), ptr(probs), ops._n(probs)))
            del keep
            return (out, probs) if want_probs else out
        if pen is not None:
            opt = _lib.SampleOptions(temp, top_k, top_p)
            hp, hstride, hlens, keep = self._token_lists(history if history is not None else [None] * self.batch)
            check(self._L.zg_gpt_sample_pen(self.h, seq_len, ptr(tokens), tokens.size, C.addressof(opt), C.addressof(pen), hp, hstride, hlens, ptr(u), seed,
                                            ptr(out), ptr(probs), ops._n(probs)))
            del keep
            return (out, probs) if want_probs else out
        self._sampled("sample", "", (seq_len, ptr(tokens), tokens.size), temp, top_k, top_p, (ptr(u), seed, ptr(out), ptr(probs), ops._n(probs)))
        return (out, probs) if want_probs else out

    def argmax(self):
        out = np.zeros(self.batch, np.uint64)
        check(self._L.zg_gpt_argmax(self.h, ptr(out), out.size))
        return out

    def hidden(self):
        x = np.empty((self.batch, self.config.n_embed), np.float32)
        check(self._L.zg_gpt_hidden(self.h, ptr(x), x.size))
        return x

    # ------------------------------------------------------------------ generate
    def _prompts(self, prompts):
        return _pack_prompts(prompts, self.batch)

    def generate(self, prompts, n_steps, logprobs=None, stop_token_ids=None, stop=None, lookahead=0):
        """generate (src/main.zig:322-342), greedy; returns tokens [batch, n_steps].  logprobs=top_n (an int, 0 .. 20): the same
        tokens with the log-probability of every pick and its top_n alternatives — returns (tokens, logprobs,
        top_ids, top_logprobs) as generate_fetch_logprobs gives them.  stop_token_ids (token ids) / stop (a list of token-id lists):
        the generation ends soon after every row has picked a stop token or completed a stop sequence, and what is
        returned is cut at its end: columns 0 .. end - 1, the same tokens as without the conditions; `stop_result()` tells where
        every row finished.  lookahead: steps the host may run ahead of the device (0: the default)."""
        if stop_token_ids is not None or stop is not None:
            return self._generate_stop(None, prompts, n_steps, None, 0, 0, 1.0, None, None, logprobs, stop_token_ids, stop, lookahead)
        return self._generate(None, prompts, n_steps, None, 0, 0, 1.0, None, None, logprobs)

    def generate_enqueue(self, prompts, n_steps):
        self._generate(None, prompts, n_steps, None, 0, 0, 1.0, None, None, None, fetch=False)

    def generate_fetch(self, n_steps):
        out = np.zeros((self.batch, n_steps), np.uint64)
        check(self._L.zg_gpt_generate_fetch(self.h, n_steps, ptr(out), out.size))
        return out

    def generate_fetch_range(self, first, n):
        """Tokens of positions first .. first + n - 1 of the last generation(s): [batch, n]."""
        out = np.zeros((self.batch, n), np.uint64)
        check(self._L.zg_gpt_generate_fetch_range(self.h, first, n, ptr(out), out.size))
        return out

    # ------------------------------------------------------------------ cache forks and beam search
    def fork_rows(self, src):
        """zg_gpt_kv_fork: row b's KV caches over the cached positions become those of row src[b] (src[b] == b: untouched).  Enqueued
        on the handle's stream; every source must be its own source."""
        src = np.ascontiguousarray(np.atleast_1d(src), dtype=np.uint64)
        check(self._L.zg_gpt_kv_fork(self.h, ptr(src), src.size))

    def kv_rows(self, layer, which, row, first_pos, n_pos):
        """zg_debug_gpt_kv_rows: the raw bytes (uint8) of positions first_pos .. first_pos + n_pos - 1 of one row of layer `layer`'s
        K (which 0) or V (which 1) cache, [n_heads][n_pos][64] elements, a 24-bit cache's byte plane behind its bf16 plane."""
        out = np.zeros(self.config.n_heads * n_pos * 64 * self._kv_bytes, np.uint8)
        check(self._L.zg_debug_gpt_kv_rows(self.h, layer, which, row, first_pos, n_pos, ptr(out), out.size))
        return out

    def beam_search_enqueue(self, prompts, n_steps, num_beams, eos_token_id=None, length_penalty=1.0, early_stopping=True, past_len=0, lookahead=0):
        """zg_gpt_generate_beam_enqueue: `prompts` holds one prompt per group (batch // num_beams of them) or one per row."""
        prompts = list(prompts)
        if len(prompts) * num_beams == self.batch and num_beams > 1:
            prompts = [p for p in prompts for _ in range(num_beams)]
        mat, lens, stride = self._prompts(prompts)
        req = _lib.generate_request(past_len=past_len, prompts=ptr(mat), prompt_stride=stride, prompt_lens=ptr(lens), n_steps=n_steps)
        opt = _lib.beam_options(num_beams, eos_token_id, length_penalty, early_stopping, lookahead)
        check(self._L.zg_gpt_generate_beam_enqueue(self.h, C.addressof(req), C.addressof(opt)))
        self._beam_width = int(num_beams)

    def generate_fetch_beams(self, num_return_sequences, max_len=None):
        """zg_gpt_generate_fetch_beams: per group a list of (tokens uint64 array, score, sum_logprob), best first."""
        n, stride = int(num_return_sequences), int(max_len or self.config.context_size)
        tok = np.zeros((self.batch, n, stride), np.uint64)  # (at least [G][n][stride])
        lens = np.zeros((self.batch, n), np.uint64)
        scores, sums = np.zeros((self.batch, n), np.float32), np.zeros((self.batch, n), np.float32)
        check(self._L.zg_gpt_generate_fetch_beams(self.h, n, ptr(tok), stride, ptr(lens), ptr(scores), ptr(sums)))
        G = self.batch // self._beam_width
        return [[(tok[g, i, : int(lens[g, i])].copy(), scores[g, i], sums[g, i]) for i in range(n) if lens[g, i] > 0] for g in range(G)]

    def generate_fetch_beam_trace(self, first, n):
        """zg_gpt_generate_fetch_beam_trace of columns first .. first + n - 1: (parents [batch, n] int32, scores [batch, n] float32),
        indexed by the slot after each step."""
        par = np.zeros((self.batch, n), np.int32)
        sc = np.zeros((self.batch, n), np.float32)
        check(self._L.zg_gpt_generate_fetch_beam_trace(self.h, first, n, ptr(par), ptr(sc), par.size))
        return par, sc

    def beam_search(self, prompts, n_steps, num_beams, eos_token_id=None, length_penalty=1.0, early_stopping=True, num_return_sequences=1, past_len=0,
                    lookahead=0):
        """Beam search in the device loop (HF generate(num_beams=...)): the handle's batch is batch // num_beams groups
        of num_beams beams, `prompts` one prompt per group.  Returns per group a list of (tokens, score, sum_logprob), best first:
        the picked tokens only (eos last where there is one), score = sum_logprob / len ** length_penalty."""
        self.beam_search_enqueue(prompts, n_steps, num_beams, eos_token_id, length_penalty, early_stopping, past_len, lookahead)
        return self.generate_fetch_beams(num_return_sequences)

    def generate_from(self, past_len, prompts, n_steps, temp=None, seed=0, top_k=0, top_p=1.0, repetition_penalty=1.0, presence_penalty=0.0,
                      frequency_penalty=0.0, prior=None, logprobs=None, stop_token_ids=None, stop=None, lookahead=0, logit_bias=None,
                      allowed_token_ids=None, banned_token_ids=None, min_p=0.0, guide_states=None, no_repeat_ngram_size=0, bad_words_ids=None,
                      min_tokens=0, suppress_token_ids=None):
        """generate entered at position past_len (zg_gpt_generate_from_enqueue): `prompts` are the new tokens of each row, fed
        behind the past_len cached positions; returns the tokens of positions past_len .. past_len + n_steps - 1 ([batch, n_steps]).
        temp=None: greedy; otherwise the sampler of generate_sample (top_k / top_p as there).  Penalties as generate_sample; the
        tokens below past_len count only when passed as `prior` (one list per row).  logprobs=top_n: as `generate`, for the
        columns past_len .. past_len + n_steps - 1.  stop_token_ids / stop / lookahead: as `generate`; the columns are absolute and
        what is returned is columns past_len .. end - 1.  logit_bias / allowed_token_ids / banned_token_ids / min_p: as `sample`.
        guide_states: as `generate_sample`; a second turn passes the states `generate_fetch_guide_states` and the tokens lead to.
        no_repeat_ngram_size / bad_words_ids / min_tokens / suppress_token_ids: as `generate_sample`; the history they read is `prior`
        followed by the new tokens and the picks — an n-gram or a bad word may straddle all three."""
        pen = self._penalties(repetition_penalty, presence_penalty, frequency_penalty)
        edits = self._edits(logit_bias, allowed_token_ids, banned_token_ids, min_p)
        bans = self._bans(no_repeat_ngram_size, bad_words_ids, min_tokens, suppress_token_ids, stop_token_ids)
        if stop_token_ids is not None or stop is not None:
            return self._generate_stop(past_len, prompts, n_steps, temp, seed, top_k, top_p, pen, prior, logprobs, stop_token_ids, stop, lookahead, edits,
                                       guide_states, bans)
        return self._generate(past_len, prompts, n_steps, temp, seed, top_k, top_p, pen, prior, logprobs, edits=edits, guide_states=guide_states, bans=bans)

    def generate_sample(self, prompts, n_steps, temp, seed=0, top_k=0, top_p=1.0, repetition_penalty=1.0, presence_penalty=0.0,
                        frequency_penalty=0.0, prior=None, logprobs=None, stop_token_ids=None, stop=None, lookahead=0, logit_bias=None,
                        allowed_token_ids=None, banned_token_ids=None, min_p=0.0, guide_states=None, no_repeat_ngram_size=0, bad_words_ids=None,
                        min_tokens=0, suppress_token_ids=None):
        """generate (src/main.zig:322-342) as the reference runs it — every token behind the prompt drawn by GPT.sample — with the
        loop on the device; the tokens of the host loop over `sample(T, tok, temp, seed=seed)`.  top_k / top_p: as `sample`.
        repetition_penalty / presence_penalty / frequency_penalty: on the tokens the row holds when a pick is drawn — `prior` (one
        list per row, optional) followed by the row's prompt and picks so far (zg_gpt_generate_pen_enqueue; defaults: today's call).
        logprobs=top_n: as `generate` — of the row the sampler received, at temperature 1 and before truncation.
        stop_token_ids / stop / lookahead: as `generate`.  logit_bias ({id: value}) / allowed_token_ids / banned_token_ids: edits of
        every step's row behind the penalties; min_p: min-p truncation (defaults: today's call).
        guide_states (a `guided` handle with a guide loaded): one start state of the loaded automaton per row, None for
        a row without a guide — every pick of a guided row is one its state allows, and the state follows the picks on the device.
        History-dependent bans, computed on the device at every step (zg_gpt_generate_banned_enqueue; defaults: today's
        call): no_repeat_ngram_size=n — no n-gram occurs twice in `prior` + prompt + picks (HF); bad_words_ids — token-id lists, the last
        token of a word is forbidden while the row ends in its first tokens (vLLM bad_words / HF bad_words_ids; the match may reach
        into the prompt); min_tokens — suppress_token_ids (default: stop_token_ids) cannot be picked until a row has that many picks.
        `bans.banned_now` is the host twin for callers who draw token by token."""
        pen = self._penalties(repetition_penalty, presence_penalty, frequency_penalty)
        edits = self._edits(logit_bias, allowed_token_ids, banned_token_ids, min_p)
        bans = self._bans(no_repeat_ngram_size, bad_words_ids, min_tokens, suppress_token_ids, stop_token_ids)
        if stop_token_ids is not None or stop is not None:
            return self._generate_stop(None, prompts, n_steps, temp, seed, top_k, top_p, pen, prior, logprobs, stop_token_ids, stop, lookahead, edits,
                                       guide_states, bans)
        return self._generate(None, prompts, n_steps, temp, seed, top_k, top_p, pen, prior, logprobs, edits=edits, guide_states=guide_states, bans=bans)

    def generate_sample_enqueue(self, prompts, n_steps, temp, seed=0, top_k=0, top_p=1.0, repetition_penalty=1.0, presence_penalty=0.0,
                                frequency_penalty=0.0, prior=None, logprobs=None, logit_bias=None, allowed_token_ids=None, banned_token_ids=None,
                                min_p=0.0, no_repeat_ngram_size=0, bad_words_ids=None, min_tokens=0, suppress_token_ids=None):
        """generate_sample without the fetch; results through generate_fetch and (logprobs=top_n) generate_fetch_logprobs."""
        pen = self._penalties(repetition_penalty, presence_penalty, frequency_penalty)
        edits = self._edits(logit_bias, allowed_token_ids, banned_token_ids, min_p)
        bans = self._bans(no_repeat_ngram_size, bad_words_ids, min_tokens, suppress_token_ids)
        self._generate(None, prompts, n_steps, temp, seed, top_k, top_p, pen, prior, logprobs, fetch=False, edits=edits, bans=bans)

    # ------------------------------------------------------------------ per-row sampling parameters
    def generate_each(self, prompts, n_steps, rows, past_len=0, prior=None, logprobs=None, stop_token_ids=None, stop=None, lookahead=0,
                      logit_bias=None, allowed_token_ids=None, banned_token_ids=None, guide_states=None, bad_words_ids=None, suppress_token_ids=None):
        """generate_sample / generate_from with the sampler parameters taken per row (zg_gpt_generate_each_enqueue): `rows` is one
        dict per row with generate_sample's keyword names — temp, top_k, top_p, min_p, repetition_penalty, presence_penalty,
        frequency_penalty — plus seed; a row's temp 0 / None is greedy (temp 1, top_k 1).  Row b gets, bit for bit, what
        generate_sample with rows[b]'s values for every row gives row b.  prior, logprobs, the stop conditions and the three edit
        lists are per call and work as there; returns what generate_from returns: columns past_len .. (end or past_len + n_steps) - 1.
        guide_states: as `generate_sample` (zg_gpt_generate_guided_enqueue with the table).
        A row's dict may also carry no_repeat_ngram_size and min_tokens; bad_words_ids and suppress_token_ids (default:
        stop_token_ids) are per call (zg_gpt_generate_banned_enqueue with the table)."""
        ban_keys = ("no_repeat_ngram_size", "min_tokens")
        bans = self._bans([int(r.get("no_repeat_ngram_size", 0)) for r in rows], bad_words_ids, [int(r.get("min_tokens", 0)) for r in rows],
                          suppress_token_ids, stop_token_ids) if len(rows) == self.batch else None
        if bans is not None and guide_states is not None:
            raise ValueError("ban rules and a guide cannot be combined: a grammar compiles its bad words into the table")
        rows = [{k: v for k, v in r.items() if k not in ban_keys} for r in rows]
        table = _lib.row_sampling(rows)
        mat, lens, stride = self._prompts(prompts)
        edits = self._edits(logit_bias, allowed_token_ids, banned_token_ids, 0.0)
        have_stop = stop_token_ids is not None or stop is not None
        conds, keep_conds = _lib.stop_conditions(stop_token_ids, stop, lookahead) if have_stop else (None, ())
        pp, pstride, plens, keep = self._token_lists(prior)
        r = _lib.generate_request(past_len=past_len, prompts=ptr(mat), prompt_stride=stride, prompt_lens=ptr(lens), n_steps=n_steps, prior=pp,
                                  prior_stride=pstride, prior_lens=plens, logprobs=int(logprobs is not None), top_n=int(logprobs or 0),
                                  stop=None if conds is None else C.addressof(conds), edits=None if edits is None else C.addressof(edits[0]))
        if bans is not None:
            check(self._L.zg_gpt_generate_banned_enqueue(self.h, C.addressof(r), C.addressof(table), len(rows), C.addressof(bans[0])))
        elif guide_states is None:
            check(self._L.zg_gpt_generate_each_enqueue(self.h, C.addressof(r), C.addressof(table), len(rows)))
        else:
            states = self._guide_states(guide_states)
            check(self._L.zg_gpt_generate_guided_enqueue(self.h, C.addressof(r), C.addressof(table), len(rows), ptr(states)))
        del keep, keep_conds
        n = self.stop_result()[0] - past_len if conds is not None and (conds.n_ids or conds.n_seqs) else n_steps
        out = self.generate_fetch_range(past_len, n)
        return out if logprobs is None else (out,) + self.generate_fetch_logprobs(past_len, n, logprobs)

    def sample_each(self, seq_len, tokens, rows, uniforms=None, history=None, want_probs=False, logit_bias=None, allowed_token_ids=None,
                    banned_token_ids=None):
        """`sample` with the sampler parameters taken per row (zg_gpt_sample_each; `rows` as generate_each).  uniforms None: the
        draw of row b is the counter PRNG of (rows[b]'s seed, seq_len, b).  history: one token list per row, read when any row is
        penalised.  Returns tokens [batch] (and probs)."""
        table = _lib.row_sampling(rows)
        tokens = np.ascontiguousarray(np.atleast_1d(tokens), dtype=np.uint64)
        u = None if uniforms is None else np.ascontiguousarray(np.atleast_1d(uniforms), dtype=np.float32)
        out = np.zeros(self.batch, np.uint64)
        probs = np.empty((self.batch, self.config.vocab_size), np.float32) if want_probs else None
        edits = self._edits(logit_bias, allowed_token_ids, banned_token_ids, 0.0)
        hp, hstride, hlens, keep = self._token_lists(history)
        check(self._L.zg_gpt_sample_each(self.h, seq_len, ptr(tokens), tokens.size, C.addressof(table), len(rows), hp, hstride, hlens,
                                         None if edits is None else C.addressof(edits[0]), ptr(u), ptr(out), ptr(probs), ops._n(probs)))
        del keep
        return (out, probs) if want_probs else out

    PROFILE_CLASSES = ["embed", "ln1_c_attn_kv", "attention", "merge_attn_proj_resid", "ln2_c_fc_gelu",
                       "mlp_proj_resid", "lnf_lm_head_argmax", "step_total"]

    def profile_step(self, seq_len, iters):
        """Average microseconds per kernel class of one eager decode step (zg_gpt_profile_step)."""
        out = np.zeros(9, np.float32)
        check(self._L.zg_gpt_profile_step(self.h, seq_len, iters, out.ctypes.data_as(_lib.f32p), out.size))
        return dict(zip(self.PROFILE_CLASSES + ["null_kernel_interval"], (float(v) for v in out)))

    def prefetch_stats(self):
        """zg_debug_prefetch_stats: {"on", "workgroups", "exit", "jobs"} (lists per XCD) of the last generate call."""
        out = np.zeros(25 + 256, np.uint32)
        check(self._L.zg_debug_prefetch_stats(self.h, out.ctypes.data_as(C.c_void_p), out.size))
        return {"on": bool(out[0]), "stalled": int(out[0]) == 2, "workgroups": out[1:9].tolist(), "exit": out[9:17].tolist(), "jobs": out[17:25].tolist(),
                "xcd_of_block0": [int(v) & 15 for v in out[25:] if v & 0x100]}

    def time_kernel(self, which, iters, walk_layers=False, at=0):
        """walk_layers: launch i of the chain takes layer i mod n_layer (weights / KV from the memory side, as in the real step);
        at: the sequence length the chain runs at (0: mid-context).  ZG_TIME_WALK_LAYERS / ZG_TIME_AT of include/zgpt2.h."""
        us, nbytes = C.c_float(), C.c_size_t()
        check(self._L.zg_gpt_time_kernel(self.h, which | (0x100 if walk_layers else 0) | (int(at) << 16), iters, C.byref(us), C.byref(nbytes)))
        return us.value, nbytes.value


class GPTGroups:
    """`n_prompts` independent prompts on ONE GPU as `groups` handles of n_prompts / groups sequences each, every handle on
    its own stream, all reading one weight region (zg_gpt_create_ex) — the embarrassingly parallel case of the reference's
    generate loop (src/main.zig:322-342) with the batch == 1 restriction of src/ops.zig:126-128 lifted by running chains side
    by side instead of in lock step.  groups == 1 is a plain GPT of batch n_prompts.  Tokens equal GPT's row for row."""

    # priorities dealt to the groups' streams: streams of different priorities never share a hardware queue
    PRIORITIES = (0, 1, -1)

    def __init__(self, config: GPTConfig, n_prompts, groups, priorities=None, **kw):
        assert groups >= 1 and n_prompts % groups == 0, (n_prompts, groups)
        self.config, self.n_prompts, self.groups = config, n_prompts, groups
        self._L = _lib.load()
        per = n_prompts // groups
        # default: priorities dealt in turn up to four groups (three distinct hardware queues: 452 against 667 us per step round at
        # 4 x 2), all alike beyond that (eight streams over three priority levels serialise completely: 2.1 ms against 0.94 at 8 x 1;
        # profiles/round6_corun_ab_final.jsonl)
        if priorities is not None:
            pr = priorities
        elif groups <= 4:
            pr = [self.PRIORITIES[i % len(self.PRIORITIES)] for i in range(groups)]
        else:
            pr = [0] * groups
        self.members = []
        for i in range(groups):
            self.members.append(GPT(config, batch=per, share_weights_with=self.members[0] if i else None,
                                    own_stream=groups > 1, stream_priority=pr[i], **kw))
        self._harr = (C.c_void_p * groups)(*[m.h for m in self.members])

    @property
    def batch(self):
        return self.n_prompts

    def close(self):
        for m in reversed(getattr(self, "members", [])):  # the weight owner last
            m.close()
        self.members = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_weights(self, weights):
        self.members[0].load_weights(weights)

    def generate_enqueue(self, prompts, n_steps):
        mat, lens, stride = _pack_prompts(prompts, self.n_prompts)
        check(self._L.zg_gpt_generate_enqueue_many(self._harr, self.groups, ptr(mat), stride, ptr(lens), n_steps))

    def generate_fetch(self, n_steps):
        out = np.zeros((self.n_prompts, n_steps), np.uint64)
        check(self._L.zg_gpt_generate_fetch_many(self._harr, self.groups, n_steps, ptr(out), out.size))
        return out

    def generate(self, prompts, n_steps):
        self.generate_enqueue(prompts, n_steps)
        return self.generate_fetch(n_steps)

    def synchronize(self):
        """Drain every member's stream (hipStreamSynchronize through zg_gpt_hidden's drain would copy; use the streams)."""
        import torch

        for m in self.members:
            s = C.c_void_p()
            check(self._L.zg_gpt_stream(m.h, C.byref(s)))
            torch.cuda.ExternalStream(s.value).synchronize()


# --------------------------------------------------------------------------------------------
# Op-tier composition: src/main.zig written against ops.py the way it is written against ops.zig.
# --------------------------------------------------------------------------------------------
class State:
    """State (src/main.zig:26-65): every buffer allocated once, by the caller."""

    def __init__(self, config: GPTConfig, alloc=None):
        z = alloc or (lambda n: np.zeros(n, np.float32))
        e, c = config.n_embed, config.context_size
        self.pos_emb, self.x, self.o = z(e), z(e), z(e)
        self.logits = z(config.vocab_size)
        self._h, self._4xh, self._qkv, self._q = z(e), z(4 * e), z(3 * e), z(e)
        self._k, self._v, self._attn = z(c * e), z(c * e), z(c)


class HostGPT:
    """GPT/Block/MLP of src/main.zig:67-208 over the op tier, with host (numpy) buffers."""

    def __init__(self, config: GPTConfig, weights):
        self.config = config
        e = config.n_embed
        w = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in weights.items()}
        self.w = w
        self.wte = ops.Embedding(e, w["wte"])
        self.wpe = ops.Embedding(e, w["wpe"])
        self.ln_f = ops.LayerNorm(e, w["ln_f_g"], w["ln_f_b"])
        self.lm_head = ops.Linear(e, config.vocab_size, w["wte"], None)  # main.zig:312
        self.h = []
        for l in range(config.n_layer):
            g = lambda n: w[f"h{l}.{n}"]  # noqa: E731
            blk = dict(
                ln_1=ops.LayerNorm(e, g("ln_1_g"), g("ln_1_b")),
                attn=ops.CausalSelfAttention(config.n_heads, e, ops.Linear(e, 3 * e, g("c_attn_w"), g("c_attn_b")),
                                             ops.Linear(e, e, g("c_proj_w"), g("c_proj_b"))),
                ln_2=ops.LayerNorm(e, g("ln_2_g"), g("ln_2_b")),
                c_fc=ops.Linear(e, 4 * e, g("c_fc_w"), g("c_fc_b")),
                c_proj=ops.Linear(4 * e, e, g("mlp_proj_w"), g("mlp_proj_b")),
                k_cache=np.zeros(config.context_size * e, np.float32),  # main.zig:298-299
                v_cache=np.zeros(config.context_size * e, np.float32),
            )
            self.h.append(blk)
        self.state = State(config)

    def _block_forward(self, blk, seq_len, inputs, st):  # main.zig:119-146
        e = self.config.n_embed
        st._h[:] = inputs
        blk["ln_1"].forward(st._h)
        blk["attn"].forward(seq_len, st._h, blk["k_cache"][: seq_len * e], blk["v_cache"][: seq_len * e], st.o,
                            st._qkv, st._q, st._k[: seq_len * e], st._v[: seq_len * e], st._attn[:seq_len])
        st._h[:] = st.o + inputs
        st.x[:] = st._h
        blk["ln_2"].forward(st._h)
        blk["c_fc"].forward(st._h, st._4xh)  # MLP.forward, main.zig:78-82
        ops.gelu(st._4xh)
        blk["c_proj"].forward(st._4xh, st.o)
        st.o += st.x
        st.x[:] = st.o

    def forward(self, seq_len, token, compute_logits=True):  # main.zig:178-195
        st = self.state
        self.wpe.forward(np.array([seq_len - 1], np.uint64), st.pos_emb)
        self.wte.forward(np.array([token], np.uint64), st.x)
        st.x += st.pos_emb
        for blk in self.h:
            self._block_forward(blk, seq_len, st.x.copy(), st)
        self.ln_f.forward(st.x)
        if compute_logits:
            self.lm_head.forward(st.x, st.logits)
            return st.logits.copy()
        return None
