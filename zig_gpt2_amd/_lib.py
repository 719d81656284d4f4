"""ctypes binding of libzgpt2_hip.so (the C ABI of include/zgpt2.h).

There is no fallback: if the HIP library is missing, load() raises.  build() compiles it in-tree
with hipcc for gfx950 (zig_gpt2_amd/csrc/Makefile), so the .so travels with the repo snapshot.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.environ.get("ZGPT2_LIB") or os.path.join(_HERE, "lib", "libzgpt2_hip.so")  # ZGPT2_LIB: diagnostic builds
HEADER = os.path.join(os.path.dirname(_HERE), "include", "zgpt2.h")

_lib = None

f32p = C.POINTER(C.c_float)
szp = C.POINTER(C.c_size_t)
vp = C.c_void_p
sz = C.c_size_t


class ZgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libzgpt2_hip error {code}: {msg}")
        self.code = code


class GptConfig(C.Structure):
    """zg_gpt_config == GPTConfig of src/main.zig:5-23."""

    _fields_ = [("vocab_size", sz), ("context_size", sz), ("n_layer", sz), ("n_heads", sz), ("n_embed", sz)]


class SampleOptions(C.Structure):
    """zg_sample_options of include/zgpt2.h."""

    _fields_ = [("temp", C.c_float), ("top_k", sz), ("top_p", C.c_float)]


class LogitPenalties(C.Structure):
    """zg_logit_penalties of include/zgpt2.h."""

    _fields_ = [("repetition", C.c_float), ("presence", C.c_float), ("frequency", C.c_float)]


class StopConditions(C.Structure):
    """zg_stop_conditions of include/zgpt2.h."""

    _fields_ = [("ids", vp), ("n_ids", sz), ("seqs", vp), ("seq_stride", sz), ("seq_lens", vp), ("n_seqs", sz), ("lookahead", sz)]


class LogitEdits(C.Structure):
    """zg_logit_edits of include/zgpt2.h."""

    _fields_ = [("bias_ids", vp), ("bias_values", vp), ("n_bias", sz), ("allowed_ids", vp), ("n_allowed", sz), ("banned_ids", vp), ("n_banned", sz),
                ("min_p", C.c_float)]


class RowSampling(C.Structure):
    """zg_row_sampling of include/zgpt2.h."""

    _fields_ = [("options", SampleOptions), ("min_p", C.c_float), ("penalties", LogitPenalties), ("seed", C.c_uint64)]


def row_sampling(rows):
    """An array of zg_row_sampling from a list of dicts with generate_sample's keyword names (temp, top_k, top_p, min_p,
    repetition_penalty, presence_penalty, frequency_penalty) plus seed.  A row's temp 0 / None is greedy: {temp 1, top_k 1}."""
    arr = (RowSampling * max(len(rows), 1))()
    known = {"temp", "top_k", "top_p", "min_p", "repetition_penalty", "presence_penalty", "frequency_penalty", "seed"}
    for b, r in enumerate(rows):
        if set(r) - known:
            raise TypeError(f"row {b}: unknown sampling parameter(s) {sorted(set(r) - known)}")
        temp, top_k = r.get("temp", 1.0), int(r.get("top_k", 0))
        if temp is None or float(temp) == 0.0:
            temp, top_k = 1.0, 1
        arr[b] = RowSampling(SampleOptions(float(temp), top_k, float(r.get("top_p", 1.0))), float(r.get("min_p", 0.0)),
                             LogitPenalties(float(r.get("repetition_penalty", 1.0)), float(r.get("presence_penalty", 0.0)),
                                            float(r.get("frequency_penalty", 0.0))), int(r.get("seed", 0)))
    return arr


class Guide(C.Structure):
    """zg_guide of include/zgpt2.h."""

    _fields_ = [("n_states", sz), ("next", vp)]


class BanRules(C.Structure):
    """zg_ban_rules of include/zgpt2.h (`size` is filled by ban_rules())."""

    _fields_ = [("size", sz), ("no_repeat_ngram", vp), ("words", vp), ("word_stride", sz), ("word_lens", vp), ("n_words", sz), ("suppress_ids", vp),
                ("n_suppress", sz), ("min_tokens", vp)]


class GenerateRequest(C.Structure):
    """zg_generate_request of include/zgpt2.h (`size` is filled by generate_request())."""

    _fields_ = [("size", sz), ("past_len", sz), ("prompts", vp), ("prompt_stride", sz), ("prompt_lens", vp), ("n_steps", sz), ("options", vp),
                ("penalties", vp), ("prior", vp), ("prior_stride", sz), ("prior_lens", vp), ("seed", C.c_uint64), ("logprobs", C.c_int), ("top_n", sz),
                ("stop", vp), ("edits", vp)]


def generate_request(**fields):
    """A zg_generate_request with its size set and every field not named left 0 / NULL."""
    r = GenerateRequest(**fields)
    r.size = C.sizeof(GenerateRequest)
    return r


class BeamOptions(C.Structure):
    """zg_beam_options of include/zgpt2.h (`size` is filled by beam_options())."""

    _fields_ = [("size", sz), ("num_beams", sz), ("eos_id", sz), ("length_penalty", C.c_float), ("early_stopping", C.c_int), ("lookahead", sz)]


def beam_options(num_beams, eos_token_id=None, length_penalty=1.0, early_stopping=True, lookahead=0):
    """A zg_beam_options with its size set; eos_token_id None: ZG_BEAM_NO_EOS."""
    return BeamOptions(C.sizeof(BeamOptions), int(num_beams), BEAM_NO_EOS if eos_token_id is None else int(eos_token_id), float(length_penalty),
                       int(bool(early_stopping)), int(lookahead))


class GptOptions(C.Structure):
    """zg_gpt_options of include/zgpt2.h."""

    _fields_ = [("share_weights_with", vp), ("own_stream", C.c_int), ("stream_priority", C.c_int)]


class TapEntry(C.Structure):
    """zg_tap_entry of include/zgpt2.h."""

    _fields_ = [("cls", C.c_int), ("layer", C.c_int), ("buffer", C.c_int), ("type", C.c_int), ("offset", sz), ("count", sz),
                ("flags", C.c_uint), ("pad", C.c_uint)]


# name -> (restype, argtypes); every symbol include/zgpt2.h declares
SIGNATURES = {
    "zg_init": (C.c_int, [C.c_int]),
    "zg_init_ex": (C.c_int, [C.c_int, sz]),
    "zg_shutdown": (C.c_int, []),
    "zg_last_error": (C.c_char_p, []),
    "zg_set_stream": (C.c_int, [vp]),
    "zg_synchronize": (C.c_int, []),
    "zg_register_tensor": (C.c_int, [vp, sz]),
    "zg_unregister_tensor": (C.c_int, [vp]),
    "zg_unregister_all": (C.c_int, []),
    "zg_debug_gemm_launches": (C.c_ulonglong, []),
    "zg_debug_gemm_stamps": (C.c_int, [vp, sz]),
    "zg_debug_ops_set_done_seq": (C.c_int, [C.c_uint]),
    "zg_debug_ops_done_state": (C.c_int, [vp, sz]),
    "zg_debug_last_kernel": (C.c_int, [C.c_char_p, sz]),
    "zg_debug_gemv_plan": (C.c_int, [C.c_int] * 6 + [C.c_uint, C.c_int, C.c_int, vp, sz]),
    "zg_debug_attn_prefill": (C.c_int, [vp, vp, sz, sz, sz, sz, vp, vp, sz, vp, sz, C.c_int]),
    "zg_debug_attn_prefill_at": (C.c_int, [vp, vp, sz, sz, sz, sz, sz, vp, vp, C.c_int, sz, vp, sz, C.c_int]),
    "zg_debug_prefill_route": (C.c_int, [C.c_int, C.c_int]),
    "zg_debug_prefill_plan": (C.c_int, [C.c_int] * 6 + [sz, C.c_uint, sz, C.c_uint, C.c_int, C.c_int, vp, sz]),
    "zg_debug_prefill_linear": (C.c_int, [vp, vp, vp, vp, sz, sz, sz, C.c_int, C.c_int, C.c_int, vp, sz]),
    "zg_linear_forward": (C.c_int, [sz, sz, vp, vp, vp, sz, vp, sz]),
    "zg_embedding_forward": (C.c_int, [sz, vp, sz, vp, sz, vp, sz]),
    "zg_layernorm_forward": (C.c_int, [sz, vp, vp, C.c_float, vp, sz]),
    "zg_attn_forward": (C.c_int, [sz, sz, vp, vp, vp, vp, sz, vp, sz] + [vp, sz] * 8),
    "zg_split_qkv": (C.c_int, [sz, sz, vp, sz, sz, vp, sz]),
    "zg_transpose": (C.c_int, [sz, sz, sz, vp, sz, vp, sz]),
    "zg_scaled_dot_product_attention": (C.c_int, [vp, sz, vp, sz, vp, sz, sz, sz, sz, vp, sz, vp, sz]),
    "zg_gemm_bf16_nt": (C.c_int, [vp, vp, vp, vp, sz, sz, sz, C.c_int, C.c_int]),
    "zg_f32_to_bf16": (C.c_int, [vp, vp, sz]),
    "zg_gelu": (C.c_int, [vp, sz]),
    "zg_softmax": (C.c_int, [vp, sz]),
    "zg_gpt_create": (C.c_int, [C.POINTER(vp), C.POINTER(GptConfig), sz, C.c_uint]),
    "zg_gpt_destroy": (C.c_int, [vp]),
    "zg_gpt_create_ex": (C.c_int, [C.POINTER(vp), C.POINTER(GptConfig), sz, C.c_uint, vp]),
    "zg_gpt_stream": (C.c_int, [vp, C.POINTER(vp)]),
    "zg_gpt_generate_enqueue_many": (C.c_int, [vp, sz, vp, sz, vp, sz]),
    "zg_gpt_generate_fetch_many": (C.c_int, [vp, sz, sz, vp, sz]),
    "zg_gpt_load_block_tensor": (C.c_int, [vp, sz, C.c_int, vp, sz]),
    "zg_gpt_load_tensor": (C.c_int, [vp, C.c_int, vp, sz]),
    "zg_gpt_weight_arena": (C.c_int, [vp, C.POINTER(vp), szp]),
    "zg_dist_available": (C.c_int, []),
    "zg_dist_unique_id": (C.c_int, [vp, sz]),
    "zg_dist_init": (C.c_int, [vp, sz, C.c_int, C.c_int]),
    "zg_dist_world": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "zg_gpt_broadcast_weights": (C.c_int, [vp, C.c_int, f32p]),
    "zg_dist_allgather": (C.c_int, [vp, vp, sz]),
    "zg_dist_finalize": (C.c_int, []),
    "zg_gpt_step_bytes": (C.c_int, [vp, sz, szp, szp]),
    "zg_gpt_forward": (C.c_int, [vp, sz, vp, sz, C.c_int, vp, sz]),
    "zg_gpt_prefill": (C.c_int, [vp, vp, sz, sz, C.c_int, vp, sz]),
    "zg_gpt_cached_len": (C.c_int, [vp, szp]),
    "zg_gpt_extend": (C.c_int, [vp, sz, vp, sz, sz, C.c_int, vp, sz]),
    "zg_gpt_generate_from_enqueue": (C.c_int, [vp, sz, vp, sz, vp, sz, vp, C.c_uint64]),
    "zg_gpt_generate_fetch_range": (C.c_int, [vp, sz, sz, vp, sz]),
    "zg_gpt_argmax": (C.c_int, [vp, vp, sz]),
    "zg_debug_gpt_step_taps": (C.c_int, [vp, sz, vp, sz, vp, sz, szp, vp, sz, szp, vp, sz]),
    "zg_debug_gpt_age": (C.c_int, [vp, sz, C.c_int, C.c_uint]),
    "zg_debug_gpt_age_state": (C.c_int, [vp, vp, sz]),
    "zg_debug_gpt_tag_census": (C.c_int, [vp, C.c_uint, C.c_uint, vp, sz]),
    "zg_debug_gpt_pass_taps": (C.c_int, [vp, sz, vp, sz, sz, C.c_int, C.c_int, sz, vp, sz, vp, sz, szp, vp, sz, szp, vp, sz]),
    "zg_gpt_sample": (C.c_int, [vp, sz, vp, sz, C.c_float, vp, C.c_uint64, vp, vp, sz]),
    "zg_gpt_hidden": (C.c_int, [vp, vp, sz]),
    "zg_gpt_generate_greedy": (C.c_int, [vp, vp, sz, vp, sz, vp, sz]),
    "zg_gpt_generate_enqueue": (C.c_int, [vp, vp, sz, vp, sz]),
    "zg_gpt_generate_fetch": (C.c_int, [vp, sz, vp, sz]),
    "zg_gpt_generate_sample_enqueue": (C.c_int, [vp, vp, sz, vp, sz, C.c_float, C.c_uint64]),
    "zg_gpt_generate_sample": (C.c_int, [vp, vp, sz, vp, sz, C.c_float, C.c_uint64, vp, sz]),
    "zg_gpt_sample_ex": (C.c_int, [vp, sz, vp, sz, vp, vp, C.c_uint64, vp, vp, sz]),
    "zg_gpt_generate_sample_ex_enqueue": (C.c_int, [vp, vp, sz, vp, sz, vp, C.c_uint64]),
    "zg_gpt_generate_sample_ex": (C.c_int, [vp, vp, sz, vp, sz, vp, C.c_uint64, vp, sz]),
    "zg_debug_sample_rows": (C.c_int, [vp, sz, sz, vp, vp, vp, vp, vp]),
    "zg_gpt_sample_pen": (C.c_int, [vp, sz, vp, sz, vp, vp, vp, sz, vp, vp, C.c_uint64, vp, vp, sz]),
    "zg_gpt_generate_pen_enqueue": (C.c_int, [vp, sz, vp, sz, vp, sz, vp, vp, vp, sz, vp, C.c_uint64]),
    "zg_debug_penalize_rows": (C.c_int, [vp, sz, sz, vp, vp, sz, vp, vp, vp]),
    "zg_gpt_generate_logprobs_enqueue": (C.c_int, [vp, sz, vp, sz, vp, sz, vp, vp, vp, sz, vp, C.c_uint64, sz]),
    "zg_gpt_generate_fetch_logprobs": (C.c_int, [vp, sz, sz, sz, vp, sz, vp, vp, sz]),
    "zg_debug_logprob_rows": (C.c_int, [vp, sz, sz, vp, sz, vp, vp, vp]),
    "zg_gpt_generate_stop_enqueue": (C.c_int, [vp, sz, vp, sz, vp, sz, vp, vp, vp, sz, vp, C.c_uint64, C.c_int, sz, vp]),
    "zg_gpt_generate_stop_result": (C.c_int, [vp, szp, vp, vp]),
    "zg_debug_stop_rows": (C.c_int, [vp, sz, sz, vp, sz, vp, vp, vp, szp]),
    "zg_debug_pick_rows": (C.c_int, [vp, vp, sz, sz, sz, vp]),
    "zg_gpt_sample_edit": (C.c_int, [vp, sz, vp, sz, vp, vp, vp, sz, vp, vp, vp, C.c_uint64, vp, vp, sz]),
    "zg_gpt_generate_request_enqueue": (C.c_int, [vp, vp]),
    "zg_debug_edit_rows": (C.c_int, [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp]),
    "zg_debug_min_p_offset": (C.c_int, [C.c_float, C.c_float, f32p]),
    "zg_gpt_generate_each_enqueue": (C.c_int, [vp, vp, vp, sz]),
    "zg_gpt_sample_each": (C.c_int, [vp, sz, vp, sz, vp, sz, vp, sz, vp, vp, vp, vp, vp, sz]),
    "zg_debug_sample_rows_each": (C.c_int, [vp, sz, sz, vp, sz, vp, vp, vp, vp, vp, vp]),
    "zg_debug_penalize_rows_each": (C.c_int, [vp, sz, sz, vp, sz, vp, sz, vp, vp, vp]),
    "zg_debug_each_plan": (C.c_int, [vp, sz, sz, vp, sz]),
    "zg_gpt_guide_load": (C.c_int, [vp, vp]),
    "zg_gpt_generate_guided_enqueue": (C.c_int, [vp, vp, vp, sz, vp]),
    "zg_gpt_generate_fetch_guide_states": (C.c_int, [vp, sz, sz, vp, sz]),
    "zg_debug_guide_rows": (C.c_int, [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp]),
    "zg_debug_guide_check": (C.c_int, [vp, sz, vp, vp, sz, C.c_int]),
    "zg_gpt_generate_banned_enqueue": (C.c_int, [vp, vp, vp, sz, vp]),
    "zg_debug_ban_check": (C.c_int, [vp, sz, sz, sz, vp, sz, vp, C.c_int, C.c_int]),
    "zg_debug_ban_rows": (C.c_int, [vp, sz, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp]),
    "zg_gpt_kv_fork": (C.c_int, [vp, vp, sz]),
    "zg_debug_gpt_kv_rows": (C.c_int, [vp, sz, C.c_int, sz, sz, sz, vp, sz]),
    "zg_gpt_generate_beam_enqueue": (C.c_int, [vp, vp, vp]),
    "zg_gpt_generate_fetch_beams": (C.c_int, [vp, sz, vp, sz, vp, vp, vp]),
    "zg_gpt_generate_fetch_beam_trace": (C.c_int, [vp, sz, sz, vp, vp, sz]),
    "zg_debug_beam_check": (C.c_int, [vp, vp, sz, sz, sz, sz]),
    "zg_debug_beam_rows": (C.c_int, [vp, vp, sz, sz, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, szp]),
    "zg_gpt_score": (C.c_int, [vp, sz, vp, sz, sz, sz, vp, sz]),
    "zg_debug_score_rows": (C.c_int, [vp, sz, sz, sz, vp, sz, vp, vp, vp]),
    "zg_gpt_time_kernel": (C.c_int, [vp, C.c_int, C.c_int, f32p, szp]),
    "zg_gpt_profile_step": (C.c_int, [vp, sz, C.c_int, f32p, sz]),
    "zg_debug_prefetch_stats": (C.c_int, [vp, vp, sz]),
    "zg_bpe_create": (C.c_int, [C.POINTER(vp), vp, vp, sz, vp, vp, sz]),
    "zg_bpe_destroy": (C.c_int, [vp]),
    "zg_bpe_encode": (C.c_int, [vp, C.c_char_p, sz, vp, sz, szp]),
    "zg_bpe_decode": (C.c_int, [vp, vp, sz, vp, sz, szp]),
}

# flags / slots of include/zgpt2.h
GPT_WEIGHTS_BF16, GPT_WEIGHTS_F32, GPT_NO_GRAPH, GPT_KV_F16, GPT_NO_PREFILL, GPT_PREFILL_2PLANE, GPT_NO_PREFETCH = 0, 1, 2, 4, 8, 16, 32
GPT_KV_B24 = 64
GPT_SAMPLED_GENERATE = 128
GPT_WEIGHTS_B24 = 256
GPT_TRUNCATED_GENERATE = 512
GPT_PENALIZED_GENERATE = 1024
GPT_LOGPROBS_GENERATE = 2048
GPT_SCORE = 4096
GPT_STOP_GENERATE = 8192
GPT_EDITED_GENERATE = 16384
GPT_GUIDED_GENERATE = 32768
GPT_BANNED_GENERATE = 65536
GPT_BEAM_GENERATE = 131072
BEAM_MAX, BEAM_NO_EOS = 8, (1 << 64) - 1
BAN_MAX_NGRAM, BAN_MAX_WORDS, BAN_MAX_WORD_LEN, BAN_MAX_SUPPRESS = 16, 64, 16, 16
GUIDE_MAX_STATES, GUIDE_DEAD, GUIDE_NONE = 256, 0xFFFF, (1 << 64) - 1
EDIT_MAX_BIAS = 512
LOGPROBS_TOP_MAX = 20
STOP_MAX_IDS, STOP_MAX_SEQS, STOP_MAX_SEQ_LEN = 16, 8, 16
STOP_NONE = (1 << 64) - 1


def stop_conditions(stop_token_ids=None, stop=None, lookahead=0):
    """zg_stop_conditions from a list of stop tokens and a list of stop sequences (token-id lists): (the structure, the arrays it
    points into — keep them alive while it is in use)."""
    import numpy as np

    ids = np.ascontiguousarray([] if stop_token_ids is None else stop_token_ids, dtype=np.uint64).reshape(-1)
    seqs = [np.ascontiguousarray(q, dtype=np.uint64).reshape(-1) for q in (stop or [])]
    lens = np.ascontiguousarray([len(q) for q in seqs], dtype=np.uint64)
    stride = max([len(q) for q in seqs] + [1])
    mat = np.zeros((len(seqs), stride), np.uint64)
    for k, q in enumerate(seqs):
        mat[k, : len(q)] = q
    c = StopConditions(ptr(ids) if ids.size else None, ids.size, ptr(mat) if seqs else None, stride, ptr(lens) if seqs else None, len(seqs), int(lookahead))
    return c, (ids, mat, lens)


def ban_rules(batch, no_repeat_ngram_size=0, bad_words_ids=None, min_tokens=0, suppress_token_ids=None):
    """zg_ban_rules for `batch` rows from an n-gram size and a min-tokens count (an int for every row, or one per row), a list of bad
    words (token-id lists) and the suppress ids: (the structure, the arrays it points into — keep them alive while it is in use)."""
    import numpy as np

    def per_row(v, name):
        a = np.asarray(v, dtype=np.int64).reshape(-1)
        if np.ndim(v) == 0:
            a = np.repeat(a, batch)
        if a.size != batch or (a < 0).any():
            raise ValueError(f"{name}: {v!r} for a batch of {batch}")
        return np.ascontiguousarray(a, dtype=np.uint64)

    ngram = per_row(no_repeat_ngram_size, "no_repeat_ngram_size")
    mins = per_row(min_tokens, "min_tokens")
    words = [np.ascontiguousarray(w, dtype=np.uint64).reshape(-1) for w in (bad_words_ids or [])]
    lens = np.ascontiguousarray([len(w) for w in words], dtype=np.uint64)
    stride = max([len(w) for w in words] + [1])
    mat = np.zeros((len(words), stride), np.uint64)
    for k, w in enumerate(words):
        mat[k, : len(w)] = w
    supp = np.ascontiguousarray([] if suppress_token_ids is None else suppress_token_ids, dtype=np.uint64).reshape(-1)
    r = BanRules(C.sizeof(BanRules), ptr(ngram), ptr(mat) if words else None, stride, ptr(lens) if words else None, len(words),
                 ptr(supp) if supp.size else None, supp.size, ptr(mins))
    return r, (ngram, mins, mat, lens, supp)


def logit_edits(logit_bias=None, allowed_token_ids=None, banned_token_ids=None, min_p=0.0):
    """zg_logit_edits from a {token id: bias} mapping, an allow-list, a ban-list and min_p: (the structure, the arrays it points
    into — keep them alive while it is in use)."""
    import numpy as np

    bias = dict(logit_bias or {})
    ids = np.ascontiguousarray(list(bias.keys()), dtype=np.uint64).reshape(-1)
    vals = np.ascontiguousarray(list(bias.values()), dtype=np.float32).reshape(-1)
    allowed = np.ascontiguousarray([] if allowed_token_ids is None else allowed_token_ids, dtype=np.uint64).reshape(-1)
    banned = np.ascontiguousarray([] if banned_token_ids is None else banned_token_ids, dtype=np.uint64).reshape(-1)
    e = LogitEdits(ptr(ids) if ids.size else None, ptr(vals) if ids.size else None, ids.size, ptr(allowed) if allowed.size else None, allowed.size,
                   ptr(banned) if banned.size else None, banned.size, float(min_p))
    return e, (ids, vals, allowed, banned)


BLOCK_SLOTS = ["ln_1_g", "ln_1_b", "c_attn_w", "c_attn_b", "c_proj_w", "c_proj_b",
               "ln_2_g", "ln_2_b", "c_fc_w", "c_fc_b", "mlp_proj_w", "mlp_proj_b"]
TOP_SLOTS = ["wte", "wpe", "ln_f_g", "ln_f_b"]
TIME_LM_HEAD = 6
# zg_debug_gpt_step_taps: buffers, element types (numpy: bf16 and the B24 byte plane stay raw), flags, info words
TAP_BUFFERS = ["x", "xp", "xst", "q", "k", "k_lo", "v", "v_lo", "part", "ap", "h4", "hp", "logits", "part_val", "part_idx",
               "a", "qkv_kv", "plan", "geo"]  # (the last four: zg_debug_gpt_pass_taps only)
TAP_DTYPES = ["<f4", "<f2", "<u2", "u1", "<i4"]
TAP_FUSED, TAP_NOT_WRITTEN = 1, 2
PASS_INFO = ["planes", "kv_mode", "weight_type", "pf_ws_floats", "stream_k_operands", "v64", "score_rows"]  # zg_debug_gpt_pass_taps
PASS_TAP_ROWS_BEHIND = 4
AGE_STATE = ["device_epoch", "steps_since_clear", "steps_total", "clears", "sk_epoch", "sk_restarts"]  # zg_debug_gpt_age_state
TAG_CENSUS = ["sk_tag", "part_tag", "qkv_tag", "sk_flags"]  # zg_debug_gpt_tag_census
TAP_INFO = ["planes", "stats", "tags", "fused", "max_splits", "lm_grid", "t_hi", "kv_mode", "weight_type"]


def build(force=False):
    """hipcc --offload-arch=gfx950 build of every HIP source into lib/libzgpt2_hip.so."""
    args = ["make", "-C", CSRC, "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    if not os.path.exists(SO_PATH):
        raise RuntimeError(f"build did not produce {SO_PATH}")
    return SO_PATH


def load():
    """Load the HIP library; raises if it is not built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            f"{SO_PATH} is missing: the HIP extension is required (run `python -c 'import __graft_entry__ as g; g.build()'`)"
        )
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (SONAME libamdhip64.so.7,
    # requested by torch as "libamdhip64.so").  If this library pulled in /opt/rocm's copy first, a
    # later `import torch` would load a second runtime that finds no GPU.  Importing torch first makes
    # the dynamic linker resolve our DT_NEEDED libamdhip64.so.7 to the copy torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(SO_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code):
    if code != 0:
        raise ZgError(code, load().zg_last_error().decode(errors="replace"))


def ptr(a):
    """Raw address of a numpy array (host) or torch tensor (host or device); None -> NULL."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    return a.ctypes.data
