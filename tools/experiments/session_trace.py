"""Scripted session for the launch-trace comparison: python tools/experiments/session_trace.py OUT.npz  (library chosen by ZGPT2_LIB)."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from zig_gpt2_amd import _lib, gpt, ops, synth

lib = _lib.load()
_lib.check(lib.zg_init(0))
out = {}
marks = []


def weights(cfg, seed=3):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed)
    w = {}
    for name, shape, mean, _ in synth.tensor_specs(cfg):
        w[name] = ((torch.randn(shape, generator=gen, device="cuda") * 0.02 + mean).to(torch.bfloat16).to(torch.float32)).contiguous()
    torch.cuda.synchronize()
    return w


def mark():
    x = np.ones(64, np.float32)
    ops.gelu(x)


def toks(seed, B, n, V):
    return np.stack([synth.rand_tokens(seed + b, n, V) for b in range(B)])


def session(tag, cfg, w, B, long=True, prefill=True, **kw):
    V, Cx = cfg.vocab_size, cfg.context_size
    m = gpt.GPT(cfg, batch=B, prefill=prefill, **kw)
    m.load_weights(w)
    r = {}
    upto = min(82, Cx)
    if prefill:
        r["pf12"] = m.prefill(toks(1, B, 12, V))
        if long:
            r["pf300"] = m.prefill(toks(2, B, 300, V))
        m.prefill(toks(3, B, 31, V), compute_logits=False)
        r["ext5"] = m.extend(31, toks(4, B, 5, V))
        if long:
            m.prefill(toks(5, B, 300, V), compute_logits=False)
            r["ext300"] = m.extend(300, toks(6, B, 300, V))
            r["rollback"] = m.extend(100, toks(7, B, 20, V))
        else:
            r["rollback"] = m.extend(10, toks(7, B, 6, V))
        r["ext0"] = m.extend(0, toks(8, B, 9, V))
    prompts = [synth.rand_tokens(20 + b, 12, V) for b in range(B)]
    r["greedy"] = m.generate(prompts, upto)
    r["samp"] = m.generate_sample(prompts, upto, 0.9, seed=5)
    r["samp_k"] = m.generate_sample(prompts, upto, 0.9, seed=5, top_k=40)
    r["samp_kp"] = m.generate_sample(prompts, upto, 0.9, seed=5, top_k=40, top_p=0.95)
    past = 40 if Cx >= 96 else 8
    m.generate(prompts, past)
    new = [synth.rand_tokens(40 + b, 6, V) for b in range(B)]
    r["from_greedy"] = m.generate_from(past, new, upto - past)
    m.generate(prompts, past)
    r["from_kp"] = m.generate_from(past, new, upto - past, temp=0.8, seed=7, top_k=40, top_p=0.95)
    for T in (1, 2, 3):
        r[f"fwd{T}"] = m.forward(T, toks(50 + T, B, 1, V)[:, 0])
    r["sample"] = m.sample(4, toks(60, B, 1, V)[:, 0], 0.9, seed=3)
    r["sample_ex"] = m.sample(5, toks(61, B, 1, V)[:, 0], 0.9, seed=3, top_k=40, top_p=0.9)
    # the sampling tail: penalties with a prior, log-probabilities behind the greedy pick and behind both filters, both on a continuation
    pen = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.2)
    prior = [synth.rand_tokens(80 + b, 5, V) for b in range(B)]  # (prior + steps stay within the context: 5 steps fewer)
    r["samp_pen"] = m.generate_sample(prompts, upto - 5, 0.9, seed=5, prior=prior, **pen)
    r["greedy_lp5"] = m.generate(prompts, upto, logprobs=5)
    r["samp_kp_lp5"] = m.generate_sample(prompts, upto, 0.9, seed=5, top_k=40, top_p=0.95, logprobs=5)
    m.generate(prompts, past)
    r["from_pen_lp20"] = m.generate_from(past, new, upto - past - 5, temp=0.8, seed=7, prior=prior, logprobs=20, **pen)
    m.forward(1, toks(62, B, 1, V)[:, 0], compute_logits=False)
    r["sample_pen"] = m.sample(2, toks(63, B, 1, V)[:, 0], 0.9, seed=3, history=[synth.rand_tokens(90 + b, 7, V) for b in range(B)], **pen)
    # the rest of the sampler chain: the stop stage (a stop sequence of two tokens that neither run it is added to ever picks in a
    # row: the generation runs to its end, so the launches do not depend on when the host saw the device finish), a bias list, an
    # allow list behind penalties, min-p alone, and the per-token call with edits and with penalties and edits together
    seen = {(int(x[i]), int(x[i + 1])) for a in (r["greedy"], r["samp_k"]) for x in a for i in range(len(x) - 1)}
    never = next([a, b] for a in range(V) for b in range(V) if (a, b) not in seen)
    r["greedy_stop"] = m.generate(prompts, upto, stop=[never])
    r["samp_k_stop_lp5"] = m.generate_sample(prompts, upto, 0.9, seed=5, top_k=40, logprobs=5, stop=[never])
    assert m.stop_result()[0] == upto
    bias = {int(t): 1.5 - 0.5 * i for i, t in enumerate(sorted(set(int(t) for t in synth.rand_tokens(95, 6, V))))}
    allowed = sorted(set(int(t) for t in synth.rand_tokens(96, V // 3, V)))
    r["samp_bias"] = m.generate_sample(prompts, upto, 0.9, seed=5, logit_bias=bias, banned_token_ids=[int(t) for t in synth.rand_tokens(97, 3, V)])
    r["samp_allow_pen"] = m.generate_sample(prompts, upto - 5, 0.9, seed=5, top_p=0.9, prior=prior, allowed_token_ids=allowed, **pen)
    r["samp_minp"] = m.generate_sample(prompts, upto, 0.9, seed=5, min_p=0.1)
    r["sample_edit"] = m.sample(3, toks(64, B, 1, V)[:, 0], 0.9, seed=3, top_k=40, logit_bias=bias, allowed_token_ids=allowed, min_p=0.05)
    r["sample_pen_edit"] = m.sample(4, toks(65, B, 1, V)[:, 0], 0.9, seed=3, history=[synth.rand_tokens(90 + b, 7, V) for b in range(B)],
                                    logit_bias=bias, **pen)
    if kw.get("score"):
        n = (300 if B == 1 else 70) if long else min(20, Cx)  # (more than one block of lm_head rows where the model is large)
        r["score0"] = m.score(toks(9, B, n, V), top_n=0, want_logits=True)
        r["score20"] = m.score(toks(10, B, 12, V), past_len=n // 2, top_n=20, want_logits=True)
    m.close()
    for k, v in r.items():
        for i, a in enumerate(v if isinstance(v, tuple) else (v,)):  # (tokens, logprobs, top_ids, top_logprobs[, logits]): one array each
            out[f"{tag}/{k}" + (f"/{i}" if isinstance(v, tuple) else "")] = np.asarray(a)
    marks.append(tag)
    mark()
    print("done", tag, flush=True)


cfg = synth.CONFIGS["124M"]
w = weights(cfg)
mark()
for B in (1, 4):
    session(f"124M b{B} bf16", cfg, w, B, score=True)
    session(f"124M b{B} bf16 kv_f16", cfg, w, B, kv_f16=True)
    session(f"124M b{B} bf16 kv_b24", cfg, w, B, kv_b24=True)
    session(f"124M b{B} f32w", cfg, w, B, weights_f32=True, score=B == 1)
    session(f"124M b{B} b24w kv_f16", cfg, w, B, weights_b24=True, kv_f16=True)
session("124M b1 no_graph", cfg, w, 1, use_graph=False)
session("124M b1 no_prefill", cfg, w, 1, prefill=False)

# two handles under zg_gpt_generate_enqueue_many
grp = gpt.GPTGroups(cfg, 2, 2)
grp.load_weights(w)
out["groups/greedy"] = grp.generate([synth.rand_tokens(70 + b, 12, cfg.vocab_size) for b in range(2)], 82)
grp.close()
marks.append("124M 2 x 1 groups")
mark()
del w

for name, B in (("tiny3", 3), ("nano-char", 1)):
    c = synth.CONFIGS[name]
    session(f"{name} b{B}", c, weights(c), B, long=False, score=True)

# the sampler chain on rows of the caller's (no handle): one call each of the three debug entry points at a vocabulary of 1000
B, V = 3, 1000
rng = np.random.default_rng(11)
x = (rng.standard_normal((B, V)) * 3).astype(np.float32)
u = rng.random(B).astype(np.float32)
tok, probs, thr, edited = np.zeros(B, np.uint64), np.zeros((B, V), np.float32), np.zeros(B, np.float32), np.zeros((B, V), np.float32)
opt = _lib.SampleOptions(0.9, 40, 0.9)
_lib.check(lib.zg_debug_sample_rows(_lib.ptr(x), B, V, C.addressof(opt), _lib.ptr(u), _lib.ptr(tok), _lib.ptr(probs), _lib.ptr(thr)))
out["rows/sample/0"], out["rows/sample/1"], out["rows/sample/2"] = tok.copy(), probs.copy(), thr.copy()
e, keep = _lib.logit_edits({5: 2.0, 999: -1.0}, None, [7, 8, 9], 0.05)
_lib.check(lib.zg_debug_edit_rows(_lib.ptr(x), B, V, C.addressof(opt), C.addressof(e), _lib.ptr(u), _lib.ptr(edited), _lib.ptr(tok), _lib.ptr(probs), _lib.ptr(thr)))
out["rows/edit/0"], out["rows/edit/1"], out["rows/edit/2"], out["rows/edit/3"] = edited.copy(), tok.copy(), probs.copy(), thr.copy()
hist = np.ascontiguousarray(rng.integers(0, V, (B, 40)), np.uint64)
lens = np.array([40, 0, 17], np.uint64)
pen = _lib.LogitPenalties(1.3, 0.4, 0.2)
counts = np.zeros((B, V), np.uint32)
_lib.check(lib.zg_debug_penalize_rows(_lib.ptr(x), B, V, C.addressof(pen), _lib.ptr(hist), 40, _lib.ptr(lens), _lib.ptr(edited), _lib.ptr(counts)))
out["rows/penalize/0"], out["rows/penalize/1"] = edited.copy(), counts.copy()
marks.append("debug rows")
mark()

np.savez(sys.argv[1], **out)
open(sys.argv[1] + ".marks", "w").write("\n".join(marks) + "\n")
print("session ok", len(out), "results")
