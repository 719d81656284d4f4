"""Scripted session for the launch-trace comparison: python tools/experiments/session_trace.py OUT.npz  (library chosen by ZGPT2_LIB)."""
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

np.savez(sys.argv[1], **out)
open(sys.argv[1] + ".marks", "w").write("\n".join(marks) + "\n")
print("session ok", len(out), "results")
