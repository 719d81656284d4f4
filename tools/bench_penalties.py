#!/usr/bin/env python3
"""Tokens/s of the sampled device loop at 124M with and without logit penalties: the plain sampler, top_k=40, and top_k=40 with
top_p=0.95, each unpenalised and with repetition 1.3 / presence 0.4 / frequency 0.15, for 1 and 8 prompts, 1024 steps, best of 3,
one handle per prompt count, all in one call (one JSON line per case; --repeats N prints every repeat's figure, for a noise band).
python tools/bench_penalties.py [--steps 1024] [--repeats 3] [--prompts 1,8]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zig_gpt2_amd import _lib, gpt as zgpt, synth

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--prompts", default="1,8")
args = ap.parse_args()
zg = _lib.load()
_lib.check(zg.zg_init(0))
cfg = synth.CONFIGS["124M"]
w = synth.make_weights(cfg, seed=0, bf16=True)
PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.15)
samplers = [("plain", {}), ("top_k=40", dict(top_k=40)), ("top_k=40,top_p=0.95", dict(top_k=40, top_p=0.95))]
for n_prompts in (int(v) for v in args.prompts.split(",")):
    prompts = [synth.rand_tokens(1000 + b, 1, cfg.vocab_size) for b in range(n_prompts)]
    m = zgpt.GPT(cfg, batch=n_prompts, sampled_generate=True, truncated_generate=True, penalized_generate=True)
    m.load_weights(w)
    for name, opts in samplers:
        base = None
        for pen_name, pen in (("", {}), (" + penalties", PEN)):
            m.generate_sample(prompts, 64, 0.8, seed=1, **opts, **pen)  # warm-up
            times = []
            for r in range(args.repeats):
                t0 = time.perf_counter()
                out = m.generate_sample(prompts, args.steps, 0.8, seed=1 + r, **opts, **pen)
                times.append(time.perf_counter() - t0)
            assert (out < cfg.vocab_size).all()
            best = min(times)
            us_step = best / args.steps * 1e6
            if base is None:
                base = us_step
            print(json.dumps({"case": name + pen_name, "prompts": n_prompts, "steps": args.steps, "tok_s_best": round(n_prompts * args.steps / best, 1),
                              "us_per_step_best": round(us_step, 2), "us_per_step_over_unpenalised": round(us_step - base, 2),
                              "tok_s_repeats": [round(n_prompts * args.steps / t, 1) for t in times]}), flush=True)
    m.close()
