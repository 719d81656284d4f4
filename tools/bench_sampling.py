#!/usr/bin/env python3
"""Tokens/s of the sampled device loop at 124M with and without truncation: untruncated generate_sample, top_k=40, top_p=0.95,
and both, for 1 and 8 prompts, 1024 steps, best of 3 (one JSON line per case; --repeats N prints every repeat's figure, for a
noise band).  On a commit without the truncated sampler only the untruncated case runs.
python tools/bench_sampling.py [--steps 1024] [--repeats 3] [--prompts 1,8]"""
import argparse
import inspect
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

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
has_trunc = "top_k" in inspect.signature(zgpt.GPT.generate_sample).parameters
cases = [("untruncated", {})]
if has_trunc:
    cases += [("top_k=40", dict(top_k=40)), ("top_p=0.95", dict(top_p=0.95)), ("top_k=40,top_p=0.95", dict(top_k=40, top_p=0.95))]
for n_prompts in (int(v) for v in args.prompts.split(",")):
    prompts = [synth.rand_tokens(1000 + b, 1, cfg.vocab_size) for b in range(n_prompts)]
    kw = dict(batch=n_prompts, sampled_generate=True)
    if has_trunc:
        kw["truncated_generate"] = True
    m = zgpt.GPT(cfg, **kw)
    m.load_weights(w)
    base = None
    for name, opts in cases:
        m.generate_sample(prompts, 64, 0.8, seed=1, **opts)  # warm-up
        times = []
        for r in range(args.repeats):
            t0 = time.perf_counter()
            out = m.generate_sample(prompts, args.steps, 0.8, seed=1 + r, **opts)
            times.append(time.perf_counter() - t0)
        assert (out < cfg.vocab_size).all()
        best = min(times)
        us_step = best / args.steps * 1e6
        if base is None:
            base = us_step
        print(json.dumps({"case": name, "prompts": n_prompts, "steps": args.steps, "tok_s_best": round(n_prompts * args.steps / best, 1),
                          "us_per_step_best": round(us_step, 2), "us_per_step_over_untruncated": round(us_step - base, 2),
                          "tok_s_repeats": [round(n_prompts * args.steps / t, 1) for t in times]}), flush=True)
    m.close()
