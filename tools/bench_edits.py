#!/usr/bin/env python3
"""Tokens/s of the sampled device loop at 124M with and without logit edits: greedy-equivalent (temp 1, top_k = 1)
and temp 0.8, each with edits off, a 300-entry logit_bias, a 10-token allow-list, min_p 0.05 alone and all three together, for 1
and 8 prompts, 1024 steps, best of 3, one handle per prompt count, all in one call (one JSON line per case; --repeats N prints
every repeat's figure, for a noise band).  "off" runs the parent's graphs: it is the figure to hold against bench.py's.
python tools/bench_edits.py [--steps 1024] [--repeats 3] [--prompts 1,8]"""
import argparse
import json
import os
import sys
import time

import numpy as np

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
rng = np.random.default_rng(0)
bias = {int(i): float(v) for i, v in zip(rng.choice(cfg.vocab_size, 300, replace=False), rng.standard_normal(300) * 2)}
allowed = sorted(int(i) for i in rng.choice(cfg.vocab_size, 10, replace=False))
edits = [("off", {}), ("bias 300", dict(logit_bias=bias)), ("allow 10", dict(allowed_token_ids=allowed)), ("min_p 0.05", dict(min_p=0.05)),
         ("bias 300 + allow 10 + min_p 0.05", dict(logit_bias=bias, allowed_token_ids=allowed, min_p=0.05))]
samplers = [("temp 1 top_k 1", 1.0, dict(top_k=1)), ("temp 0.8", 0.8, {})]
for n_prompts in (int(v) for v in args.prompts.split(",")):
    prompts = [synth.rand_tokens(1000 + b, 1, cfg.vocab_size) for b in range(n_prompts)]
    m = zgpt.GPT(cfg, batch=n_prompts, sampled_generate=True, truncated_generate=True, edited_generate=True)
    m.load_weights(w)
    for name, temp, opts in samplers:
        base = None
        for edit_name, kw in edits:
            m.generate_sample(prompts, 64, temp, seed=1, **opts, **kw)  # warm-up
            times = []
            for r in range(args.repeats):
                t0 = time.perf_counter()
                out = m.generate_sample(prompts, args.steps, temp, seed=1 + r, **opts, **kw)
                times.append(time.perf_counter() - t0)
            assert (out < cfg.vocab_size).all()
            if "allowed_token_ids" in kw:
                assert set(int(t) for t in out[:, 1:].ravel()) <= set(allowed)
            best = min(times)
            us_step = best / args.steps * 1e6
            if base is None:
                base = us_step
            print(json.dumps({"sampler": name, "edits": edit_name, "prompts": n_prompts, "steps": args.steps,
                              "tok_s_best": round(n_prompts * args.steps / best, 1), "us_per_step_best": round(us_step, 2),
                              "us_per_step_over_off": round(us_step - base, 2), "tok_s_repeats": [round(n_prompts * args.steps / t, 1) for t in times]}),
                  flush=True)
    m.close()
