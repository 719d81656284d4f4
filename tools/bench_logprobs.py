#!/usr/bin/env python3
"""Tokens/s of the device loop at 124M with and without the log-probability stage: greedy and temperature 0.8, each
with log-probabilities off and on with top_n = 0, 5 and 20, for 1 and 8 prompts over the full context (1024 steps), best of 3, one
handle per prompt count with every graph captured at create, all in one call.  Prints one JSON line.  --off-only measures the
plain generations alone (what a build without the stage can run: the same line from both builds is the comparison).
python tools/bench_logprobs.py [--steps 1024] [--repeats 3] [--prompts 1,8] [--off-only]"""
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
ap.add_argument("--off-only", action="store_true")
args = ap.parse_args()
zg = _lib.load()
_lib.check(zg.zg_init(0))
cfg = synth.CONFIGS["124M"]
w = synth.make_weights(cfg, seed=0, bf16=True)
levels = [None] if args.off_only else [None, 0, 5, 20]
cases = []
for n_prompts in (int(v) for v in args.prompts.split(",")):
    prompts = [synth.rand_tokens(1000 + b, 1, cfg.vocab_size) for b in range(n_prompts)]
    m = zgpt.GPT(cfg, batch=n_prompts, sampled_generate=True, **({} if args.off_only else dict(logprobs_generate=True)))
    m.load_weights(w)

    def run(sampler, top_n, steps, seed):
        kw = {} if top_n is None else dict(logprobs=top_n)
        out = m.generate(prompts, steps, **kw) if sampler == "greedy" else m.generate_sample(prompts, steps, 0.8, seed=seed, **kw)
        return out if top_n is None else out[0]

    for sampler in ("greedy", "temp=0.8"):
        base = None
        for top_n in levels:
            run(sampler, top_n, 64, 1)  # warm-up
            times = []
            for r in range(args.repeats):
                t0 = time.perf_counter()
                out = run(sampler, top_n, args.steps, 1 + r)  # (returns behind the fetch: the stream is drained)
                times.append(time.perf_counter() - t0)
            assert (out < cfg.vocab_size).all()
            best = min(times)
            us_step = best / args.steps * 1e6
            if base is None:
                base = us_step
            cases.append({"prompts": n_prompts, "sampler": sampler, "logprobs": "off" if top_n is None else top_n,
                          "tok_s_best": round(n_prompts * args.steps / best, 1), "us_per_step_best": round(us_step, 2),
                          "us_per_step_over_off": round(us_step - base, 2), "tok_s_repeats": [round(n_prompts * args.steps / t, 1) for t in times]})
    m.close()
print(json.dumps({"model": "124M", "steps": args.steps, "repeats": args.repeats, "cases": cases}), flush=True)
