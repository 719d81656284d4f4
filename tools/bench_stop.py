#!/usr/bin/env python3
"""The cost of stop conditions in the device loop at 124M, for 1 and 8 prompts, greedy and temperature 0.8, one
handle per prompt count with every graph captured at create, all in one call:
(a) tokens/s over the full context (1024 steps) with conditions that never match — a token no row picks, checked on the run without
    conditions — for every `lookahead` of the sweep, against the same call without conditions (the path and rate of a build without
    the stage).  The configurations alternate inside every repeat, so that they share whatever else the host is doing; each reports
    its best, its median and all repeats: the spread of the unlimited lookahead (1024) is what the others are judged against.
(b) wall time of a generation every row of which finishes at about column 256 of 1024 (a token each row picks there), against the
    full run, with the default lookahead.
Every timed window ends behind a fetch: the stream is drained.  Prints one JSON line.
python tools/bench_stop.py [--steps 1024] [--repeats 5] [--prompts 1,8] [--lookaheads 8,16,32,64,128,256,1024] [--finish-at 256]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zig_gpt2_amd import _lib, gpt as zgpt, synth

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=1024)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--prompts", default="1,8")
ap.add_argument("--lookaheads", default="8,16,32,64,128,256,1024")
ap.add_argument("--finish-at", type=int, default=256)
ap.add_argument("--model", default="124M")
args = ap.parse_args()
zg = _lib.load()
_lib.check(zg.zg_init(0))
cfg = synth.CONFIGS[args.model]
w = synth.make_weights(cfg, seed=0, bf16=True)
lookaheads = [int(v) for v in args.lookaheads.split(",")]
sweep, early = [], []
for n_prompts in (int(v) for v in args.prompts.split(",")):
    prompts = [synth.rand_tokens(1000 + b, 1, cfg.vocab_size) for b in range(n_prompts)]
    m = zgpt.GPT(cfg, batch=n_prompts, sampled_generate=True, stop_generate=True)
    m.load_weights(w)

    def run(sampler, steps, **stop):
        mode = {} if sampler == "greedy" else dict(temp=0.8, seed=1)
        return m.generate_from(0, prompts, steps, **mode, **stop)

    def timed(sampler, **stop):
        t0 = time.perf_counter()
        out = run(sampler, args.steps, **stop)  # (returns behind the fetch: the stream is drained)
        return time.perf_counter() - t0, out

    for sampler in ("greedy", "temp=0.8"):
        twin = run(sampler, args.steps)
        absent = next(t for t in range(cfg.vocab_size) if not (twin == t).any())
        configs = [("off", {})] + [(la, dict(stop_token_ids=[absent], stop=[[absent, absent]], lookahead=la)) for la in lookaheads]
        for _, stop in configs:
            run(sampler, 64, **stop)  # warm-up
        times = {name: [] for name, _ in configs}
        for r in range(args.repeats):
            for name, stop in configs[r % len(configs):] + configs[: r % len(configs)]:  # alternating, the order rotating
                t, out = timed(sampler, **stop)
                assert out.shape == twin.shape and (out == twin).all(), (name, "the tokens changed")
                times[name].append(t)
        for name, _ in configs:
            ts = times[name]
            sweep.append({"prompts": n_prompts, "sampler": sampler, "lookahead": name, "tok_s_best": round(n_prompts * args.steps / min(ts), 1),
                          "tok_s_median": round(n_prompts * args.steps / statistics.median(ts), 1),
                          "us_per_step_best": round(min(ts) / args.steps * 1e6, 2), "tok_s_repeats": [round(n_prompts * args.steps / t, 1) for t in ts]})
        # (b) every row picks its stop token at finish_at - b at the latest
        at = min(args.finish_at, args.steps - 1)
        ids = sorted({int(twin[b, at - b]) for b in range(n_prompts)})
        full, cut = [], []
        for r in range(args.repeats):
            full.append(timed(sampler)[0])
            t, out = timed(sampler, stop_token_ids=ids)
            end, cols, _ = m.stop_result()
            assert (out == twin[:, :end]).all()
            cut.append(t)
        early.append({"prompts": n_prompts, "sampler": sampler, "last_finish_col": max(cols), "end": end, "ms_full_best": round(min(full) * 1e3, 2),
                      "ms_stopped_best": round(min(cut) * 1e3, 2), "ms_full_median": round(statistics.median(full) * 1e3, 2),
                      "ms_stopped_median": round(statistics.median(cut) * 1e3, 2)})
    m.close()
print(json.dumps({"model": args.model, "steps": args.steps, "repeats": args.repeats, "never_matching": sweep, "early_end": early}), flush=True)
