#!/usr/bin/env python3
"""Tokens/s of the sampled device loop at 124M with guided decoding, for 1 and 8 prompts, 1024 steps, temp 0.8:
off -> a 300-entry logit_bias alone -> guided -> guided + the same bias.  The guide is a cycle of 16 states, state s allowing the
tokens of s's parity (half the vocabulary) and leading to s + 1: every step reads another bitmap and follows a transition.

"off" and "bias 300" run the PARENT's graphs and are measured as tools/bench_each.py measures: a build of the parent commit
(--parent-lib: its libzgpt2_hip.so) and this one as two live worker processes on the same GPU, measuring the same case in turn —
parent, this, this, parent ... — and read against the spread of the parent's own repetitions, never against this build alone.  The
guided cases exist on this build only; what they cost is read against this build's own "off" / "bias 300" of the same call, in
microseconds a step.

The expectation, written down before the first run: the mask is one launch of the edit stage's cost class (DESIGN §3.10 measured
2.2-5.9 us a step for that launch), the advance one launch of the stop stage's class; guided + bias costs one launch more than the
bias alone (the advance), the row being rewritten by one launch for both.

Every case is warmed up once at full length before anything is timed; a time is a host clock around enqueue + fetch.  One JSON
line per (case, prompts).  python tools/bench_guided.py [--parent-lib PATH] [--steps 1024] [--repeats 7] [--prompts 1,8]

Measured 2026-10-21, one MI355X, 7 repetitions, tok/s median (DESIGN §3.12 has the spreads):
  1 prompt   off 5244 (parent) -> 5208, bias 5159 -> 5122, guided 5074 (+5.1 us a step over off), guided + bias 5033 (+3.4 us over bias)
  8 prompts  off 24324 -> 24340, bias 23921 -> 23927, guided 23717 (+8.6 us a step over off), guided + bias 23576 (+5.0 us over bias)
One prompt "off" is 0.7 % below the parent and outside its spread, as in tools/bench_each.py's account and without a cause in the
code (the graphs are the parent's); eight prompts are inside."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUIDE_SYMBOLS = ["zg_gpt_guide_load", "zg_gpt_generate_guided_enqueue", "zg_gpt_generate_fetch_guide_states", "zg_debug_guide_rows", "zg_debug_guide_check"]
CASES = ["off", "bias 300", "guided", "guided + bias 300"]
N_STATES = 16


def worker(parent_build):
    """One library, one handle per prompt count; measures what the driver names, one line in, one line out."""
    import time

    import numpy as np

    sys.path.insert(0, ROOT)
    from zig_gpt2_amd import _lib, gpt as zgpt, synth

    if parent_build:  # (a parent build lacks the guided entry points)
        for name in GUIDE_SYMBOLS:
            _lib.SIGNATURES.pop(name)
    _lib.check(_lib.load().zg_init(0))
    cfg = synth.CONFIGS["124M"]
    V = cfg.vocab_size
    w = synth.make_weights(cfg, seed=0, bf16=True)
    rng = np.random.default_rng(0)
    bias = {int(i): float(v) for i, v in zip(rng.choice(V, 300, replace=False), rng.standard_normal(300) * 2)}
    guide = None
    if not parent_build:
        from zig_gpt2_amd.guide import DEAD, Guide

        nxt = np.full((N_STATES, V), DEAD, np.uint16)
        for s in range(N_STATES):
            nxt[s, s % 2:: 2] = (s + 1) % N_STATES
        guide = Guide(nxt)
    handles = {}
    print(json.dumps({"ready": True}), flush=True)
    for line in sys.stdin:
        q = json.loads(line)
        n, case, steps = q["prompts"], q["case"], q["steps"]
        if n not in handles:
            kw = {} if parent_build else dict(guided=True)
            handles[n] = zgpt.GPT(cfg, batch=n, sampled_generate=True, edited_generate=True, **kw)
            handles[n].load_weights(w)
            if guide is not None:
                handles[n].load_guide(guide)
        m = handles[n]
        prompts = [synth.rand_tokens(1000 + b, 1, V) for b in range(n)]
        kw = dict(logit_bias=bias) if "bias" in case else {}
        if "guided" in case:
            kw["guide_states"] = [b % N_STATES for b in range(n)]
        t0 = time.perf_counter()
        out = m.generate_sample(prompts, steps, 0.8, seed=q["seed"], **kw)
        dt = time.perf_counter() - t0
        assert out.shape == (n, steps) and (np.asarray(out) < V).all()
        if "guided" in case:  # row b starts in state b: the pick of column p has the parity of b + p - 1
            par = (np.arange(n)[:, None] + np.arange(steps)[None, :] - 1) % 2
            assert (np.asarray(out[:, 1:]) % 2 == par[:, 1:]).all()
        print(json.dumps({"s": dt}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libzgpt2_hip.so built from the parent commit")
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--prompts", default="1,8")
    ap.add_argument("--worker", choices=["this", "parent"], default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker == "parent")
    libs = (["parent"] if args.parent_lib else []) + ["this"]
    procs = {}
    for lib in libs:  # a fresh process per library: each initialises the GPU itself
        env = dict(os.environ)
        if lib == "parent":
            env["ZGPT2_LIB"] = os.path.abspath(args.parent_lib)
        else:
            env.pop("ZGPT2_LIB", None)
        procs[lib] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", lib], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True,
                                      env=env)

    def ask(lib, **q):
        p = procs[lib]
        if q:
            p.stdin.write(json.dumps(q) + "\n")
            p.stdin.flush()
        line = p.stdout.readline()
        if not line:
            raise RuntimeError(f"the {lib} worker ended (exit status {p.wait()})")
        return json.loads(line)

    try:
        for lib in libs:
            ask(lib)
        for n in (int(v) for v in args.prompts.split(",")):
            us = {}  # this build's median microseconds a step, by case
            for case in CASES:
                on = [lib for lib in libs if not (lib == "parent" and "guided" in case)]
                for lib in on:  # warm-up at full length
                    ask(lib, prompts=n, case=case, steps=args.steps, seed=1)
                rate = {lib: [] for lib in on}
                for r in range(args.repeats):  # interleaved, and whoever went first goes second in the next repetition
                    for lib in (on if r % 2 == 0 else on[::-1]):
                        rate[lib].append(n * args.steps / ask(lib, prompts=n, case=case, steps=args.steps, seed=2 + r)["s"])
                rec = {"case": case, "prompts": n, "steps": args.steps}
                for lib in on:
                    rec[f"{lib}_tok_s"] = [round(v, 1) for v in rate[lib]]
                    rec[f"{lib}_median"] = round(statistics.median(rate[lib]), 1)
                if "parent" in on:
                    rec["parent_spread"] = [round(min(rate["parent"]), 1), round(max(rate["parent"]), 1)]
                    rec["inside"] = statistics.median(rate["this"]) >= min(rate["parent"])
                us[case] = n * 1e6 / statistics.median(rate["this"])
                rec["this_us_per_step"] = round(us[case], 2)
                if case == "guided":
                    rec["us_per_step_over_off"] = round(us[case] - us["off"], 2)
                if case == "guided + bias 300":
                    rec["us_per_step_over_bias"] = round(us[case] - us["bias 300"], 2)
                print(json.dumps(rec), flush=True)
    finally:
        for p in procs.values():
            p.stdin.close()
        for p in procs.values():
            p.wait()


if __name__ == "__main__":
    main()
