#!/usr/bin/env python3
"""Tokens/s of the sampled device loop at 124M with per-row sampling parameters, beside the uniform calls, for 1 and
8 prompts, 1024 steps.  Two questions:

- Do the uniform calls keep their rate?  temp 0.8 plain, top_k 40 + top_p 0.95, penalised, and both filters + penalties, each on a
  build of the PARENT commit (--parent-lib: its libzgpt2_hip.so) and on this one, in the same call on the same GPU: one worker
  process per library, both alive, measuring the same case in turn — parent, this, this, parent, parent, this ... — so that
  whatever else shares the host, and whatever going first or second is worth, hits both alike.  The margin is the spread of the
  parent's own repetitions, nothing tighter.
- What does a per-row call cost?  A table mixing plain / one filter / two filters / penalised rows (one prompt: one row with both
  filters and penalties) launches the chain of the uniform call with both filters + penalties, which is what it is held against —
  that call on the parent.

Every case is warmed up once at full length (graphs for every bucket exist, code objects are loaded) before anything is timed; a
time is a host clock around enqueue + fetch, which ends in a device synchronise.  One JSON line per (case, prompts):
tok/s of every repetition for both libraries, medians, and `inside`: this commit's median is no lower than the parent's slowest
repetition.  Without --parent-lib only this commit is measured.

python tools/bench_each.py [--parent-lib PATH] [--steps 1024] [--repeats 7] [--prompts 1,8]

Measured 2026-10-21, one MI355X, 8 repetitions, tok/s median parent -> this commit (DESIGN §3.11 has the spreads):
  1 prompt   plain 5276 -> 5207, filters 4399 -> 4335, penalised 5007 -> 4959, filters + penalised 4224 -> 4166; per-row 4178
  8 prompts  plain 24377 -> 24369, filters 21368 -> 21319, penalised 23549 -> 23485, filters + penalised 20678 -> 20627; per-row mix 20871
The one-prompt uniform calls are 1.0-1.4 % below the parent, outside its spread (+-0.3 %); this library in both seats reads the same
in both (5214 / 5231); each build alone in a process of its own reads within 0.5 % of the other (plain: 5267 / 5241 against 5243 /
5245).  The cause is not found."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EACH_SYMBOLS = ["zg_gpt_generate_each_enqueue", "zg_gpt_sample_each", "zg_debug_sample_rows_each", "zg_debug_penalize_rows_each", "zg_debug_each_plan"]
PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.15)
FILT = dict(top_k=40, top_p=0.95)
UNIFORM = {"plain": {}, "top_k 40 + top_p 0.95": FILT, "penalised": PEN, "top_k 40 + top_p 0.95 + penalised": dict(FILT, **PEN)}
MIX = [dict(temp=0.8), dict(temp=0.7, top_k=40), dict(temp=0.8, **FILT), dict(temp=1.0, **PEN), dict(temp=0.9, top_p=0.9), dict(temp=0.8, **FILT, **PEN),
       dict(temp=1.2), dict(temp=0.8, top_k=1)]
EACH = "per-row mix"


def worker(parent_build):
    """One library, one handle per prompt count; measures what the driver names, one line in, one line out."""
    import time

    import numpy as np

    sys.path.insert(0, ROOT)
    from zig_gpt2_amd import _lib, gpt as zgpt, synth

    if parent_build:  # (a parent build lacks the per-row entry points)
        for name in EACH_SYMBOLS:
            _lib.SIGNATURES.pop(name)
    _lib.check(_lib.load().zg_init(0))
    cfg = synth.CONFIGS["124M"]
    w = synth.make_weights(cfg, seed=0, bf16=True)
    handles = {}
    print(json.dumps({"ready": True}), flush=True)
    for line in sys.stdin:
        q = json.loads(line)
        n, case, steps = q["prompts"], q["case"], q["steps"]
        if n not in handles:
            handles[n] = zgpt.GPT(cfg, batch=n, sampled_generate=True, truncated_generate=True, penalized_generate=True)
            handles[n].load_weights(w)
        m = handles[n]
        prompts = [synth.rand_tokens(1000 + b, 1, cfg.vocab_size) for b in range(n)]
        t0 = time.perf_counter()
        if case == EACH:
            rows = [dict(MIX[(5 if n == 1 else b) % len(MIX)], seed=q["seed"] + b) for b in range(n)]
            out = m.generate_each(prompts, steps, rows)
        else:
            out = m.generate_sample(prompts, steps, 0.8, seed=q["seed"], **UNIFORM[case])
        dt = time.perf_counter() - t0
        assert out.shape == (n, steps) and (np.asarray(out) < cfg.vocab_size).all()
        print(json.dumps({"s": dt}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libzgpt2_hip.so built from the parent commit")
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--prompts", default="1,8")
    ap.add_argument("--cases", default=None, help="comma-separated subset of the cases (default: all)")
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
            beside = None
            for case in [c for c in list(UNIFORM) + [EACH] if args.cases is None or c in args.cases.split(",")]:
                on = [lib for lib in libs if not (lib == "parent" and case == EACH)]
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
                same_chain = "top_k 40 + top_p 0.95 + penalised"
                if case == same_chain:
                    beside = {lib: rec[f"{lib}_median"] for lib in on}
                if case == EACH and beside:  # held against the uniform call that launches the same chain, on the parent where there is one
                    rec["uniform_same_chain_median"] = beside.get("parent", beside["this"])
                    rec["over_uniform_same_chain"] = round(rec["this_median"] / rec["uniform_same_chain_median"], 4)
                print(json.dumps(rec), flush=True)
    finally:
        for p in procs.values():
            p.stdin.close()
        for p in procs.values():
            p.wait()


if __name__ == "__main__":
    main()
