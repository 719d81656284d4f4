#!/usr/bin/env python3
"""Tokens/s of the sampled device loop at 124M with the history-dependent bans, for 1 and 8 prompts, 1024 steps, temp
0.8: off -> no_repeat_ngram_size 3 -> 32 bad words (of 2 to 4 tokens) -> min_tokens 64 with 8 suppress ids -> all three, and the
same five beside a 300-entry logit_bias.

"off" and "bias 300" run the PARENT's graphs and are measured as tools/bench_guided.py measures: a build of the parent commit
(--parent-lib: its libzgpt2_hip.so) and this one as two live worker processes on the same GPU, measuring the same case in turn —
parent, this, this, parent ... — and read against the spread of the parent's own repetitions, never against this build alone.  The
banned cases exist on this build only; what they cost is read against this build's own "off" / "bias 300" of the same call, in
microseconds a step.

The expectation, written down before the first run: the ban launch is one workgroup per row that loads at most 1024 tokens into the
LDS and compares them once, and the rebuild is the penalty stage's second launch — two launches of the penalty stage's shapes, so
near its cost; beside the bias the edit launch rebuilds and the bans add ONE launch.

Every case is warmed up once at full length before anything is timed; a time is a host clock around enqueue + fetch.  One JSON
line per (case, prompts).  python tools/bench_bans.py [--parent-lib PATH] [--steps 1024] [--repeats 7] [--prompts 1,8]

Measured 2026-10-21, one MI355X, 7 repetitions, tok/s median (DESIGN §3.13 has the table and the spreads):
  1 prompt   off 5226 (parent) -> 5264, n = 3 5116 (+5.5 us a step over off), 32 words 5110 (+5.7), min_tokens 5167 (+3.6), all three
             5094 (+6.3); bias 5119 -> 5168, and beside it +3.2 / +3.4 / +1.3 / +4.2 us a step over the bias alone
  8 prompts  off 24299 -> 24306, n = 3 23762 (+7.5), 32 words 23742 (+7.8), min_tokens 23899 (+5.6), all three 23698 (+8.4); bias
             23896 -> 23881, and beside it +4.4 / +4.8 / +2.3 / +5.4
"Off" and the bias alone are inside the parent's spread at both prompt counts."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAN_SYMBOLS = ["zg_gpt_generate_banned_enqueue", "zg_debug_ban_check", "zg_debug_ban_rows"]
RULES = ["off", "ngram 3", "words 32", "min_tokens", "all three"]
CASES = RULES + [f"{r} + bias 300" if r != "off" else "bias 300" for r in RULES]


def worker(parent_build):
    """One library, one handle per prompt count; measures what the driver names, one line in, one line out."""
    import time

    import numpy as np

    sys.path.insert(0, ROOT)
    from zig_gpt2_amd import _lib, gpt as zgpt, synth

    if parent_build:  # (a parent build lacks the banned entry points)
        for name in BAN_SYMBOLS:
            _lib.SIGNATURES.pop(name)
    _lib.check(_lib.load().zg_init(0))
    cfg = synth.CONFIGS["124M"]
    V = cfg.vocab_size
    w = synth.make_weights(cfg, seed=0, bf16=True)
    rng = np.random.default_rng(0)
    bias = {int(i): float(v) for i, v in zip(rng.choice(V, 300, replace=False), rng.standard_normal(300) * 2)}
    words = [[int(t) for t in rng.integers(0, V, 2 + k % 3)] for k in range(32)]
    suppress = [int(t) for t in rng.choice(V, 8, replace=False)]
    handles = {}
    print(json.dumps({"ready": True}), flush=True)
    for line in sys.stdin:
        q = json.loads(line)
        n, case, steps = q["prompts"], q["case"], q["steps"]
        if n not in handles:
            kw = {} if parent_build else dict(banned_generate=True)
            handles[n] = zgpt.GPT(cfg, batch=n, sampled_generate=True, edited_generate=True, **kw)
            handles[n].load_weights(w)
        m = handles[n]
        prompts = [synth.rand_tokens(1000 + b, 1, V) for b in range(n)]
        kw = dict(logit_bias=bias) if "bias" in case else {}
        if "ngram" in case or "all three" in case:
            kw["no_repeat_ngram_size"] = 3
        if "words" in case or "all three" in case:
            kw["bad_words_ids"] = words
        if "min_tokens" in case or "all three" in case:
            kw.update(min_tokens=64, suppress_token_ids=suppress)
        t0 = time.perf_counter()
        out = m.generate_sample(prompts, steps, 0.8, seed=q["seed"], **kw)
        dt = time.perf_counter() - t0
        assert out.shape == (n, steps) and (np.asarray(out) < V).all()
        if "min_tokens" in kw:
            assert not np.isin(np.asarray(out[:, 1:65]), suppress).any()
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
                on = [lib for lib in libs if lib == "this" or case in ("off", "bias 300")]
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
                base = "bias 300" if case.endswith("+ bias 300") else "off"
                if case not in ("off", "bias 300"):
                    rec[f"us_per_step_over_{base.split()[0]}"] = round(us[case] - us[base], 2)
                print(json.dumps(rec), flush=True)
    finally:
        for p in procs.values():
            p.stdin.close()
        for p in procs.values():
            p.wait()


if __name__ == "__main__":
    main()
