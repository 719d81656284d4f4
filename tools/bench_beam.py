#!/usr/bin/env python3
"""Beam search in the device loop at 124M: 1024 steps on a handle of 8, num_beams 4 (two groups) and 8 (one group).

For each W: steps/s of the beam generation and of the SAME build's greedy generation with logprobs = 2 W — the chain without the
beam launch and the cache fork —, the microseconds a step the two launches add, and the mean rows forked per step, taken from the
recorded parents.  The worst case of the fork by itself: 7 of 8 rows copied at cached length 1023 (zg_gpt_kv_fork with the table
[0] * 8), microseconds a call.

The untouched paths — the sampled device loop at 1 and 8 prompts — are measured as tools/bench_bans.py measures: a build of the
parent commit (--parent-lib: its libzgpt2_hip.so) and this one as two live worker processes on the same GPU, measuring the same
case in turn — parent, this, this, parent ... — and read against the spread of the parent's own repetitions.

Every case is warmed up once at full length before anything is timed; a time is a host clock around enqueue + fetch.  One JSON
line per case.  python tools/bench_beam.py [--parent-lib PATH] [--steps 1024] [--repeats 7]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEAM_SYMBOLS = ["zg_gpt_kv_fork", "zg_debug_gpt_kv_rows", "zg_gpt_generate_beam_enqueue", "zg_gpt_generate_fetch_beams", "zg_gpt_generate_fetch_beam_trace",
                "zg_debug_beam_check", "zg_debug_beam_rows"]
SHARED = ["sampled 1", "sampled 8"]                      # both builds
OWN = ["greedy lp 8", "beam 4", "greedy lp 16", "beam 8", "fork 7 rows at 1023"]  # this build


def worker(parent_build):
    """One library; measures what the driver names, one line in, one line out."""
    import time

    import numpy as np

    sys.path.insert(0, ROOT)
    from zig_gpt2_amd import _lib, gpt as zgpt, synth

    if parent_build:  # (a parent build lacks the new entry points)
        for name in BEAM_SYMBOLS:
            _lib.SIGNATURES.pop(name)
    lib = _lib.load()
    _lib.check(lib.zg_init(0))
    cfg = synth.CONFIGS["124M"]
    V = cfg.vocab_size
    w = synth.make_weights(cfg, seed=0, bf16=True)
    handles = {}

    def handle(key, batch, **kw):
        if key not in handles:
            handles[key] = zgpt.GPT(cfg, batch=batch, **kw)
            handles[key].load_weights(w)
        return handles[key]

    print(json.dumps({"ready": True}), flush=True)
    for line in sys.stdin:
        q = json.loads(line)
        case, steps = q["case"], q["steps"]
        rec = {}
        if case.startswith("sampled"):
            n = int(case.split()[1])
            m = handle(("sampled", n), n, sampled_generate=True)
            prompts = [synth.rand_tokens(1000 + b, 1, V) for b in range(n)]
            t0 = time.perf_counter()
            out = m.generate_sample(prompts, steps, 0.8, seed=q["seed"])
            rec["s"] = time.perf_counter() - t0
            assert out.shape == (n, steps)
        elif case.startswith("greedy lp"):
            top = int(case.split()[2])
            m = handle("beam", 8, logprobs_generate=True, beam_generate=True)
            prompts = [synth.rand_tokens(1000 + b // (top // 2), 1, V) for b in range(8)]
            t0 = time.perf_counter()
            out = m.generate(prompts, steps, logprobs=top)
            rec["s"] = time.perf_counter() - t0
            assert out[0].shape == (8, steps)
        elif case.startswith("beam"):
            W = int(case.split()[1])
            m = handle("beam", 8, logprobs_generate=True, beam_generate=True)
            prompts = [synth.rand_tokens(1000 + g, 1, V) for g in range(8 // W)]
            t0 = time.perf_counter()
            res = m.beam_search(prompts, steps, W)
            rec["s"] = time.perf_counter() - t0
            assert len(res) == 8 // W and len(res[0][0][0]) == steps - 1
            par, _ = m.generate_fetch_beam_trace(1, steps - 1)
            rec["rows_forked_per_step"] = float((par != np.arange(8)[:, None]).sum()) / (steps - 1)
        else:  # the fork by itself: 7 rows at 1023 cached positions, `reps` calls behind one another
            m = handle("beam", 8, logprobs_generate=True, beam_generate=True)
            m.prefill(np.stack([synth.rand_tokens(2000 + b, 1023, V) for b in range(8)]), compute_logits=False)
            reps = 50
            m.fork_rows([0] * 8)
            _lib.check(lib.zg_synchronize())
            t0 = time.perf_counter()
            for _ in range(reps):
                m.fork_rows([0] * 8)
            _lib.check(lib.zg_synchronize())
            rec["s"] = (time.perf_counter() - t0) / reps
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libzgpt2_hip.so built from the parent commit")
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
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
        us = {}  # this build's median microseconds a step (a call, for the fork), by case
        for case in SHARED + OWN:
            on = [lib for lib in libs if lib == "this" or case in SHARED]
            for lib in on:  # warm-up at full length
                ask(lib, case=case, steps=args.steps, seed=1)
            secs = {lib: [] for lib in on}
            extra = {}
            for r in range(args.repeats):  # interleaved, and whoever went first goes second in the next repetition
                for lib in (on if r % 2 == 0 else on[::-1]):
                    a = ask(lib, case=case, steps=args.steps, seed=2 + r)
                    secs[lib].append(a.pop("s"))
                    extra = a or extra
            rec = {"case": case, "steps": args.steps}
            if case.startswith("fork"):
                rec["us_per_call"] = round(1e6 * statistics.median(secs["this"]), 2)
                rec["us_per_call_all"] = [round(1e6 * v, 2) for v in secs["this"]]
            else:
                for lib in on:
                    rate = [args.steps / v for v in secs[lib]]
                    rec[f"{lib}_steps_s"] = [round(v, 1) for v in rate]
                    rec[f"{lib}_median"] = round(statistics.median(rate), 1)
                if "parent" in on:
                    rate = [args.steps / v for v in secs["parent"]]
                    rec["parent_spread"] = [round(min(rate), 1), round(max(rate), 1)]
                    rec["inside"] = args.steps / statistics.median(secs["this"]) >= min(rate)
                us[case] = 1e6 * statistics.median(secs["this"]) / args.steps
                rec["this_us_per_step"] = round(us[case], 2)
                if case.startswith("beam"):
                    rec["us_per_step_over_greedy_lp"] = round(us[case] - us[f"greedy lp {2 * int(case.split()[1])}"], 2)
                rec.update(extra)
            print(json.dumps(rec), flush=True)
    finally:
        for p in procs.values():
            p.stdin.close()
        for p in procs.values():
            p.wait()


if __name__ == "__main__":
    main()
