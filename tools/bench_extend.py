"""Time zg_gpt_extend (the whole-prompt pass behind cached positions) against what a caller had before it.

usage: python tools/bench_extend.py [--model 124M] [--batches 1,8] [--past 512] [--lengths 16,64,256,511]
For every (batch, n), best of --reps timed calls, each variant in a fresh handle:
  (a) extend(past, n)          behind a prefilled past (the past is rebuilt, untimed, before every timed call)
  (b) prefill(past + n)        from position 0: what a second turn cost so far
  (c) n calls of forward       the per-token route behind the same past
and prefill(n) at offset 0, for comparison with tools/bench_prefill.py of the parent commit.  One JSON line per (batch, n).
Host wall time around synchronous calls (each drains the stream), after one warm-up call per variant.
"""
import argparse
import json
import time

import numpy as np

from zig_gpt2_amd import _lib, gpt as zgpt, synth


def best(reps, setup, run):
    t = []
    for _ in range(reps + 1):  # the first round warms up
        setup()
        t0 = time.perf_counter()
        run()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="124M")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--past", type=int, default=512)
    ap.add_argument("--lengths", default="16,64,256,511")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    cfg = synth.CONFIGS[a.model]
    w = synth.make_weights(cfg, seed=0, bf16=True)
    _lib.check(_lib.load().zg_init(0))
    past = a.past
    for batch in (int(x) for x in a.batches.split(",")):
        for n in (int(x) for x in a.lengths.split(",")):
            n = min(n, cfg.context_size - past)
            toks = np.stack([synth.rand_tokens(900 + b, past + n, cfg.vocab_size) for b in range(batch)])

            def fresh():
                m = zgpt.GPT(cfg, batch=batch)
                m.load_weights(w)
                return m

            def forwards(m):
                for s in range(past, past + n):
                    m.forward(s + 1, toks[:, s], compute_logits=False)

            m = fresh()
            ext = best(a.reps, lambda: m.prefill(toks[:, :past], compute_logits=False), lambda: m.extend(past, toks[:, past:], compute_logits=False))
            m.close()
            m = fresh()
            whole = best(a.reps, lambda: None, lambda: m.prefill(toks, compute_logits=False))
            m.close()
            m = fresh()
            loop = best(a.reps, lambda: m.prefill(toks[:, :past], compute_logits=False), lambda: forwards(m))
            m.close()
            m = fresh()
            at0 = best(a.reps, lambda: None, lambda: m.prefill(toks[:, :n], compute_logits=False))
            m.close()
            print(json.dumps({"model": a.model, "batch": batch, "past": past, "n": n, "extend_ms": round(ext, 3), "prefill_past_plus_n_ms": round(whole, 3),
                              "forward_loop_ms": round(loop, 3), "prefill_n_at_0_ms": round(at0, 3)}), flush=True)


if __name__ == "__main__":
    main()
