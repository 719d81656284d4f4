"""Time zg_gpt_score against the pass it rides on and against the only route there was before it.

usage: python tools/bench_score.py [--model 124M] [--batches 1,8] [--n 1023] [--top-ns 0,5,20]
124M synthetic weights.  For every (batch, top_n), on one handle created with score=True, the best of 5 timed calls after a warm-up:
  score_ms          GPT.score(tokens, top_n=top_n): zg_gpt_score and the fetch of its n columns
  extend_ms         GPT.extend(0, tokens, compute_logits=True) over the same tokens: what the pass costs without scoring
  forward_ms_per_position
                    forward(T, tok, want_logits=True) position by position plus a numpy log-softmax of the row — the route without
                    zg_gpt_score — timed over the first 128 positions and divided by 128
Host wall time around synchronous calls (each drains the stream).  One JSON line in all."""
import argparse
import json
import time

import numpy as np

from zig_gpt2_amd import _lib, gpt as zgpt, synth


def best(run, reps=5):
    t = []
    for _ in range(reps + 1):  # the first round warms up
        t0 = time.perf_counter()
        run()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="124M")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--n", type=int, default=1023)
    ap.add_argument("--top-ns", default="0,5,20")
    a = ap.parse_args()
    cfg = synth.CONFIGS[a.model]
    w = synth.make_weights(cfg, seed=0, bf16=True)
    _lib.check(_lib.load().zg_init(0))
    n = min(a.n, cfg.context_size)
    rows = []
    for batch in (int(x) for x in a.batches.split(",")):
        toks = np.stack([synth.rand_tokens(700 + b, n, cfg.vocab_size) for b in range(batch)])
        m = zgpt.GPT(cfg, batch=batch, score=True)
        m.load_weights(w)
        extend = best(lambda: m.extend(0, toks, compute_logits=True))
        first = min(128, n)

        def per_position():
            for T in range(1, first + 1):
                x = m.forward(T, toks[:, T - 1], want_logits=True).astype(np.float64)
                x -= x.max(axis=1, keepdims=True)
                x -= np.log(np.exp(x).sum(axis=1, keepdims=True))

        forward = best(per_position) / first
        for top_n in (int(x) for x in a.top_ns.split(",")):
            score = best(lambda: m.score(toks, top_n=top_n))
            rows.append({"batch": batch, "n": n, "top_n": top_n, "score_ms": round(score, 3), "extend_ms": round(extend, 3),
                         "forward_ms_per_position": round(forward, 4)})
        m.close()
    print(json.dumps({"model": a.model, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()
