#!/usr/bin/env python3
"""The truncated sampler (zg_gpt_sample_ex: top-k, then top-p over what it kept, then GPT.sample's draw) over random models,
batches, temperatures, k and p against the float64 restatement of its semantics (tests/trunc_ref.py) applied to the oracle's
logits, both sides fed the device's picks.  The device rounds differently from the oracle, so a position is compared only where
the oracle's cuts are wider than the parity bound (k-th / (k+1)-th logit gap > 1e-3 max|logit|, cumulative masses >= 1e-4 from
top_p); there the kept set is the reference's exactly, probabilities agree, and the pick is the reference's except where u x total
lands within 1e-6 of a boundary of its running sum.  Then the device loop (zg_gpt_generate_sample_ex) against the host loop over
the per-token call with the same seed: identical tokens, always.  python tests/sweeps/sample_trunc.py [first_seed] [count]"""
import os, sys, traceback
root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests")); sys.path.insert(0, os.path.join(root, "oracle"))
import numpy as np
import oracle
from golden_io import assert_model_close
from trunc_ref import filter_row, weighted_index
from zig_gpt2_amd import _lib, gpt as zgpt, synth

zg = _lib.load(); _lib.check(zg.zg_init(0))
first, count = (int(v) for v in (sys.argv[1:3] + ["0", "60"][len(sys.argv) - 1:]))
bad = []
compared = 0
for seed in range(first, first + count):
    rng = np.random.default_rng(3000 + seed)
    name = ["tiny", "tiny3", "nano-char", "medium-slice"][int(rng.integers(0, 4))]
    cfg = synth.CONFIGS[name]
    batch = int(rng.integers(1, 9))
    temp = float(rng.choice([0.3, 0.8, 1.0, 1.7, 5.0]))
    k = int(rng.choice([0, 1, 2, 5, 40, cfg.vocab_size - 1, cfg.vocab_size + 3]))
    p = float(np.float32(rng.choice([1.0, 0.95, 0.9, 0.5, 0.1])))
    if k in (0, cfg.vocab_size + 3) and p == 1.0:
        k = 3
    steps = int(rng.integers(1, min(cfg.context_size, 30)))
    what = f"seed {seed}: {name} batch {batch} temp {temp} k {k} p {p} steps {steps}"
    try:
        w = synth.make_weights(cfg, seed=500 + seed, bf16=True)
        m = zgpt.GPT(cfg, batch=batch)
        m.load_weights(w)
        ref = [oracle.GPT(cfg, w) for _ in range(batch)]
        toks = [int(t) for t in rng.integers(0, cfg.vocab_size, batch)]
        near = n_cmp = 0
        for s in range(steps):
            us = rng.random(batch).astype(np.float32)
            got, probs = m.sample(s + 1, toks, temp, uniforms=us, want_probs=True, top_k=k, top_p=p)
            for b in range(batch):
                x = np.asarray(ref[b].forward(s + 1, toks[b], True), np.float32)
                r = filter_row(x, temp, k, p)
                assert int(got[b]) < cfg.vocab_size and probs[b][int(got[b])] > 0, (what, "draw outside the device's kept set")
                assert abs(float(probs[b].sum(dtype=np.float64)) - 1.0) < 1e-5, what
                srt = np.sort(x)[::-1]
                wide = (not 0 < k < cfg.vocab_size or srt[k - 1] - srt[k] > 1e-3 * np.abs(x).max()) and (p == 1.0 or np.abs(r.cum - p).min() >= 1e-4)
                if not wide:
                    continue
                n_cmp += 1
                assert np.array_equal(probs[b] != 0, r.kept | ((probs[b] != 0) & (r.probs < 1e-37))), (what, s, b, "kept set")
                assert_model_close(r.probs, probs[b], what + f" probs step {s} row {b}")
                exp_tok, dist = weighted_index(r.probs, us[b])
                if int(got[b]) != exp_tok:
                    assert dist < 1e-6, (what, s, b, int(got[b]), exp_tok)
                    near += 1
            toks = [int(t) for t in got]
        assert near <= max(2, n_cmp // 20), (what, near)
        compared += n_cmp
        n_gen = min(cfg.context_size, steps + 8)
        prompts = [synth.rand_tokens(9000 + 31 * seed + b, 1 + (seed + b) % 3, cfg.vocab_size) for b in range(batch)]
        got = m.generate_sample(prompts, n_gen, temp, seed=seed, top_k=k, top_p=p)
        want = np.zeros_like(got)
        draws = [0] * batch
        min_np = min(len(q) for q in prompts)
        for s in range(n_gen):
            fed = [int(q[s]) if s < len(q) else (int(q[-1]) if s == len(q) else int(draws[b])) for b, q in enumerate(prompts)]
            if s >= min_np:
                draws = m.sample(s + 1, fed, temp, seed=seed, top_k=k, top_p=p)
            else:
                m.forward(s + 1, fed, compute_logits=False)
            for b, q in enumerate(prompts):
                want[b, s] = fed[b] if s < len(q) else draws[b]
        assert np.array_equal(got, want), (what, "device loop vs host loop", np.argwhere(got != want)[:3].tolist())
        m.close()
    except Exception:
        bad.append(seed)
        print(what)
        traceback.print_exc(limit=1)
print(f"{count} runs from seed {first}: {len(bad)} failed {bad}; {compared} positions compared with the reference")
sys.exit(1 if bad else 0)
