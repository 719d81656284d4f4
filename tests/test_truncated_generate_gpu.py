"""Top-k / nucleus truncation through the model tier: zg_gpt_sample_ex and the device loop zg_gpt_generate_sample_ex (graphs of
their own beside the sampled ones).  The device loop equals the host loop over the per-token call token for token; the per-token
call is held to the float64 restatement of the semantics (trunc_ref.py) applied to the ORACLE's logits, teacher-forced on the
device's draws, at positions whose cuts are wider than the project's parity bound (asserted, model seeds chosen on the CPU)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from trunc_ref import filter_row, uniform
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_loop(m, prompts, n_steps, temp, seed, top_k, top_p, probs_of=None):
    """generate's token logic around the per-token truncated sampler (probs_of: a list that receives row 0's probabilities)."""
    B = len(prompts)
    out = np.zeros((B, n_steps), np.uint64)
    draws = [0] * B
    min_np = min(len(p) for p in prompts)
    for s in range(n_steps):
        toks = [int(p[s]) if s < len(p) else (int(p[-1]) if s == len(p) else int(draws[b])) for b, p in enumerate(prompts)]
        if s >= min_np:
            if probs_of is not None:
                draws, pr = m.sample(s + 1, toks, temp, seed=seed, top_k=top_k, top_p=top_p, want_probs=True)
                probs_of.append((s, pr[0].copy()))
            else:
                draws = m.sample(s + 1, toks, temp, seed=seed, top_k=top_k, top_p=top_p)
        else:
            m.forward(s + 1, toks, compute_logits=False)
        for b, p in enumerate(prompts):
            out[b, s] = toks[b] if s < len(p) else draws[b]
    return out


@pytest.mark.parametrize("at_create", [False, True])
@pytest.mark.parametrize("name,batch,graph", [("tiny", 1, True), ("tiny3", 3, True), ("tiny", 8, True), ("nano-char", 2, False)])
def test_device_loop_equals_host_loop(zg, name, batch, graph, at_create):
    cfg = synth.CONFIGS[name]
    w = synth.make_weights(cfg, seed=61, bf16=True)
    prompts = [synth.rand_tokens(610 + b, 1 + b % 3, cfg.vocab_size) for b in range(batch)]
    n_steps = min(cfg.context_size, 70)
    for temp, seed, k, p in ((0.8, 5, 7, 1.0), (1.7, 123456789, 0, 0.9), (0.8, 9, 12, 0.8)):
        m = zgpt.GPT(cfg, batch=batch, use_graph=graph, truncated_generate=at_create and graph)
        m.load_weights(w)
        got = m.generate_sample(prompts, n_steps, temp, seed=seed, top_k=k, top_p=p)
        again = m.generate_sample(prompts, n_steps, temp, seed=seed, top_k=k, top_p=p)
        other = m.generate_sample(prompts, n_steps, temp, seed=seed + 1, top_k=k, top_p=p)
        want = host_loop(m, prompts, n_steps, temp, seed, k, p)
        m.close()
        assert np.array_equal(got, again)
        assert np.array_equal(got, want), (k, p, np.argwhere(got != want)[:4])
        assert not np.array_equal(got, other)
        for b, pr in enumerate(prompts):
            assert np.array_equal(got[b, : len(pr)], pr)


def test_filters_off_is_generate_sample(zg):
    cfg = synth.CONFIGS["tiny3"]
    w = synth.make_weights(cfg, seed=64, bf16=True)
    prompts = [synth.rand_tokens(640 + b, 2, cfg.vocab_size) for b in range(3)]
    m = zgpt.GPT(cfg, batch=3)
    m.load_weights(w)
    want = m.generate_sample(prompts, 40, 0.8, seed=3)
    out = np.zeros((3, 40), np.uint64)
    mat, lens, stride = m._prompts(prompts)
    for k in (0, cfg.vocab_size, cfg.vocab_size + 9):  # through the new entry point itself
        opt = _lib.SampleOptions(0.8, k, 1.0)
        _lib.check(zg.zg_gpt_generate_sample_ex(m.h, _lib.ptr(mat), stride, _lib.ptr(lens), 40, C.addressof(opt), 3, _lib.ptr(out), out.size))
        assert np.array_equal(out, want), k
    toks = [int(p[0]) for p in prompts]
    t0, p0 = m.sample(1, toks, 0.8, seed=3, want_probs=True)
    tok = np.zeros(3, np.uint64)
    pr = np.empty((3, cfg.vocab_size), np.float32)
    tk = np.ascontiguousarray(toks, np.uint64)
    opt = _lib.SampleOptions(0.8, 0, 1.0)
    _lib.check(zg.zg_gpt_sample_ex(m.h, 1, _lib.ptr(tk), 3, C.addressof(opt), None, 3, _lib.ptr(tok), _lib.ptr(pr), pr.size))
    m.close()
    assert np.array_equal(tok, t0) and np.array_equal(pr.view(np.uint32), p0.view(np.uint32))


def test_top_k_1_is_greedy(zg):
    for name, batch in (("tiny", 1), ("tiny3", 3)):
        cfg = synth.CONFIGS[name]
        w = synth.make_weights(cfg, seed=65, bf16=True)
        prompts = [synth.rand_tokens(650 + b, 1 + b, cfg.vocab_size) for b in range(batch)]
        m = zgpt.GPT(cfg, batch=batch)
        m.load_weights(w)
        n = min(cfg.context_size, 60)
        got = m.generate_sample(prompts, n, 0.8, seed=1, top_k=1)
        greedy = m.generate(prompts, n)
        m.close()
        assert np.array_equal(got, greedy), np.argwhere(got != greedy)[:4]


def oracle_margins(cfg, w, prompt, toks, temp, k, p):
    """Teacher-forced on `toks`: the oracle's reference filter per sampled position, and whether every cut is wide enough (the
    gap between the k-th and (k+1)-th largest logit > 1e-3 max|logit|; the cumulative masses next to top_p >= 1e-4 away)."""
    ref = oracle.GPT(cfg, w)
    rows, ok = [], True
    for s in range(len(toks)):
        tok = int(prompt[s]) if s < len(prompt) else (int(prompt[-1]) if s == len(prompt) else int(toks[s - 1]))
        logits = ref.forward(s + 1, tok, s >= len(prompt))
        if s < len(prompt):
            continue
        x = np.asarray(logits, np.float32)
        srt = np.sort(x)[::-1]
        ok = ok and (srt[k - 1] - srt[k]) > 1e-3 * np.abs(x).max()
        r = filter_row(x, temp, k, p)
        ok = ok and np.abs(r.cum - p).min() >= 1e-4
        rows.append((s, r))
    return rows, ok


def test_per_token_kept_set_against_the_oracle(zg):
    cfg = synth.CONFIGS["tiny3"]
    prompt = synth.rand_tokens(620, 2, cfg.vocab_size)
    n_steps, temp, seed, k, p = cfg.context_size, 0.8, 77, 9, 0.85
    found = None
    for wseed in range(70, 90):  # a model whose cuts, along the device's own draws, are wider than the parity bound
        w = synth.make_weights(cfg, seed=wseed, bf16=True)
        m = zgpt.GPT(cfg)
        m.load_weights(w)
        probs = []
        got = host_loop(m, [prompt], n_steps, temp, seed, k, p, probs_of=probs)[0]
        dev = m.generate_sample([prompt], n_steps, temp, seed=seed, top_k=k, top_p=p)[0]
        m.close()
        rows, ok = oracle_margins(cfg, w, prompt, got, temp, k, p)
        if ok:
            found = (got, dev, probs, rows)
            break
    assert found is not None, "no model seed in 70..89 keeps every cut clear of the parity bound"
    got, dev, probs, rows = found
    assert np.array_equal(got, dev)
    assert len(rows) == len(probs) == n_steps - len(prompt)
    for (s, r), (s2, pr) in zip(rows, probs):  # every position, none skipped
        assert s == s2
        assert np.array_equal(pr != 0, r.kept), (s, np.flatnonzero((pr != 0) != r.kept)[:5])
        assert r.kept[int(got[s])]


def test_truncated_generation_behind_a_whole_prompt_pass(zg):
    cfg = synth.CONFIGS["tiny3"]
    w = synth.make_weights(cfg, seed=63, bf16=True)
    prompts = [synth.rand_tokens(630 + b, 7, cfg.vocab_size) for b in range(2)]
    n_steps, temp, seed, k, p = 40, 0.8, 31, 10, 0.9
    m = zgpt.GPT(cfg, batch=2)
    m.load_weights(w)
    got = m.generate_sample(prompts, n_steps, temp, seed=seed, top_k=k, top_p=p)
    m.prefill(np.stack(prompts), compute_logits=False)
    want = np.zeros_like(got)
    want[:, :7] = np.stack(prompts)
    toks = [int(pr[-1]) for pr in prompts]
    for s in range(7, n_steps):
        toks = [int(t) for t in m.sample(s + 1, toks, temp, seed=seed, top_k=k, top_p=p)]
        want[:, s] = toks
    m.close()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


def test_top_k_40_top_p_095_at_124m(zg):
    cfg = synth.CONFIGS["124M"]
    w = synth.make_weights(cfg, seed=0, bf16=True)
    prompt = [synth.rand_tokens(1000, 1, cfg.vocab_size)]
    m = zgpt.GPT(cfg)
    m.load_weights(w)
    n = 64
    got = m.generate_sample(prompt, n, 0.8, seed=1, top_k=40, top_p=0.95)
    probs = []
    want = host_loop(m, prompt, n, 0.8, 1, 40, 0.95, probs_of=probs)
    m.close()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    for s, pr in probs:  # the probabilities are those of the step's logits: the 40 largest are the 40 largest probabilities' superset
        kept = np.flatnonzero(pr)
        assert 1 <= kept.size <= 40 and int(got[0, s]) in kept, (s, kept.size)


def test_bad_options_are_refused_and_the_handle_lives(zg):
    cfg = synth.CONFIGS["tiny"]
    w = synth.make_weights(cfg, seed=66, bf16=True)
    prompts = [synth.rand_tokens(660, 2, cfg.vocab_size)]
    m = zgpt.GPT(cfg)
    m.load_weights(w)
    want = m.generate_sample(prompts, 30, 0.8, seed=2, top_k=5, top_p=0.9)
    mat, lens, stride = m._prompts(prompts)
    out = np.zeros((1, 30), np.uint64)
    tok = np.zeros(1, np.uint64)
    one = np.ascontiguousarray([3], np.uint64)
    bad = [(0.0, 1.0), (-1.0, 0.9), (0.8, 0.0), (0.8, -0.1), (0.8, 1.01), (0.8, float("nan"))]
    for temp, p in bad:
        opt = _lib.SampleOptions(temp, 5, p)
        assert zg.zg_gpt_generate_sample_ex(m.h, _lib.ptr(mat), stride, _lib.ptr(lens), 30, C.addressof(opt), 2, _lib.ptr(out), out.size) == -6
        assert zg.zg_gpt_generate_sample_ex_enqueue(m.h, _lib.ptr(mat), stride, _lib.ptr(lens), 30, C.addressof(opt), 2) == -6
        assert zg.zg_gpt_sample_ex(m.h, 1, _lib.ptr(one), 1, C.addressof(opt), None, 2, _lib.ptr(tok), None, 0) == -6
    assert zg.zg_gpt_generate_sample_ex(m.h, _lib.ptr(mat), stride, _lib.ptr(lens), 30, None, 2, _lib.ptr(out), out.size) == -6
    assert zg.zg_gpt_sample_ex(m.h, 1, _lib.ptr(one), 1, None, None, 2, _lib.ptr(tok), None, 0) == -6
    again = m.generate_sample(prompts, 30, 0.8, seed=2, top_k=5, top_p=0.9)
    m.close()
    assert np.array_equal(again, want)


def test_existing_entry_points_after_a_truncated_generation(zg):
    cfg = synth.CONFIGS["tiny3"]
    w = synth.make_weights(cfg, seed=67, bf16=True)
    prompts = [synth.rand_tokens(670 + b, 2, cfg.vocab_size) for b in range(2)]
    n = min(cfg.context_size, 50)
    fresh = zgpt.GPT(cfg, batch=2)
    fresh.load_weights(w)
    greedy, sampled = fresh.generate(prompts, n), fresh.generate_sample(prompts, n, 0.8, seed=4)
    fresh.close()
    m = zgpt.GPT(cfg, batch=2)
    m.load_weights(w)
    m.generate_sample(prompts, n, 0.8, seed=4, top_k=6, top_p=0.9)
    g2 = m.generate(prompts, n)
    m.generate_sample(prompts, n, 0.8, seed=4, top_k=6)
    s2 = m.generate_sample(prompts, n, 0.8, seed=4)
    m.close()
    assert np.array_equal(g2, greedy) and np.array_equal(s2, sampled)


def test_sweep_slice():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sweeps", "sample_trunc.py"), "500", "10"], cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    print(out.stdout.strip().splitlines()[-1])
