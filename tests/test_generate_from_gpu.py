"""zg_gpt_generate_from_enqueue on a real MI355X: generate (src/main.zig:322-342) entered at position past_len of a sequence the
handle already holds — the second turn of a conversation.

Greedy: after generate(prompts, n1), generate_from(n1, turn2, n2) must give the tokens an uninterrupted generation over everything
fed so far gives: with F the tokens actually fed at positions < n1 (the prompt, its last token again, then the picks), the tokens of
positions >= n1 equal generate(F ++ turn2, n1 + n2)[n1:] on a fresh handle, and the oracle's.  Sampled: exactly the tokens of the
host loop extend + zg_gpt_sample per position, the equality include/zgpt2.h promises for zg_gpt_generate_sample*."""
import numpy as np
import pytest

import oracle
from golden_io import assert_greedy_ids_match
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu


def make(cfg, w, **kw):
    m = zgpt.GPT(cfg, **kw)
    m.load_weights(w)
    return m


def fed_tokens(prompt, out, n1):
    """The tokens generate fed at positions 0 .. n1 - 1: prompt, its last token again, then the picks (out = its result row)."""
    prompt = [int(t) for t in prompt]
    return np.array([prompt[s] if s < len(prompt) else prompt[-1] if s == len(prompt) else int(out[s - 1]) for s in range(n1)], np.uint64)


def second_turn_matches(cfg, w, prompts, turns, n1, n2, **kw):
    B = len(prompts)
    m = make(cfg, w, batch=B, **kw)
    out1 = m.generate(prompts, n1)
    assert m.cached_len() == n1
    out2 = m.generate_from(n1, turns, n2)
    assert m.cached_len() == n1 + n2
    assert np.array_equal(m.generate_fetch_range(0, n1), out1), "the first turn's tokens must stay"
    m.close()
    full = [np.concatenate([fed_tokens(prompts[b], out1[b], n1), np.asarray(turns[b], np.uint64)]) for b in range(B)]
    fresh = make(cfg, w, batch=B)
    whole = fresh.generate(full, n1 + n2)
    fresh.close()
    for b in range(B):
        nt = len(turns[b])
        assert np.array_equal(out2[b, :nt], turns[b]), f"row {b}: the fed tokens come back"
        ids_ref, lg = oracle.GPT(cfg, w).generate_greedy(full[b], n1 + n2, want_logits=True)
        top = np.sort(lg, axis=1)
        k = min(nt, n2)
        assert_greedy_ids_match(ids_ref[n1 + k:], out2[b, k:], top[:, -1], top[:, -2], f"row {b} against the oracle")
        assert_greedy_ids_match(ids_ref[n1 + k:], whole[b, n1 + k:], top[:, -1], top[:, -2], f"row {b}: uninterrupted generation against the oracle")
        assert_greedy_ids_match(whole[b, n1 + k:], out2[b, k:], top[:, -1], top[:, -2], f"row {b} against the uninterrupted generation")
    return out2


# n1 = 21 and 37 are no multiples of the graphs' 8 steps: single steps until aligned; tiny 21 + 43 and nano-char 90 + 166 run to full context
@pytest.mark.parametrize("name,batch,n1,n2", [("tiny", 1, 21, 43), ("tiny", 4, 16, 30), ("nano-char", 1, 90, 166), ("nano-char", 4, 37, 80)])
def test_greedy_second_turn(zg, name, batch, n1, n2):
    cfg = synth.CONFIGS[name]
    w = synth.make_weights(cfg, seed=191, bf16=True)
    prompts = [synth.rand_tokens(1910 + b, 3 + 4 * b, cfg.vocab_size) for b in range(batch)]  # ragged: 3, 7, 11, 15
    turns = [synth.rand_tokens(1920 + b, 6 + 3 * ((b + 1) % 3), cfg.vocab_size) for b in range(batch)]  # ragged: 9, 12, 6, 9
    second_turn_matches(cfg, w, prompts, turns, n1, n2)


def test_second_turn_without_a_whole_prompt_pass(zg):
    """ZG_GPT_NO_PREFILL handles take the new tokens through the decode loop; so do turns shorter than the pass's threshold."""
    cfg = synth.CONFIGS["tiny"]
    w = synth.make_weights(cfg, seed=192, bf16=True)
    prompts, turns = [synth.rand_tokens(1930, 5, cfg.vocab_size)], [synth.rand_tokens(1931, 9, cfg.vocab_size)]
    a = second_turn_matches(cfg, w, prompts, turns, 20, 30, prefill=False)
    b = second_turn_matches(cfg, w, prompts, turns, 20, 30)
    ids_ref, lg = oracle.GPT(cfg, w).generate_greedy(np.concatenate([fed_tokens(prompts[0], make_first(cfg, w, prompts, 20), 20), turns[0]]), 50,
                                                     want_logits=True)
    top = np.sort(lg, axis=1)
    assert_greedy_ids_match(b[0, 9:], a[0, 9:], top[:, -1], top[:, -2], "prefill=False against a prefill handle")
    second_turn_matches(cfg, w, prompts, [turns[0][:2]], 20, 30)


def make_first(cfg, w, prompts, n1):
    m = make(cfg, w, batch=len(prompts))
    out = m.generate(prompts, n1)[0]
    m.close()
    return out


@pytest.mark.parametrize("top_k,top_p", [(0, 1.0), (5, 0.9)])
def test_sampled_second_turn_equals_host_loop(zg, top_k, top_p):
    cfg = synth.CONFIGS["tiny3"]
    w = synth.make_weights(cfg, seed=193, bf16=True)
    B, p, n, temp, seed = 2, 13, 30, 0.8, 77
    past = np.stack([synth.rand_tokens(1940 + b, p, cfg.vocab_size) for b in range(B)])
    turn = np.stack([synth.rand_tokens(1950 + b, 6, cfg.vocab_size) for b in range(B)])
    m = make(cfg, w, batch=B)
    m.prefill(past, compute_logits=False)
    got = m.generate_from(p, list(turn), n, temp=temp, seed=seed, top_k=top_k, top_p=top_p)
    # the host loop: the turn in one pass, its last token again, then the draws
    m.prefill(past, compute_logits=False)
    m.extend(p, turn, compute_logits=False)
    want = np.zeros_like(got)
    want[:, :6] = turn
    tok = turn[:, -1].copy()
    for s in range(p + 6, p + n):
        tok = m.sample(s + 1, tok, temp, seed=seed, top_k=top_k, top_p=top_p)
        want[:, s - p] = tok
    m.close()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


def test_fetch_range_agrees_with_fetch(zg):
    cfg = synth.CONFIGS["tiny"]
    w = synth.make_weights(cfg, seed=194, bf16=True)
    m = make(cfg, w, batch=2)
    out = m.generate([synth.rand_tokens(1960, 3, cfg.vocab_size), synth.rand_tokens(1961, 5, cfg.vocab_size)], 40)
    assert np.array_equal(m.generate_fetch(40), out)
    assert np.array_equal(m.generate_fetch_range(0, 40), out)
    assert np.array_equal(m.generate_fetch_range(7, 20), out[:, 7:27])
    assert m.generate_fetch_range(64, 0).shape == (2, 0)
    m.close()
