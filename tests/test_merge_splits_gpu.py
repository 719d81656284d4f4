"""The head merge in front of attn c_proj at batch 1, specialised by split count (gemv_ksplit.hip: exactly NS partials per chunk, the
(m, l) words through wave-uniform loads), against the four-slot prologue it replaces on the default path, which stays reachable as
ZGPT2_DECODE_PATHS_OFF bit 128 (and against bit 256: specialised, but every lane loads its own (m, l)).  The specialisation leaves
out terms that added fmaf(0, finite, r) == r, so every result must be BITWISE the generic prologue's: logits compared as uint32 at the split boundaries (256 positions per split) and the bucket edges
next to them, eager and by graph replay, at the three alignments a wave's K quarter can have with 64-wide heads — inside one head
(E = 128), straddling (E = 384), whole heads (E = 768) — and the flagship's neighbour E = 1024; fp32 and B24 weights; a greedy run.

The embed step kernel now takes what its first loads are addressed by as leading scalar parameters; its three token modes are
held to the tokens recorded in tests/golden/gpt_tiny.npz (greedy, forced) and to the host loop over the per-token sampler."""
import ctypes as C

import numpy as np
import pytest

from golden_io import assert_greedy_ids_match, load_gpt
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 255, 256, 257, 512, 513, 768, 769, 1024)
PATHS = {"by split count": None, "four slots": "128", "vector (m, l)": "256"}  # (256: by split count, every lane loads its own (m, l))
CTX, VOCAB = 1024, 257
HEADS_PER_QUARTER = {128: 1, 384: 2, 768: 3, 1024: 4}  # the most heads a wave's K quarter touches: the kernel's NH


def config(width, n_layer=1):
    return synth.GPTConfig(VOCAB, CTX, n_layer, width // 64, width)


def make(monkeypatch, path, cfg, w, **kw):
    monkeypatch.delenv("ZGPT2_DECODE_PATHS_OFF", raising=False)
    if PATHS[path] is not None:
        monkeypatch.setenv("ZGPT2_DECODE_PATHS_OFF", PATHS[path])
    m = zgpt.GPT(cfg, **kw)
    m.load_weights(w)
    return m


def class3_symbol(m, at):
    m.time_kernel(3, 64, at=at)
    sym = C.create_string_buffer(160)
    _lib.check(_lib.load().zg_debug_last_kernel(sym, 160))
    return sym.value.decode()


def logits_at_lengths(monkeypatch, cfg, w, **kw):
    """{path: {t: logits}}: the cache filled by one whole-prompt pass, then one decode step at every length of LENGTHS."""
    toks = synth.rand_tokens(43, CTX, cfg.vocab_size)
    got = {}
    for path in PATHS:
        m = make(monkeypatch, path, cfg, w, **kw)
        m.prefill(toks[None, : CTX - 1], compute_logits=False)  # (the step at 1024 writes the last position itself, as every step does)
        got[path] = {t: m.forward(t, [int(toks[t - 1])]) for t in LENGTHS}
        m.close()
    return got


def assert_bitwise(got):
    for t in LENGTHS:
        a = got["by split count"][t]
        assert np.isfinite(a).all(), t
        for other in ("four slots", "vector (m, l)"):
            b = got[other][t]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (other, t, np.abs(a - b).max())


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("width", [128, 384, 768, 1024])
def test_logits_bitwise_at_split_boundaries(zg, monkeypatch, width, use_graph):
    cfg = config(width)
    w = synth.make_weights(cfg, seed=300 + width, bf16=True)
    assert_bitwise(logits_at_lengths(monkeypatch, cfg, w, use_graph=use_graph))


@pytest.mark.parametrize("width", [128, 384, 768, 1024])
def test_each_path_runs_its_own_instantiation(zg, monkeypatch, width):
    cfg = config(width)
    w = synth.make_weights(cfg, seed=300 + width, bf16=True)
    for path in PATHS:
        m = make(monkeypatch, path, cfg, w)
        for at, ns in ((200, 1), (257, 2), (700, 3), (1024, 4)):
            want = {"by split count": (ns, HEADS_PER_QUARTER[width]), "four slots": (5, 0), "vector (m, l)": (ns, 0)}[path]
            assert class3_symbol(m, at) == "gemv_ksplit_kernel<unsigned short, 16, 2, 2, %d, %d>" % want, (path, at)
        m.close()


@pytest.mark.parametrize("width,kw", [(384, {"weights_f32": True}), (768, {"weights_b24": True})], ids=["fp32-384", "b24-768"])
def test_logits_bitwise_with_other_weight_formats(zg, monkeypatch, width, kw):
    cfg = config(width)
    w = synth.make_weights(cfg, seed=17, bf16=False)  # not bf16-representable: the fp32 / B24 kernels' own values
    assert_bitwise(logits_at_lengths(monkeypatch, cfg, w, **kw))


def test_greedy_full_context_identical(zg, monkeypatch):
    cfg = config(768, n_layer=2)
    w = synth.make_weights(cfg, seed=19, bf16=True)
    prompt = [synth.rand_tokens(7, 1, cfg.vocab_size)]
    ids = {}
    for path in PATHS:
        m = make(monkeypatch, path, cfg, w, prefill=False)
        ids[path] = m.generate(prompt, CTX)
        m.close()
    assert np.array_equal(ids["by split count"], ids["four slots"])
    assert np.array_equal(ids["by split count"], ids["vector (m, l)"])


def test_embed_step_modes_give_the_recorded_tokens(zg):
    """Mode 0 (greedy generation), mode 1 (forced tokens, the pick read back by argmax) against the tokens recorded for `tiny`;
    mode 2 (the sampler's draw takes the pick's place) against the host loop that feeds the draws back as forced tokens."""
    cfg, g = load_gpt("tiny")
    w = synth.make_weights(cfg, seed=int(g["weight_seed"]), bf16=True)
    n_steps, n_prompt = len(g["out_tokens"]), len(g["prompt"])
    want = g["out_tokens"][n_prompt:]
    for use_graph in (True, False):
        m = zgpt.GPT(cfg, use_graph=use_graph)
        m.load_weights(w)
        ids = m.generate([g["prompt"]], n_steps)[0]  # mode 0
        assert np.array_equal(ids[:n_prompt], g["prompt"])
        assert_greedy_ids_match(want, ids[n_prompt:], g["top1"], g["top2"], "mode 0")
        forced = []
        for s in range(n_steps):  # mode 1: step s feeds fed[s]; from the step that feeds the last prompt token again, its pick is column s
            m.forward(s + 1, [int(g["fed"][s])], compute_logits=s >= n_prompt, want_logits=False)
            if s >= n_prompt:
                forced.append(int(m.argmax()[0]))
        assert_greedy_ids_match(want, forced, g["top1"], g["top2"], "mode 1")
        temp, seed = 0.8, 5  # mode 2
        drawn = m.generate_sample([g["prompt"]], n_steps, temp, seed=seed)[0]
        host = list(int(t) for t in g["prompt"])
        tok = int(g["prompt"][-1])
        for s in range(n_prompt):
            m.forward(s + 1, [int(g["prompt"][s])], compute_logits=False)
        for s in range(n_prompt, n_steps):
            tok = int(m.sample(s + 1, [tok], temp, seed=seed)[0])
            host.append(tok)
        m.close()
        assert np.array_equal(drawn, np.asarray(host, np.uint64)), np.argwhere(drawn != np.asarray(host, np.uint64))[:4]
