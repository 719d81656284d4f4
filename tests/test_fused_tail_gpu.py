"""The producer side of the hand-over inside the fused ln_1 + c_attn + attention launch (attn_qkv.hip): the c_attn role stores the
tagged word the attention workgroups wait for in FRONT of the q / cache store (ZGPT2_DECODE_PATHS_OFF bit 512 set: behind it, as
before).  The word carries the value the epilogue stores, so no result bit may change: logits are held BITWISE equal between the
default path, bit 512, and the two-launch path (bit 64), which runs the same attention body with FUSED == false.

Sequence lengths (split = 256 positions = 4 waves x 64, bucket = 64): 1, 2 (holder of row T - 1 in wave 0), 63, 64 (T == t_hi on a
bucket edge), 65 (holder in wave 1), 255 / 256 (holder in wave 3, T == t_hi on a split edge), 257 (holder in a second split whose
waves 1 - 3 are idle), 1024 (the last wave of the last split; 124M only)."""
import numpy as np
import pytest

from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu

PATHS = {"default": None, "tag stored last": "512", "two launches": "64"}
EDGES = (1, 2, 63, 64, 65, 255, 256, 257)


def make(monkeypatch, path, cfg, w, **kw):
    monkeypatch.delenv("ZGPT2_DECODE_PATHS_OFF", raising=False)
    if PATHS[path] is not None:
        monkeypatch.setenv("ZGPT2_DECODE_PATHS_OFF", PATHS[path])
    m = zgpt.GPT(cfg, **kw)  # (the bit is read once, here)
    m.load_weights(w)
    return m


@pytest.fixture(scope="module")
def w124():
    return synth.make_weights(synth.CONFIGS["124M"], seed=2025, bf16=True)


def logits_at_edges(m, cfg, toks, edges, far=None):
    """Decode steps 1 .. max(edges) one by one; `far`: then a whole-prompt pass over far - 1 tokens and the decode step at far."""
    got = {}
    for t in range(1, max(edges) + 1):
        lg = m.forward(t, [int(toks[t - 1])], want_logits=t in edges)
        if t in edges:
            got[t] = lg.copy()
    if far:
        m.prefill(toks[None, : far - 1])
        got[far] = m.forward(far, [int(toks[far - 1])]).copy()
    return got


def assert_same(got, edges):
    ref = got["default"]
    for path, g in got.items():
        for t in edges:
            assert np.isfinite(g[t]).all(), (path, t)
            assert np.array_equal(g[t].view(np.uint32), ref[t].view(np.uint32)), (path, t, float(np.abs(g[t] - ref[t]).max()))


@pytest.mark.parametrize("use_graph", [True, False])
def test_tiny_logits_bitwise(zg, monkeypatch, use_graph):
    cfg = synth.CONFIGS["tiny"]  # 2 heads, context 64: one split, every bucket position up to the edge
    w = synth.make_weights(cfg, seed=31, bf16=True)
    toks = synth.rand_tokens(32, cfg.context_size, cfg.vocab_size)
    edges = tuple(t for t in EDGES if t <= cfg.context_size)
    got = {}
    for path in PATHS:
        m = make(monkeypatch, path, cfg, w, use_graph=use_graph, prefill=False)
        got[path] = logits_at_edges(m, cfg, toks, edges)
        m.close()
    assert_same(got, edges)


@pytest.mark.parametrize("use_graph", [True, False])
def test_124m_logits_bitwise(zg, monkeypatch, w124, use_graph):
    cfg = synth.CONFIGS["124M"]
    toks = synth.rand_tokens(33, cfg.context_size, cfg.vocab_size)
    got = {}
    for path in PATHS:
        m = make(monkeypatch, path, cfg, w124, use_graph=use_graph)
        got[path] = logits_at_edges(m, cfg, toks, EDGES, far=cfg.context_size)
        m.close()
    assert_same(got, EDGES + (cfg.context_size,))


def test_greedy_generation_identical(zg, monkeypatch, w124):
    cfg = synth.CONFIGS["124M"]
    prompt = [synth.rand_tokens(34, 3, cfg.vocab_size)]
    ids = {}
    for path in PATHS:
        m = make(monkeypatch, path, cfg, w124, prefill=False)
        ids[path] = m.generate(prompt, 96)
        m.close()
    for path in PATHS:
        assert np.array_equal(ids[path], ids["default"]), path
