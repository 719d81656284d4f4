"""The consumer side of the hand-over inside the fused ln_1 + c_attn + attention launch (attn_qkv.hip, attn_decode.h): the attention
workgroups poll the tagged (value, tag) words of q — and, in the wave that holds row T - 1, of the new k / v row — with 16-byte
loads, two words each (ZGPT2_DECODE_PATHS_OFF bit 1024 set: with 8-byte loads, as before; the handle reads the bit once at create).
The wider load may not change a result bit: logits are held BITWISE equal between the default, bit 1024, bits 512 + 1024 (the
hand-over as it was before both sides were changed) and the two-launch path (bit 64), which runs the same attention body with
FUSED == false.

The holder wave takes the new row from the words of its lanes' group g = (T - 1) % 4 and keeps it in slot i = (T - 1) % 64 / 4 of
its 64 positions: the tiny model (context 64) therefore runs EVERY T from 1 to 64, which puts the new row in each of the 64 (i, g)
slots once — an edge list cannot see a wrong slot.  124M: 65 .. 257 put the holder in waves 1, 2 and 3 and on split and bucket
edges; 1024 (whole-prompt pass + one step) is the last wave of the last split."""
import numpy as np
import pytest

from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu

PATHS = {"default": None, "8-byte poll": "1024", "8-byte poll, tag stored last": "1536", "two launches": "64"}
EDGES_124M = (65, 128, 129, 192, 193, 255, 256, 257)


def make(monkeypatch, off, cfg, w, **kw):
    monkeypatch.delenv("ZGPT2_DECODE_PATHS_OFF", raising=False)
    if off is not None:
        monkeypatch.setenv("ZGPT2_DECODE_PATHS_OFF", off)
    m = zgpt.GPT(cfg, **kw)  # (the bit is read once, here)
    m.load_weights(w)
    return m


@pytest.fixture(scope="module")
def w124():
    return synth.make_weights(synth.CONFIGS["124M"], seed=2026, bf16=True)


def logits_at(m, toks, wanted, far=None):
    """Decode steps 1 .. max(wanted) one by one; `far`: then a whole-prompt pass over far - 1 tokens and the decode step at far."""
    got = {}
    for t in range(1, max(wanted) + 1):
        lg = m.forward(t, [int(toks[t - 1])], want_logits=t in wanted)
        if t in wanted:
            got[t] = lg.copy()
    if far:
        m.prefill(toks[None, : far - 1])
        got[far] = m.forward(far, [int(toks[far - 1])]).copy()
    return got


def assert_same(got, wanted):
    ref = got["default"]
    for path, g in got.items():
        for t in wanted:
            assert np.isfinite(g[t]).all(), (path, t)
            assert np.array_equal(g[t].view(np.uint32), ref[t].view(np.uint32)), (path, t, float(np.abs(g[t] - ref[t]).max()))


def run_paths(monkeypatch, cfg, w, toks, wanted, far=None, **kw):
    got = {}
    for path, off in PATHS.items():
        m = make(monkeypatch, off, cfg, w, **kw)
        got[path] = logits_at(m, toks, wanted, far=far)
        m.close()
    assert_same(got, tuple(wanted) + ((far,) if far else ()))


@pytest.mark.parametrize("use_graph", [True, False])
def test_tiny_every_slot_bitwise(zg, monkeypatch, use_graph):
    cfg = synth.CONFIGS["tiny"]  # 2 heads, context 64: one split, one wave holds the new row in each of its 64 slots in turn
    w = synth.make_weights(cfg, seed=35, bf16=True)
    toks = synth.rand_tokens(36, cfg.context_size, cfg.vocab_size)
    run_paths(monkeypatch, cfg, w, toks, tuple(range(1, cfg.context_size + 1)), use_graph=use_graph, prefill=False)


@pytest.mark.parametrize("use_graph", [True, False])
def test_124m_logits_bitwise(zg, monkeypatch, w124, use_graph):
    cfg = synth.CONFIGS["124M"]
    toks = synth.rand_tokens(37, cfg.context_size, cfg.vocab_size)
    run_paths(monkeypatch, cfg, w124, toks, EDGES_124M, far=cfg.context_size, use_graph=use_graph)


def test_greedy_generation_identical(zg, monkeypatch, w124):
    cfg = synth.CONFIGS["124M"]
    prompt = [synth.rand_tokens(38, 3, cfg.vocab_size)]
    ids = {}
    for path, off in PATHS.items():
        m = make(monkeypatch, off, cfg, w124, prefill=False)
        ids[path] = m.generate(prompt, 96)
        m.close()
    for path in PATHS:
        assert np.array_equal(ids[path], ids["default"]), path
