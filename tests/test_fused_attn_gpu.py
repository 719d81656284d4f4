"""One sequence: ln_1 + c_attn and the decode attention of a layer as one launch (attn_qkv.hip) against the two launches it
replaces (ZGPT2_DECODE_PATHS_OFF bit 64).  The fused kernel runs the same device code for both roles and hands q and the new
k / v row over as tagged words carrying the values the caches receive, so every result must be BITWISE that of the two-launch
path: logits at the split (256) and bucket (64) edges on the graph and on the eager path, greedy and sampled generation, a
whole-prompt pass followed by decode, and the nano-char / XL shapes."""
import ctypes as C

import numpy as np
import pytest

from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu

EDGES = (1, 2, 64, 65, 255, 256, 257, 512, 1024)
PATHS = {"fused": None, "two launches": "64"}


def make(monkeypatch, path, cfg, w, **kw):
    monkeypatch.delenv("ZGPT2_DECODE_PATHS_OFF", raising=False)
    if PATHS[path] is not None:
        monkeypatch.setenv("ZGPT2_DECODE_PATHS_OFF", PATHS[path])
    m = zgpt.GPT(cfg, **kw)
    m.load_weights(w)
    return m


def class1_symbol(m):
    m.time_kernel(1, 64, at=300)
    sym = C.create_string_buffer(160)
    _lib.check(_lib.load().zg_debug_last_kernel(sym, 160))
    return sym.value.decode()


@pytest.fixture(scope="module")
def w124():
    return synth.make_weights(synth.CONFIGS["124M"], seed=2024, bf16=True)


def test_fused_launch_is_taken_at_batch_1_only(zg, monkeypatch, w124):
    cfg = synth.CONFIGS["124M"]
    m = make(monkeypatch, "fused", cfg, w124)
    assert class1_symbol(m).startswith("attn_qkv_kernel<"), class1_symbol(m)
    m.close()
    m = make(monkeypatch, "two launches", cfg, w124)
    assert class1_symbol(m).startswith("gemv_lnk_kernel<")
    m.close()
    m = make(monkeypatch, "fused", cfg, w124, kv_f16=True)  # another cache: two launches
    assert class1_symbol(m).startswith("gemv_lnk_kernel<")
    m.close()
    m = make(monkeypatch, "fused", cfg, w124, batch=2)  # the lock-step batch: two launches
    assert not class1_symbol(m).startswith("attn_qkv_kernel<")
    m.close()


def test_fused_launch_at_xl_shapes_and_on_a_private_stream(zg, monkeypatch):
    """GPT-2 XL's fused grid (600 c_attn + 25 heads x splits attention workgroups) does not fit the chip at once: it still takes
    the fused launch, which is correct because every XCD places all c_attn workgroups before its attention workgroups (and faster:
    profiles/round7_fused_attn_other_configs.json).  A handle on a private stream (a co-running group) takes it too."""
    cfg = synth.CONFIGS["xl-slice"]
    w = synth.make_weights(cfg, seed=13, bf16=True)
    prompt = [synth.rand_tokens(15, 2, cfg.vocab_size)]
    ids = {}
    for path in PATHS:
        m = make(monkeypatch, path, cfg, w, prefill=False)
        want = "attn_qkv_kernel<" if path == "fused" else "gemv_lnk_kernel<"
        assert class1_symbol(m).startswith(want), class1_symbol(m)
        ids[path] = m.generate(prompt, cfg.context_size)
        m.close()
    assert np.array_equal(ids["fused"], ids["two launches"])
    cfg = synth.CONFIGS["nano-char"]
    w = synth.make_weights(cfg, seed=14, bf16=True)
    m = make(monkeypatch, "fused", cfg, w, prefill=False, own_stream=True)
    assert class1_symbol(m).startswith("attn_qkv_kernel<"), class1_symbol(m)
    m.close()


@pytest.mark.parametrize("use_graph", [True, False])
def test_logits_bitwise_at_split_and_bucket_edges(zg, monkeypatch, w124, use_graph):
    cfg = synth.CONFIGS["124M"]
    toks = synth.rand_tokens(41, cfg.context_size, cfg.vocab_size)
    got = {}
    for path in PATHS:
        m = make(monkeypatch, path, cfg, w124, use_graph=use_graph, prefill=False)
        got[path] = {}
        for t in range(1, cfg.context_size + 1):
            lg = m.forward(t, [int(toks[t - 1])], want_logits=t in EDGES)
            if t in EDGES:
                got[path][t] = lg
        m.close()
    for t in EDGES:
        a, b = got["fused"][t], got["two launches"][t]
        assert np.isfinite(a).all(), t
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (t, np.abs(a - b).max())


def test_greedy_and_sampled_generation_identical(zg, monkeypatch, w124):
    cfg = synth.CONFIGS["124M"]
    prompt = [synth.rand_tokens(7, 1, cfg.vocab_size)]
    out = {}
    for path in PATHS:
        m = make(monkeypatch, path, cfg, w124, prefill=False)
        greedy = m.generate(prompt, cfg.context_size)
        sampled = m.generate_sample([synth.rand_tokens(8, 3, cfg.vocab_size)], 300, 0.9, seed=5)
        m.close()
        out[path] = (greedy, sampled)
    assert np.array_equal(out["fused"][0], out["two launches"][0])
    assert np.array_equal(out["fused"][1], out["two launches"][1])


def test_prompt_pass_then_decode_identical(zg, monkeypatch, w124):
    cfg = synth.CONFIGS["124M"]
    prompt = synth.rand_tokens(9, 300, cfg.vocab_size)
    out = {}
    for path in PATHS:
        m = make(monkeypatch, path, cfg, w124)
        ids = m.generate([prompt], 600)
        lg = m.prefill(prompt[None, :200])
        nxt = m.forward(201, [int(prompt[200])])
        m.close()
        out[path] = (ids, lg, nxt)
    for a, b in zip(out["fused"], out["two launches"]):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


@pytest.mark.parametrize("name,n", [("nano-char", 256), ("xl", 80)])
def test_other_shapes_identical(zg, monkeypatch, name, n):
    cfg = synth.CONFIGS[name]
    w = synth.make_weights(cfg, seed=11, bf16=True)
    prompt = [synth.rand_tokens(12, 2, cfg.vocab_size)]
    out = {}
    for path in PATHS:
        m = make(monkeypatch, path, cfg, w, prefill=False)
        ids = m.generate(prompt, n)
        lg = m.forward(n // 2, [3])
        m.close()
        out[path] = (ids, lg)
    assert np.array_equal(out["fused"][0], out["two launches"][0])
    assert np.array_equal(out["fused"][1].view(np.uint32), out["two launches"][1].view(np.uint32))
