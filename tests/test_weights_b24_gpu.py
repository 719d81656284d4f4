"""ZG_GPT_WEIGHTS_B24: the matrices stored as 24-bit floats (each fp32 weight rounded to nearest even at 16 mantissa bits,
rows of [upper halves | low bytes]).  round_b24(W) below is W with its six matrices rounded by synth.round_b24, the exact values
such a handle holds (vectors stay fp32), so:
  * against the oracle on round_b24(W), a B24 handle loaded with unrounded W must hold north_star's 1e-3 at every position;
  * against an fp32-storage handle loaded with round_b24(W) it must be BITWISE equal: after the load the decode kernels run the
    fp32 kernels' arithmetic, and the whole-prompt pass multiplies the same weight planes;
  * on a real-style checkpoint (unrounded N(0, 0.02^2) weights, where bf16 storage leaves the bound: test_weight_storage_gpu.py)
    it stays within 1e-4 of the logit scale of the fp32 oracle, every argmax the oracle's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle
from golden_io import assert_greedy_ids_match, assert_model_close
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth, weights_io

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zig_gpt2_amd", "bin", "zgpt2_main")
ZG_ERR_ARG = -6


def round_b24(w):
    return {k: (synth.round_b24(v) if np.ndim(v) == 2 else v) for k, v in w.items()}


def make(cfg, w, **kw):
    m = zgpt.GPT(cfg, **kw)
    m.load_weights(w)
    return m


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def w124():
    return synth.make_weights(synth.CONFIGS["124M"], seed=24, bf16=False)


@pytest.mark.parametrize("name", ["tiny", "tiny3", "xl-slice", "medium-slice", "max-slice"])
@pytest.mark.parametrize("batch,use_graph", [(1, True), (1, False), (3, True), (8, True)])
def test_b24_handle_matches_oracle_on_the_rounded_values(zg, name, batch, use_graph):
    cfg = synth.CONFIGS[name]
    w = synth.make_weights(cfg, seed=31, bf16=False)
    wr = round_b24(w)
    assert not np.array_equal(w["h0.c_attn_w"], wr["h0.c_attn_w"])  # the handle really rounds
    m = make(cfg, w, batch=batch, weights_b24=True, use_graph=use_graph)
    T = cfg.context_size
    toks = np.stack([synth.rand_tokens(500 + b, T, cfg.vocab_size) for b in range(batch)])
    exp = [oracle.GPT(cfg, wr).forced_logits(toks[b], 0) for b in range(batch)]
    for t in range(1, T + 1):
        lg = m.forward(t, [int(toks[b, t - 1]) for b in range(batch)])
        for b in range(batch):
            assert_model_close(exp[b][t - 1], lg[b], f"{name} x{batch} row {b} position {t}")
    prompts = [synth.rand_tokens(600 + b, 1 + (b % 3) * 2, cfg.vocab_size) for b in range(batch)]
    ids = m.generate(prompts, T)
    for b in range(batch):
        ids_ref, lg_ref = oracle.GPT(cfg, wr).generate_greedy(prompts[b], T, want_logits=True)
        top = np.sort(lg_ref, axis=1)
        n = len(prompts[b])
        assert np.array_equal(ids[b, :n], prompts[b])
        assert_greedy_ids_match(ids_ref[n:], ids[b, n:], top[:, -1], top[:, -2], f"{name} x{batch} row {b}")
    m.close()


@pytest.mark.parametrize("batch", [1, 4])
def test_logits_bitwise_equal_to_fp32_storage_of_the_same_values(zg, w124, batch):
    cfg = synth.CONFIGS["124M"]
    edges = (1, 64, 65, 256, 257)
    toks = np.stack([synth.rand_tokens(41 + b, max(edges), cfg.vocab_size) for b in range(batch)])
    got = {}
    for kind, kw, w in (("b24", {"weights_b24": True}, w124), ("f32", {"weights_f32": True}, round_b24(w124))):
        m = make(cfg, w, batch=batch, prefill=False, **kw)
        got[kind] = {}
        for t in range(1, max(edges) + 1):
            lg = m.forward(t, [int(toks[b, t - 1]) for b in range(batch)], want_logits=t in edges)
            if t in edges:
                got[kind][t] = lg
        m.close()
    for t in edges:
        assert np.isfinite(got["b24"][t]).all(), t
        assert same_bits(got["b24"][t], got["f32"][t]), (batch, t, np.abs(got["b24"][t] - got["f32"][t]).max())


def test_generation_identical_to_fp32_storage_of_the_same_values(zg, w124):
    cfg = synth.CONFIGS["124M"]
    out = {}
    for kind, kw, w in (("b24", {"weights_b24": True}, w124), ("f32", {"weights_f32": True}, round_b24(w124))):
        m = make(cfg, w, **kw)
        greedy = m.generate([synth.rand_tokens(7, 1, cfg.vocab_size)], cfg.context_size)
        sampled = m.generate_sample([synth.rand_tokens(8, 3, cfg.vocab_size)], 300, 0.9, seed=5)
        prompt = synth.rand_tokens(9, 300, cfg.vocab_size)
        with_prompt = m.generate([prompt], 600)  # the whole-prompt pass, then decode
        lg = m.prefill(prompt[None, :200])
        nxt = m.forward(201, [int(prompt[200])])
        m.close()
        out[kind] = (greedy, sampled, with_prompt, lg, nxt)
    for a, b in zip(out["b24"], out["f32"]):
        assert same_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b)


def test_real_style_checkpoint_inside_the_bound(zg):
    """test_weight_storage_gpu.py's measurement with B24 storage: 124M, unrounded N(mean, 0.02^2) weights, 64 teacher-forced
    positions against the fp32 oracle.  Each weight is off by at most 2^-17 relative, which moves the logits by ~2e-5 of their
    scale (the largest |logit|, test_weight_storage_gpu.py's measure; bf16 storage: 6e-3): asserted <= 1e-4, ten times inside
    north_star's 1e-3, with every argmax the oracle's.  The element-wise metric with its near-zero floor of 1e-5 rms is an
    fp32-grade yardstick (measured 8e-3, like the two-plane prompt pass of DESIGN.md §4): printed, not asserted."""
    cfg = synth.CONFIGS["124M"]
    w = synth.make_weights(cfg, seed=11, bf16=False)
    prompt = synth.rand_tokens(77, 1, cfg.vocab_size)
    m = make(cfg, w, weights_b24=True)
    ref = oracle.GPT(cfg, w)
    worst_rms, worst_scale, worst_elem, same = 0.0, 0.0, 0.0, 0
    tok = int(prompt[0])
    n = 64
    for s in range(n):
        exp = np.asarray(ref.forward(s + 1, tok), np.float64)
        got = np.asarray(m.forward(s + 1, [tok])[0], np.float64)
        err = np.abs(exp - got)
        rms = float(np.sqrt(np.mean(exp * exp)))
        worst_rms = max(worst_rms, float(err.max()) / rms)
        worst_scale = max(worst_scale, float(err.max() / np.abs(exp).max()))
        worst_elem = max(worst_elem, float((err / np.maximum(np.abs(exp), 1e-2 * rms)).max()))
        same += int(np.argmax(exp) == np.argmax(got))
        tok = int(np.argmax(exp))
    m.close()
    print(f"unrounded 124M weights, 64 positions, B24 storage: {worst_scale:.2e} of the logit scale (max |logit|), {worst_rms:.2e} of "
          f"the logit rms, element-wise (floor 1e-2 rms) {worst_elem:.2e}, argmax agreement {same / n:.3f}")
    assert worst_scale <= 1e-4 and same == n


def test_decode_routes_take_the_b24_kernels(zg, w124):
    cfg = synth.CONFIGS["124M"]
    m = make(cfg, w124, weights_b24=True)
    sym = C.create_string_buffer(160)
    names = {}
    for cls in (1, 3, 4, 5, 6):
        m.time_kernel(cls, 16, at=300)
        _lib.check(_lib.load().zg_debug_last_kernel(sym, 160))
        names[cls] = sym.value.decode()
    m.close()
    assert names[1].startswith("attn_qkv_kernel<b24,"), names
    for cls in (3, 4, 5, 6):
        assert "<b24," in names[cls], names


def test_surface(zg, w124):
    cfg = synth.CONFIGS["124M"]
    with pytest.raises(_lib.ZgError) as e:
        zgpt.GPT(cfg, weights_f32=True, weights_b24=True)
    assert e.value.code == ZG_ERR_ARG
    m = zgpt.GPT(cfg, weights_b24=True)
    E, L, V = cfg.n_embed, cfg.n_layer, cfg.vocab_size
    assert m.step_bytes(10)[0] == 3 * (12 * L * E * E + V * E)
    m.close()
    cfg = synth.CONFIGS["tiny3"]
    w = synth.make_weights(cfg, seed=5, bf16=False)
    owner = make(cfg, w, weights_b24=True)
    for kw in ({}, {"weights_f32": True}):  # another layout of the weight region
        with pytest.raises(_lib.ZgError) as e:
            zgpt.GPT(cfg, share_weights_with=owner, **kw)
        assert e.value.code == ZG_ERR_ARG
    plain = make(cfg, synth.make_weights(cfg, seed=5, bf16=True))
    with pytest.raises(_lib.ZgError) as e:
        zgpt.GPT(cfg, weights_b24=True, share_weights_with=plain)
    assert e.value.code == ZG_ERR_ARG
    plain.close()
    borrower = zgpt.GPT(cfg, weights_b24=True, share_weights_with=owner, own_stream=True)
    prompt = [synth.rand_tokens(3, 2, cfg.vocab_size)]
    a = owner.generate(prompt, cfg.context_size)
    b = borrower.generate(prompt, cfg.context_size)
    assert np.array_equal(a, b)
    assert np.array_equal(a, oracle.GPT(cfg, round_b24(w)).generate_greedy(prompt[0], cfg.context_size)[None])
    borrower.close()
    owner.close()


class _DevMem:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


@pytest.mark.parametrize("name", ["tiny3", "124M"])
def test_receiver_of_the_region_rederives_and_matches(zg, name):
    """test_receiver_gpu.py for B24 handles: a handle that never loads weights gets the sender's region by a device copy (and
    one that ran with other weights before); it must re-derive c2 / c3 from the B24 values and generate the sender's tokens."""
    cfg = synth.CONFIGS[name]
    w = synth.make_weights(cfg, seed=41, bf16=False)
    steps = min(cfg.context_size, 192)
    prompts = [synth.rand_tokens(410, 3, cfg.vocab_size)]
    a = make(cfg, w, weights_b24=True)
    b = make(cfg, synth.make_weights(cfg, seed=42, bf16=False), weights_b24=True)
    b.generate(prompts, 8)  # ran with its own weights: its folded vectors belong to those
    pa, na = a.weight_arena()
    pb, nb = b.weight_arena()
    assert na == nb
    src = torch.as_tensor(_DevMem(pa, na), device="cuda")
    dst = torch.as_tensor(_DevMem(pb, nb), device="cuda")
    torch.cuda.synchronize()
    dst.copy_(src)
    torch.cuda.synchronize()
    assert np.array_equal(a.generate(prompts, steps), b.generate(prompts, steps))
    assert same_bits(a.forward(1, [int(prompts[0][0])]), b.forward(1, [int(prompts[0][0])]))
    toks = synth.rand_tokens(420, 12, cfg.vocab_size)[None]
    assert same_bits(a.prefill(toks), b.prefill(toks))
    a.close()
    b.close()


def test_host_program_model_tier_with_b24(zg, tmp_path):
    cfg = synth.CONFIGS["tiny3"]
    w = synth.make_weights(cfg, seed=43, bf16=False)
    d = str(tmp_path / "raw")
    weights_io.save_raw_dir(d, cfg, w)
    prompt = synth.rand_tokens(431, 3, cfg.vocab_size)
    args = [BIN, "tiny3", d, ",".join(str(int(t)) for t in prompt), "40", "--model-tier", "--weights-b24"]
    env = dict(os.environ, ZGPT2_STAGING_MB="64")
    out = subprocess.run(args, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr
    ids = np.array([int(t) for t in out.stdout.split()], dtype=np.uint64)
    m = zgpt.GPT.from_raw_dir(d, cfg, weights_b24=True)
    assert np.array_equal(ids, m.generate([prompt], 40)[0].astype(np.uint64))
    m.close()
    # the flag needs a raw directory and the model tier (or --gpus)
    bad = subprocess.run([BIN, "tiny3", "43", "1,2", "8", "--model-tier", "--weights-b24"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2
