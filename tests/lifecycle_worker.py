"""One process of tests/test_lifecycle_gpu.py: zg_init_ex / zg_shutdown / zg_init again, in a process of its own because
zg_shutdown frees what every handle of the process stages through.  Prints one JSON line; the test asserts on it.
usage: lifecycle_worker.py main | bad_device"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from golden_io import assert_ref_close  # noqa: E402
from zig_gpt2_amd import _lib, gpt, ops, synth  # noqa: E402

E, HEADS, T = 128, 2, 6


def z(*shape):
    return np.zeros(shape, np.float32)


def rel_err(exp, got):
    exp, got = np.asarray(exp, np.float64), np.asarray(got, np.float64)
    return float(np.abs(exp - got).max() / max(np.abs(exp).max(), 1e-30))


def close(exp, got, what):
    """golden_io.assert_ref_close with the floor test_ops_gpu.py gives seeded inputs: "" when it holds, else its message."""
    try:
        assert_ref_close(exp, got, what, scale_floor=2e-6)
        return ""
    except AssertionError as e:
        return str(e)


def linear_code(lib, w, x, y):
    n, k = w.shape
    return int(lib.zg_linear_forward(k, n, w.ctypes.data, None, x.ctypes.data, x.size, y.ctypes.data, y.size))


def generations(cfg, w):
    m = gpt.GPT(cfg)
    m.load_weights(w)
    prompt = synth.rand_tokens(9, 3, cfg.vocab_size)
    greedy = m.generate([prompt], 32)[0]
    sampled = m.generate_sample([prompt], 32, 0.8, seed=3)[0]
    m.close()
    return [int(t) for t in greedy], [int(t) for t in sampled]


class Attn:
    """zg_attn_forward over host caches this object owns, beside the oracle's."""

    def __init__(self):
        self.caw = synth.fill_normal(70, 3 * E * E, 0, 0.08).reshape(3 * E, E)
        self.cab = synth.fill_normal(71, 3 * E, 0, 0.05)
        self.cpw = synth.fill_normal(72, E * E, 0, 0.08).reshape(E, E)
        self.cpb = synth.fill_normal(73, E, 0, 0.05)
        self.attn = ops.CausalSelfAttention(HEADS, E, ops.Linear(E, 3 * E, self.caw, self.cab), ops.Linear(E, E, self.cpw, self.cpb))
        self.k, self.v = z(T * E), z(T * E)
        self.scratch = (z(3 * E), z(E), z(T * E), z(T * E), z(T))

    def oracle(self):
        return oracle.CausalSelfAttention(HEADS, E, self.caw, self.cab, self.cpw, self.cpb, T)

    def step(self, t, x):
        out = z(E)
        qkv, q, k_, v_, a = self.scratch
        self.attn.forward(t, x, self.k[: t * E], self.v[: t * E], out, qkv, q, k_[: t * E], v_[: t * E], a[:t])
        return out


def main():
    import torch

    lib = _lib.load()
    res = {}
    cfg = synth.CONFIGS["tiny"]
    w = synth.make_weights(cfg, seed=5, bf16=True)
    gcfg = _lib.GptConfig(cfg.vocab_size, cfg.context_size, cfg.n_layer, cfg.n_heads, cfg.n_embed)

    # ---- 1. a small arena
    res["init_ex"] = int(lib.zg_init_ex(0, 1 << 20))
    big_w, big_x, big_y = synth.fill_normal(1, 600 * 600, 0, 0.05).reshape(600, 600), synth.fill_normal(2, 600).reshape(1, 600), z(1, 600)
    res["linear_beyond_arena"] = linear_code(lib, big_w, big_x, big_y)  # 1.44 MB of weight through a 1 MiB arena
    wl = synth.fill_normal(3, 40 * 64, 0, 0.05).reshape(40, 64)
    xl = synth.fill_normal(4, 3 * 64).reshape(3, 64)
    yl = z(3, 40)
    res["linear_fits"] = linear_code(lib, wl, xl, yl)
    res["linear_fits_close"] = close(oracle.linear_forward(64, 40, wl, None, xl), yl, "Linear in a small arena")
    # ---- 2. another device while initialised
    res["init_other_device"] = int(lib.zg_init(1))
    res["init_same_device"] = int(lib.zg_init(0))
    # ---- 3. a handle's life, a registered weight, three positions of a host KV cache; then shutdown
    res["tokens_1"] = generations(cfg, w)
    res["register"] = int(lib.zg_register_tensor(wl.ctypes.data, wl.size))
    at = Attn()
    ref = at.oracle()
    xs = synth.fill_normal(74, T * E, 0, 1.0).reshape(T, E)
    res["attn_close_before"] = "".join(close(ref.forward(t, xs[t - 1]), at.step(t, xs[t - 1]), f"attn step {t}") for t in (1, 2, 3))
    res["shutdown_1"] = int(lib.zg_shutdown())
    # ---- 4. after shutdown
    h = C.c_void_p()
    res["after_shutdown"] = {
        "zg_set_stream": int(lib.zg_set_stream(None)),
        "zg_synchronize": int(lib.zg_synchronize()),
        "zg_register_tensor": int(lib.zg_register_tensor(wl.ctypes.data, wl.size)),
        "zg_linear_forward": linear_code(lib, wl, xl, z(3, 40)),
        "zg_gpt_create": int(lib.zg_gpt_create(C.byref(h), C.byref(gcfg), 1, 0)),
    }
    res["shutdown_twice"] = int(lib.zg_shutdown())
    # ---- 5. again
    res["init_again"] = int(lib.zg_init(0))
    res["tokens_2"] = generations(cfg, w)
    wl *= np.float32(-2.0)  # in place, NOT registered again: a registry that survived would multiply by the old bytes
    yl2 = z(3, 40)
    res["linear_after"] = linear_code(lib, wl, xl, yl2)
    res["linear_after_close"] = close(oracle.linear_forward(64, 40, wl, None, xl), yl2, "Linear on the changed weight")
    res["linear_after_err"] = rel_err(oracle.linear_forward(64, 40, wl, None, xl), yl2)
    res["linear_after_err_if_stale"] = rel_err(oracle.linear_forward(64, 40, wl, None, xl), yl)
    # the caches now hold the rows of ANOTHER sequence (edited behind the library's back, which a live mirror forbids): position 4
    # is right only if rows 0 .. 2 are uploaded from the caller's buffers again
    ref2 = at.oracle()
    xs2 = synth.fill_normal(75, T * E, 0, 1.0).reshape(T, E)
    for t in (1, 2, 3):
        ref2.forward(t, xs2[t - 1])
    stale_k = at.k[: 3 * E].copy()
    at.k[: 3 * E], at.v[: 3 * E] = ref2.k_cache[: 3 * E], ref2.v_cache[: 3 * E]
    res["attn_rows_differ"] = bool(np.abs(stale_k - at.k[: 3 * E]).max() > 0.1)
    got4 = at.step(4, xs2[3])
    res["attn_close_after"] = close(ref2.forward(4, xs2[3]), got4, "attn step 4 over the other sequence's rows")
    res["attn_err_after"] = rel_err(ref2.forward(4, xs2[3]), got4)
    res["attn_err_if_stale"] = rel_err(ref.forward(4, xs2[3]), ref2.forward(4, xs2[3]))
    # ---- 6. the same life with the library on a caller's stream when it is shut down
    s = torch.cuda.Stream()
    res["set_stream"] = int(lib.zg_set_stream(s.cuda_stream))
    res["tokens_3"] = generations(cfg, w)
    res["register_3"] = int(lib.zg_register_tensor(wl.ctypes.data, wl.size))
    res["shutdown_on_caller_stream"] = int(lib.zg_shutdown())
    res["after_shutdown_2"] = int(lib.zg_synchronize())
    with torch.cuda.stream(s):  # the caller's stream is the caller's: still alive
        t = torch.arange(8, device="cuda").sum()
    s.synchronize()
    res["caller_stream_alive"] = int(t.item())
    res["init_third"] = int(lib.zg_init(0))
    res["tokens_4"] = generations(cfg, w)
    res["shutdown_3"] = int(lib.zg_shutdown())
    print(json.dumps(res))


def bad_device():
    lib = _lib.load()
    res = {"init_ex_device_out_of_range": int(lib.zg_init_ex(1 << 20, 1 << 20)), "init_negative_device": int(lib.zg_init(-1)),
           "synchronize_uninitialised": int(lib.zg_synchronize())}
    print(json.dumps(res))


if __name__ == "__main__":
    {"main": main, "bad_device": bad_device}[sys.argv[1]]()
