"""Scripted op-tier session for the launch-trace comparison: python tools/experiments/op_session_trace.py OUT.npz  (library chosen
by ZGPT2_LIB).  Every src/ops.zig entry once on host buffers and once on device pointers, a wide (K > 8192) and a matrix-core
Linear, 300 consecutive small calls (crosses the 256-call drain), 20 zg_attn_forward steps on host caches.  Each block opens with
an op-tier gelu launch: session_trace_compare.py cuts the trace there (OUT.npz.marks names the blocks)."""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from zig_gpt2_amd import _lib, ops, synth

lib = _lib.load()
_lib.check(lib.zg_init(0))
out = {}
E, H, T = 128, 2, 20
rnd = lambda seed, n, std=1.0: synth.fill_normal(seed, n, 0, std)


def every_op(tag, mk):
    """mk(array) -> the buffer handed to the library (the array itself, or a device tensor); results are read back from it"""
    back = lambda a: np.array(a.cpu().numpy() if hasattr(a, "cpu") else a, copy=True)
    h = mk(rnd(1, 3 * E))
    ops.gelu(h)  # (the block's marker)
    out[f"{tag}/gelu"] = back(h)
    g, b = mk(rnd(2, E, 0.1) + 1), mk(rnd(3, E, 0.1))
    x = mk(rnd(4, 3 * E))
    ops.LayerNorm(E, g, b).forward(x)
    out[f"{tag}/layernorm"] = back(x)
    w, bias, y = mk(rnd(5, 3 * E * E, 0.05)), mk(rnd(6, E, 0.05)), mk(np.zeros(3 * E, np.float32))
    ops.Linear(E, E, w[: E * E], bias).forward(x, y)  # (on host buffers: its input is LayerNorm's output, the device twin)
    out[f"{tag}/linear"] = back(y)
    emb = mk(np.zeros(3 * E, np.float32))
    idx = mk(np.array([7, 0, 31], np.int64 if mk is dev else np.uint64))  # (usize: numpy uint64 / torch int64)
    ops.Embedding(E, w[: 32 * E]).forward(idx, emb)
    out[f"{tag}/embedding3"] = back(emb)
    ops.Embedding(E, w[: 32 * E]).forward(idx[:1], emb[:E])
    out[f"{tag}/embedding1"] = back(emb)
    sm = mk(rnd(7, 1000, 3.0))
    ops.softmax(sm)
    out[f"{tag}/softmax"] = back(sm)
    attn = ops.CausalSelfAttention(H, E, None, None)
    qkv, part = mk(rnd(8, 5 * 3 * E)), mk(np.zeros(5 * E, np.float32))
    attn.split_qkv(5, qkv, 1, part)
    out[f"{tag}/split_qkv"] = back(part)
    tr = mk(np.zeros(5 * E, np.float32))
    attn.transpose((5, H, E // H), part, tr)
    out[f"{tag}/transpose"] = back(tr)
    q, k, v, o = mk(rnd(9, H * 64)), mk(rnd(10, H * 70 * 64)), mk(rnd(11, H * 70 * 64)), mk(np.zeros(H * 64, np.float32))
    ops.scaled_dot_product_attention(q, k, v, H, 70, 64, o, mk(np.zeros(70, np.float32)))
    out[f"{tag}/sdpa"] = back(o)
    caw, cab, cpw, cpb = mk(rnd(12, 3 * E * E, 0.08)), mk(rnd(13, 3 * E, 0.05)), mk(rnd(14, E * E, 0.08)), mk(rnd(15, E, 0.05))
    full = ops.CausalSelfAttention(H, E, ops.Linear(E, 3 * E, caw, cab), ops.Linear(E, E, cpw, cpb))
    z = lambda n: mk(np.zeros(n, np.float32))
    kc, vc, res = z(2 * E), z(2 * E), z(E)
    for t in (1, 2):
        full.forward(t, mk(rnd(15 + t, E)), kc[: t * E], vc[: t * E], res, z(3 * E), z(E), z(2 * E), z(2 * E), z(2))
        out[f"{tag}/attn{t}"] = back(res)
    out[f"{tag}/k_cache"] = back(kc)


keep = lambda a: a
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
every_op("host", keep)
every_op("device", dev)

h = rnd(20, 64)
ops.gelu(h)  # marker: the Linears
for tag, m, k, n in (("wide", 3, 8192 + 579, 70), ("mfma", 48, 256, 96)):
    w, x, y = rnd(21, n * k, 0.05).reshape(n, k), rnd(22, m * k), np.zeros(m * n, np.float32)
    before = lib.zg_debug_gemm_launches()
    ops.Linear(k, n, w, rnd(23, n, 0.05)).forward(x, y)
    assert (lib.zg_debug_gemm_launches() > before) == (tag == "mfma")
    out[f"linear/{tag}"] = y

ops.gelu(h)  # marker: 300 small calls, alternately one that announces its own completion (4 rows) and one that does not (5 rows)
g, b = rnd(30, E, 0.1) + 1, rnd(31, E, 0.1)
ln = ops.LayerNorm(E, g, b)
x4, x5 = rnd(32, 4 * E), rnd(33, 5 * E)
for i in range(150):
    ln.forward(x4)
    ln.forward(x5)
out["small/x4"], out["small/x5"] = x4, x5

ops.gelu(h)  # marker: the attention walk on host caches (mirrors)
caw, cab, cpw, cpb = rnd(40, 3 * E * E, 0.08), rnd(41, 3 * E, 0.05), rnd(42, E * E, 0.08), rnd(43, E, 0.05)
attn = ops.CausalSelfAttention(H, E, ops.Linear(E, 3 * E, caw.reshape(3 * E, E), cab), ops.Linear(E, E, cpw.reshape(E, E), cpb))
kc, vc = np.zeros(T * E, np.float32), np.zeros(T * E, np.float32)
xs = rnd(44, T * E).reshape(T, E)
z = lambda n: np.zeros(n, np.float32)
for s in range(T):
    o, _qkv, _q = z(E), z(3 * E), z(E)
    attn.forward(s + 1, xs[s], kc[: (s + 1) * E], vc[: (s + 1) * E], o, _qkv, _q, z(T * E), z(T * E), z(T))
    out[f"walk/{s}/out"], out[f"walk/{s}/qkv"], out[f"walk/{s}/q"] = o, _qkv, _q
out["walk/k_cache"], out["walk/v_cache"] = kc, vc

np.savez(sys.argv[1], **out)
open(sys.argv[1] + ".marks", "w").write("\n".join(["host buffers", "device pointers", "wide and matrix-core Linear", "300 small calls",
                                                    "attention walk"]) + "\n")
print("session ok", len(out), "results")
