"""Decode speed by weight storage: bf16 (default), B24 (ZG_GPT_WEIGHTS_B24) and fp32 (ZG_GPT_WEIGHTS_F32) handles of GPT-2 124M,
greedy generation of 1024 positions from 1-token prompts at batch 1 and batch 8 (bench.py's headline workload and its
8-prompt configuration).  All six handles are created first; then ROUNDS rounds each time every storage in turn, so that the
three storages alternate in one process.  Per storage and batch also: every decode kernel class timed with the layers walked
(zg_gpt_time_kernel(..., ZG_TIME_WALK_LAYERS), weights from the memory side as in the real step), its algorithmic bytes per
launch and the fraction of the 8 TB/s HBM peak, and the kernel symbol the class took.

    python tools/bench_weight_storage.py [--rounds 3] [--gens 3] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
STORAGES = {"bf16": {}, "b24": {"weights_b24": True}, "f32": {"weights_f32": True}}
WBYTES = {"bf16": 2, "b24": 3, "f32": 4}


def class_table(m, cfg, batch, wsz, lib):
    from zig_gpt2_amd import _lib

    E, L, V = cfg.n_embed, cfg.n_layer, cfg.vocab_size
    t_mid = cfg.context_size // 2
    classes = [(1, "ln_1 + c_attn (+ attention at batch 1)", L, 3 * E * E * wsz + (2 * t_mid * E * 4 if batch == 1 else 0)),
               (2, "attention (split-KV decode)", L, 2 * t_mid * E * 4 * batch),
               (3, "head merge + attn c_proj + residual", L, E * E * wsz),
               (4, "ln_2 + c_fc + GELU", L, 4 * E * E * wsz),
               (5, "mlp c_proj + residual", L, 4 * E * E * wsz),
               (6, "ln_f + lm_head + argmax", 1, V * E * wsz)]
    rows = []
    for which, name, n_launch, nbytes in classes:
        us, _ = m.time_kernel(which, 256, walk_layers=True)
        sym = C.create_string_buffer(160)
        _lib.check(lib.zg_debug_last_kernel(sym, 160))
        rows.append({"class": which, "name": name, "kernel_symbol": sym.value.decode(), "launches_per_token": n_launch,
                     "us_layers_walked": round(us, 3), "algorithmic_bytes_per_launch": int(nbytes),
                     "hbm_frac": round(nbytes / us / 1e3 / HBM_PEAK_GBS, 4), "us_per_token": round(us * n_launch, 2)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--gens", type=int, default=3, help="timed generations per handle and round")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    from zig_gpt2_amd import _lib, gpt, synth

    lib = _lib.load()
    _lib.check(lib.zg_init(0))
    cfg = synth.CONFIGS["124M"]
    ctx = cfg.context_size
    w = synth.make_weights(cfg, seed=1, bf16=False)  # an fp32 checkpoint: what B24 storage is for
    w = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
    batches = [int(b) for b in a.batches.split(",")]
    handles = {}
    for b in batches:
        for s, kw in STORAGES.items():
            m = gpt.GPT(cfg, batch=b, **kw)
            m.load_weights(w)
            handles[(s, b)] = m
    del w
    torch.cuda.synchronize()
    prompts = {b: [synth.rand_tokens(2000 + i, 1, cfg.vocab_size) for i in range(b)] for b in batches}
    for (s, b), m in handles.items():  # warm-up: every graph bucket captured, every kernel loaded
        m.generate(prompts[b], ctx)
    runs = {f"{s}_x{b}": [] for (s, b) in handles}
    for r in range(a.rounds):
        for b in batches:
            for s in STORAGES:
                m = handles[(s, b)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.gens):
                    m.generate_enqueue(prompts[b], ctx)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                m.generate_fetch(ctx)
                runs[f"{s}_x{b}"].append(round(b * (ctx - 1) * a.gens / wall, 1))
                print(f"round {r} {s} x{b}: {runs[f'{s}_x{b}'][-1]} tok/s", file=sys.stderr, flush=True)
    out = {"workload": "GPT-2 124M greedy decode, 1-token prompts, 1024 positions, unrounded fp32 checkpoint",
           "rounds": a.rounds, "gens_per_round": a.gens, "tokens_per_s": {}, "classes": {}, "weight_bytes_per_token": {}}
    for (s, b), m in handles.items():
        k = f"{s}_x{b}"
        v = runs[k]
        out["tokens_per_s"][k] = {"runs": v, "median": float(np.median(v)), "min": min(v), "max": max(v)}
        out["weight_bytes_per_token"][k] = m.step_bytes(1)[0]
        out["classes"][k] = class_table(m, cfg, b, WBYTES[s], lib)
    for b in batches:
        med = {s: out["tokens_per_s"][f"{s}_x{b}"]["median"] for s in STORAGES}
        out[f"b24_over_f32_x{b}"] = round(med["b24"] / med["f32"], 3)
        out[f"b24_over_bf16_x{b}"] = round(med["b24"] / med["bf16"], 3)
    for m in handles.values():
        m.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
