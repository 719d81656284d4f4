#!/usr/bin/env python3
"""In-kernel timeline of the decode GEMVs (needs `make -C zig_gpt2_amd/csrc stamps`,
ZGPT2_LIB=zig_gpt2_amd/lib/libzgpt2_hip_stamps.so).  Prints, per kernel class, the median
s_memtime deltas between the stamps of wave 0 of the first / last workgroup over a graph chain.

  kernel_stamps.py [model [batch [classes [lengths]]]]   e.g. 124M 1 3 200,400,700,1000
classes / lengths: comma-separated kernel classes (default 1,3,4,5,6) and sequence lengths the chain runs at (default 0:
mid-context).

  kernel_stamps.py 124M 1 fused [lengths]   (default lengths 64,256,512,1024)
the attention role of the fused ln_1 + c_attn + attention launch (class 1 at batch 1; attn_decode.h ZG_ASTAMP): per split and
wave of head 0, the medians of entry -> K / V loads issued -> first poll round back -> tags matched -> arithmetic done ->
published (the arithmetic split into `new row in place` + the rest), the poll rounds consumed, and which wave held row T - 1;
beside them the c_attn role's own phases (workgroup 0).  Classes 1 and 4 at batch 1 (gemv_lnk_body) also print their issue phase
split into weight loads, x + ln_g, and c2 / c3.  ZGPT2_DECODE_PATHS_OFF selects the hand-over's paths as everywhere (bits 512,
1024)."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from zig_gpt2_amd import _lib, gpt, synth

lib = _lib.load(); _lib.check(lib.zg_init(0))
raw = C.CDLL(_lib.SO_PATH)
raw.zg_debug_stamps_read.argtypes = [C.c_void_p, C.c_size_t]
cfg = synth.CONFIGS[sys.argv[1] if len(sys.argv) > 1 else "124M"]
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1
m = gpt.GPT(cfg, batch=B); m.load_weights(synth.make_weights(cfg, seed=0, bf16=True))
m.generate([synth.rand_tokens(b, 1, cfg.vocab_size) for b in range(B)], min(64, cfg.context_size))
names = ["t0 entry", "t1 W issued+T", "t2 LN stats barrier", "t3 xs ready", "t4 xr in regs", "t5 pass A done", "t6 pass B done", "t7 loop end", "t9 flush"]
fused = len(sys.argv) > 3 and sys.argv[3] == "fused"
classes = [1] if fused else [int(c) for c in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 3, 4, 5, 6]
lengths = [int(t) for t in sys.argv[4].split(",")] if len(sys.argv) > 4 else [64, 256, 512, 1024] if fused else [0]
ATTN = 0x10000  # word 8 of an attention-role record: ATTN | split << 4 | wave


def fused_report(rec):
    """The attention role's records of one chain: a line per (split, wave) of head 0."""
    r = rec[(rec[:, 8] & ATTN) != 0]
    print(f"  attention role, head 0: {len(r)} records (ticks of s_memtime; medians over the chain's launches behind the first four)")
    print("    split wave holder  K/V-issued  first-round-back  tags-matched  arithmetic (row placed + rest)  published  | entry->published  rounds med / max  first round matched")
    for key in sorted(set(r[:, 8].tolist())):
        q = r[r[:, 8] == key]
        q = q[np.argsort(q[:, 0])][4:] if len(q) > 8 else q
        idle = q[:, 1] == 0  # a wave beyond t_hi issues nothing and only meets the barrier
        if idle.all():
            print(f"    {(key >> 4) & 0xfff:5d} {key & 15:4d}   idle (no positions below t_hi): entry->barrier {np.median(q[:, 5] - q[:, 0]):.0f}")
            continue
        q = q[~idle]
        t = q[:, :6].copy()
        t[:, 2] &= ~1  # (bit 0 of the first-round stamp: that round did not match)
        d = np.median(np.diff(t, axis=1), axis=0)
        first_ok = np.mean((q[:, 2] & 1) == 0)
        rounds, holder = q[:, 6] & 0xffffffff, q[:, 6] >> 32
        placed = np.median(q[:, 7] - t[:, 3])  # tags matched -> the new row in place (word 7); the rest is the arithmetic proper
        print(f"    {(key >> 4) & 0xfff:5d} {key & 15:4d} {int(np.median(holder)):6d}  {d[0]:10.0f}  {d[1]:16.0f}  {d[2]:12.0f}  {d[3]:10.0f} ({placed:4.0f} + {d[3] - placed:4.0f})"
              f"          {d[4]:9.0f}  | {np.median(t[:, 5] - t[:, 0]):16.0f}  {np.median(rounds):10.1f} / {rounds.max():3d}  {100 * first_ok:17.0f} %")
for cls, at in ((c, t) for c in classes for t in lengths):
    assert raw.zg_debug_stamps_begin() == 0
    m.time_kernel(cls, 64, at=at)
    buf = np.zeros(16 + 10 * 4096, np.uint64)
    assert raw.zg_debug_stamps_read(buf.ctypes.data, buf.size) == 0
    n = int(buf[0]); rec = buf[16:16 + 10 * n].reshape(n, 10).astype(np.int64)
    print(f"== class {cls} {gpt.GPT.PROFILE_CLASSES[cls]}" + (f" at T = {at}" if at else "") + f": {n} records")
    if fused:
        fused_report(rec)
    rec = rec[(rec[:, 8] & ATTN) == 0]
    for which, label in ((0, "first WG"), (None, "last WG")):
        r = rec[rec[:, 8] == 0] if which == 0 else rec[rec[:, 8] != 0]
        if len(r) == 0: continue
        r = r[np.argsort(r[:, 0])]
        lnk = cls in (1, 4) and B == 1  # gemv_lnk_body: stamps 6 / 7 split its issue phase (weight loads issued / x and ln_g issued)
        ts = np.concatenate([r[:, :6] if lnk else r[:, :8], r[:, 9:10]], axis=1)
        d = np.diff(ts, axis=1)
        med = np.median(d[4:], axis=0)
        gap = np.median(np.diff(r[:, 0])[4:]) if len(r) > 6 else -1
        tags = [n.split()[0] for n in names[1:6]] + ["t9"] if lnk else [n.split()[0] for n in names[1:]]
        print(f"  {label}: launch-to-launch {gap:.0f} ticks; phases " + " ".join(f"{tags[i]}:{med[i]:.0f}" for i in range(len(tags))) + f"  body {np.median(ts[4:, -1] - ts[4:, 0]):.0f}")
        if lnk:
            g1, g2, rest = (np.median(x[4:]) for x in (r[:, 6] - r[:, 0], r[:, 7] - r[:, 6], r[:, 1] - r[:, 7]))
            print(f"      issue phase t0 -> t1: weight loads {g1:.0f}, x + ln_g {g2:.0f}, c2 / c3 and T {rest:.0f}")
