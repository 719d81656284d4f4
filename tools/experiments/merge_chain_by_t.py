"""Chain cost of head merge + attn c_proj (kernel class 3) by sequence length on 124M at batch 1, for the three forms of the
merge prologue (gemv_ksplit.hip): specialised by split count with the (m, l) words by wave-uniform loads (default), the same with
the lanes' own vector loads (ZGPT2_DECODE_PATHS_OFF=256), and the four-slot prologue (=128); mlp c_proj (class 5) beside them.
Every figure is the average over a 256-launch graph chain that walks the layers, taken three times; one JSON line per form."""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
from zig_gpt2_amd import _lib, gpt, synth

lib = _lib.load()
_lib.check(lib.zg_init(0))
cfg = synth.CONFIGS["124M"]
w = synth.make_weights(cfg, seed=0, bf16=True)
for rep in range(2):  # the forms alternated, twice over
    for form, off in (("by split count, scalar (m, l)", None), ("by split count, vector (m, l)", "256"), ("four slots", "128")):
        os.environ.pop("ZGPT2_DECODE_PATHS_OFF", None)
        if off is not None:
            os.environ["ZGPT2_DECODE_PATHS_OFF"] = off  # (read when a launch is planned: the chain below is captured under it)
        m = gpt.GPT(cfg)
        m.load_weights(w)
        row = {"form": form, "paths_off": int(off or 0), "rep": rep}
        for T in (64, 256, 257, 512, 768, 1024):
            row[f"T{T}"] = [round(m.time_kernel(3, 256, walk_layers=True, at=T)[0], 3) for _ in range(3)]
        row["mlp_proj"] = [round(m.time_kernel(5, 256, walk_layers=True)[0], 3) for _ in range(3)]
        print(json.dumps(row), flush=True)
        m.close()
