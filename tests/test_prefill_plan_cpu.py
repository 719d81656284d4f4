"""The route table of the whole-prompt Linear, pinned on the CPU: zg_debug_prefill_plan (prefill_gemm_plan, csrc/prefill.hip) over a
fixed list of launches against tests/golden/prefill_plan.json, which records what commit 4e1d508 — the last one that decided a
whole-prompt Linear in six places across prefill.hip and gemm_s4.hip — decided and launched for the same list.  Equality is
exact, field by field, and no row is skipped.  A deliberate change of a threshold changes the fixture with it, in the same commit,
for the reviewer to see."""
import ctypes as C
import hashlib
import json
import os

from zig_gpt2_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prefill_plan.json")

FIELDS = ["status", "family", "tail", "partial", "grid_x", "grid_y", "block", "lds", "slices", "slabs", "ns", "nspl", "xcd_rows", "tiles_n", "s4_kind", "stream_k",
          "band", "npairs", "pa_bits", "pb_bits", "plane_major"]
GEOMETRY = ["grid_x", "grid_y", "slices", "slabs", "xcd_rows", "tiles_n", "band"]  # what varies with the shape under one kernel choice
KERNEL = [f for f in FIELDS if f not in GEOMETRY]
PF_F32, PF_RESID, PF_GELU_SPLIT, PF_PARTIAL, PF_QKV = 0, 1, 2, 3, 4
WS, LN, QKV, SK_WS, SK_FLAGS = 1, 2, 4, 8, 16
WEIGHT_PLANES = 33
S4, T128, T128_WP = 1, 2, 3
S4_PARTIAL, S4_QKV, S4_SPLIT3 = 1, 2, 3
NO_TAIL, LN_SPLIT, REDUCE, REDUCE_LN_SPLIT, REDUCE_RESID_LN = 0, 1, 2, 3, 4
OK, ERR_SHAPE, ERR_UNSUPPORTED, ERR_ARG = 0, -2, -5, -6


def cases():
    """(ZGPT2_GEMM_WGS or 0, M, N, K, ldc, epilogue, nsplit, ws_floats, operands, sk_ws_bytes, sk_flags_words, force kernel, force
    slices), in a fixed order.  The cross product of the widths, row counts, plane counts, Linear roles, workspaces and forces,
    without the combinations in which an axis cannot matter: only a residual add is followed by a LayerNorm, and the fourth
    workspace is the third where 3 M 4E <= 2^24 (60,480 combinations, 49,896 different launches).  A bf16 c_attn is given the
    stream-K operands as the model gives them (the workspace itself, 512 flag words) whenever there is a workspace."""
    out = []
    for E in (128, 384, 768, 1024, 1280, 1600, 2048, 2560):
        for nsplit in (2, 3, WEIGHT_PLANES):
            for M in (1, 3, 24, 100, 257, 600, 1023, 2046, 4092, 8184):
                roles = [(3 * E, E, 3 * E, PF_QKV, QKV)]                                     # c_attn
                for ln in (0, LN):
                    roles.append((E, E, E, PF_RESID, ln))                                    # attn c_proj
                roles.append((4 * E, E, 0, PF_GELU_SPLIT, 0))                                # c_fc
                for ln in (0, LN):
                    roles.append((E, 4 * E, E, PF_RESID, ln))                                # mlp c_proj
                roles.append((E, E, E, PF_F32, 0))                                           # a plain Linear
                for ln in (0, LN):
                    roles.append((E, E, E + 64, PF_RESID, ln))                               # a residual add into wider rows
                for (N, K, ldc, epi, ops) in roles:
                    for ws in sorted({0, 1 << 20, 1 << 24, max(1 << 24, 3 * M * 4 * E)}):
                        sk = epi == PF_QKV and nsplit != WEIGHT_PLANES and ws > 0
                        o = ops | (WS if ws else 0) | (SK_WS | SK_FLAGS if sk else 0)
                        for (fk, fs, wgs) in ((0, 0, 0), (96, 0, 0), (2, 0, 0), (1, 0, 0), (1, 2, 0), (1, 3, 0), (1, 0, 16)):
                            out.append((wgs, M, N, K, ldc, epi, nsplit, ws, o, ws * 4 if sk else 0, 512 if sk else 0, fk, fs))
    # outside the grid: what must stay refused, and the bounds of the persistent kernel's packed arguments
    big = 1 << 26
    for fk in (0, 1, 2):
        out.append((0, 0, 768, 768, 768, PF_RESID, 3, big, WS, 0, 0, fk, 0))                 # no rows
        out.append((0, 600, 800, 768, 800, PF_F32, 3, big, WS, 0, 0, fk, 0))                 # N % 64 != 0
        out.append((0, 600, 768, 800, 768, PF_F32, 3, big, WS, 0, 0, fk, 0))                 # K % 64 != 0
        out.append((0, 600, 768, 768, 768, PF_RESID, 5, big, WS, 0, 0, fk, 0))               # a plane count that does not exist
        out.append((0, 600, 2304, 768, 2304, PF_QKV, 3, big, WS, 0, 0, fk, 0))               # qkv without the cache description
        out.append((0, 600, 2304, 768, 2368, PF_QKV, 3, big, WS | QKV, 0, 0, fk, 0))         # ... with wider rows
        out.append((0, 600, 768, 768, 768, PF_PARTIAL, 3, big, WS, 0, 0, fk, 0))             # the internal epilogue
        out.append((0, 600, 768, 16384, 768, PF_RESID, 3, big, WS, 0, 0, fk, 0))             # 256 K-steps per plane
        out.append((0, 600, 768, 21888, 768, PF_RESID, 3, big, WS, 0, 0, fk, 0))             # 3 K >= 65536
        out.append((0, 600, 768, 64, 768, PF_RESID, 3, big, WS, 0, 0, fk, 0))                # one K-step
        out.append((2048, 8184, 10240, 2560, 0, PF_GELU_SPLIT, 3, big, WS, 0, 0, fk, 0))     # 1024 workgroups and more
        out.append((0, 40000, 1024, 12288, 1024, PF_RESID, 3, big, WS, 0, 0, fk, 0))         # planes of 2 GiB and more
        out.append((0, 8184, 98304, 8192, 0, PF_GELU_SPLIT, WEIGHT_PLANES, 1 << 32, WS, 0, 0, fk, 0))  # weight planes beyond a descriptor
    for (wsb, words) in ((1 << 27, 512), (128 * 196608, 512), (128 * 196608 - 1, 512), (1 << 27, 511)):  # stream-K and its buffers
        for ops in (SK_WS | SK_FLAGS, SK_WS, SK_FLAGS):
            out.append((0, 8184, 2304, 768, 2304, PF_QKV, 3, 1 << 24, WS | QKV | ops, wsb, words, 0, 0))
    for wgs in (8, 16, 24, 32, 48):
        for M in (600, 1023, 2046, 3000, 4092):
            out.append((wgs, M, 2304, 768, 2304, PF_QKV, 2, 1 << 24, WS | QKV | SK_WS | SK_FLAGS, 1 << 27, 512, 1, 0))
    return out


def plan_all(rows):
    lib = _lib.load()
    out = (C.c_int * len(FIELDS))()
    plans = []
    saved = os.environ.get("ZGPT2_GEMM_WGS")
    try:
        for (wgs, *args) in rows:
            if wgs:
                os.environ["ZGPT2_GEMM_WGS"] = str(wgs)  # (os.environ calls putenv: the library's getenv sees it)
            else:
                os.environ.pop("ZGPT2_GEMM_WGS", None)
            _lib.check(lib.zg_debug_prefill_plan(*args, out, len(FIELDS)))
            plans.append(list(out))
    finally:
        if saved is None:
            os.environ.pop("ZGPT2_GEMM_WGS", None)
        else:
            os.environ["ZGPT2_GEMM_WGS"] = saved
    return plans


def recorded(gold):
    """The fixture keeps each distinct plan once, as (kernel number, geometry fields cut behind the last that is not 0) with each
    distinct list of kernel fields once, and, for the rows in order, runs of (plan number, how many rows)."""
    runs, plans = gold["runs"], []
    for (k, *geo) in gold["plans"]:
        d = dict(zip(KERNEL, gold["kernels"][k]), **dict(zip(GEOMETRY, geo + [0] * len(GEOMETRY))))
        plans.append([d[f] for f in FIELDS])
    return [plans[p] for p, n in zip(runs[0::2], runs[1::2]) for _ in range(n)]


def outcome(row, plan):
    """What the coverage assertion counts: (family, instantiation, tail), or the refusal."""
    p = dict(zip(FIELDS, plan))
    if p["status"] != OK:
        return ("refused", p["status"])
    if p["family"] == S4:
        return (S4, p["s4_kind"], p["stream_k"], p["slices"], p["tail"])
    epi = row[5]
    return (p["family"], PF_PARTIAL if p["partial"] else epi, p["ns"], p["nspl"], p["tail"])


def test_every_plan_is_what_the_parent_decided():
    gold = json.load(open(GOLDEN))
    assert (gold["fields"], gold["kernel_fields"], gold["geometry_fields"]) == (FIELDS, KERNEL, GEOMETRY)
    rows = cases()
    assert len(rows) > 49896 and len(set(rows)) == len(rows)
    assert hashlib.sha256(repr(rows).encode()).hexdigest() == gold["cases_sha256"], "the fixture was recorded for another list of launches"
    want_all = recorded(gold)
    assert len(want_all) == len(rows)
    seen = set()
    for row, want, got in zip(rows, want_all, plan_all(rows)):
        seen.add(outcome(row, want))  # (coverage is a property of the recorded table)
        if got != want:
            diff = {f: (w, g) for f, w, g in zip(FIELDS, want, got) if w != g}
            raise AssertionError(f"(wgs, M, N, K, ldc, epilogue, nsplit, ws_floats, operands, sk_ws_bytes, sk_flags_words, force kernel, force slices) = {row}: "
                                 f"(recorded, planned) {diff}")
    # the list reaches every outcome the planner has
    tails = (REDUCE, REDUCE_LN_SPLIT, REDUCE_RESID_LN)
    want = {(S4, S4_PARTIAL, 0, n, t) for n in (1, 2, 4) for t in tails}
    # (three slices + reduce then LayerNorm needs N > 2048 with K / 64 divisible by 3: not in this list)
    want |= {(S4, S4_PARTIAL, 0, 3, REDUCE), (S4, S4_PARTIAL, 0, 3, REDUCE_RESID_LN)}
    want |= {(S4, S4_SPLIT3, 0, 1, NO_TAIL), (S4, S4_QKV, 0, 1, NO_TAIL), (S4, S4_QKV, 1, 1, NO_TAIL)}
    for ns in (1, 2):
        for nspl in (2, 3):
            want |= {(T128, epi, ns, nspl, NO_TAIL) for epi in (PF_F32, PF_RESID, PF_GELU_SPLIT, PF_QKV)}
            want.add((T128, PF_RESID, ns, nspl, LN_SPLIT))
        want |= {(T128_WP, PF_PARTIAL, ns, 0, t) for t in tails}
    # (wide tiles need at least 256 tiles and K slices at most 128: the partial 128-row kernel is never wide)
    want |= {(T128, PF_PARTIAL, 1, nspl, t) for nspl in (2, 3) for t in tails}
    assert not any(o[:3] == (T128, PF_PARTIAL, 2) for o in seen)
    want |= {("refused", ERR_ARG), ("refused", ERR_UNSUPPORTED), ("refused", ERR_SHAPE)}
    assert want <= seen, sorted(want - seen)
    # ... and by name: stream-K at eight prompts of 1023 tokens of the 124M model (384 tiles on 256 workgroups), the fp32-weight
    # launch without a sufficient workspace, K or N off the 64 grid, no rows
    by_row = dict(zip(rows, want_all))
    sk = by_row[(0, 8184, 2304, 768, 2304, PF_QKV, 3, 1 << 24, WS | QKV | SK_WS | SK_FLAGS, 4 << 24, 512, 0, 0)]
    assert (sk[FIELDS.index("stream_k")], sk[FIELDS.index("grid_x")]) == (1, 256)
    assert by_row[(0, 1023, 768, 3072, 768, PF_RESID, WEIGHT_PLANES, 0, 0, 0, 0, 0, 0)][0] == ERR_ARG
    assert by_row[(0, 600, 800, 768, 800, PF_F32, 3, 1 << 26, WS, 0, 0, 0, 0)][0] == ERR_UNSUPPORTED
    assert by_row[(0, 600, 768, 800, 768, PF_F32, 3, 1 << 26, WS, 0, 0, 0, 0)][0] == ERR_UNSUPPORTED
    assert by_row[(0, 0, 768, 768, 768, PF_RESID, 3, 1 << 26, WS, 0, 0, 0, 0)][0] == ERR_UNSUPPORTED
