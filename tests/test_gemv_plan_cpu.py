"""The route table of the decode-regime Linear, pinned on the CPU: zg_debug_gemv_plan (gemv_plan, csrc/gemv.hip) over a fixed list
of launches against tests/golden/gemv_plan.json, which records what commit 73f30f8 — the last one that answered these questions
with a dozen predicates in four files — decided and launched for the same list.  Equality is exact, field by field, and no row
is skipped.  A deliberate change of a threshold changes the fixture with it, in the same commit, for the reviewer to see."""
import ctypes as C
import hashlib
import json
import os

from zig_gpt2_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemv_plan.json")

FIELDS = ["route", "grid", "kslices", "block", "lds", "mt", "lpr", "cpl", "ks", "nw", "line", "gpl", "alias", "pairs", "steps", "rows_per_wave",
          "waves_per_wg", "row_group", "rows_per_wg", "pf_tiles", "supported", "can_take_planes", "can_write_planes", "pl4_with_planes"]
PRO_NONE, PRO_LN, PRO_MERGE = 0, 1, 2
EPI_STORE, EPI_RESID, EPI_GELU, EPI_QKV, EPI_ARGMAX = 0, 1, 2, 3, 4
BF16, F32, B24 = 0, 1, 2
LN_FOLDED, PLANES_IN, STATS_IN, SPLIT_K, RAGGED = 1, 2, 4, 8, 16


def cases():
    """(paths_off, M, N, K, prologue, epilogue, weight_type, operands, sk_tiles, t_hi), in a fixed order.  The cross product of the
    batch sizes, weight types, widths, Linear roles, optional operands, t_hi and ZGPT2_DECODE_PATHS_OFF values, without the
    combinations in which an axis cannot matter: t_hi is read by the head-merge prologue alone; planes, tile statistics, the
    split-K workspace and the path bits 2 / 16 / 32 belong to the matrix-core routes (bf16, 2..8 rows; elsewhere the bits are
    tried all at once, as 50); statistics and ragged strides need planes; lm_head takes no planes."""
    out = []
    for wt in (F32, BF16, B24):
        for M in (1, 2, 3, 4, 5, 8):
            mc = wt == BF16 and M >= 2
            offs = (0, 2, 16, 32, 50) if mc else (0, 50)
            sks = (0, SPLIT_K) if mc else (0,)
            for E in (128, 384, 768, 1024, 1280, 1600, 2048):
                roles = []  # (N, K, prologue, epilogue, operands, sk_tiles, t_hi)

                def planes(ln):
                    if not mc:
                        return [0]
                    v = [0, PLANES_IN, PLANES_IN | RAGGED]
                    return v + [PLANES_IN | STATS_IN, PLANES_IN | STATS_IN | RAGGED] if ln else v

                for fold in (0, LN_FOLDED):
                    for pl in planes(True):
                        for sk in sks:
                            roles.append((3 * E, E, PRO_LN, EPI_QKV, fold | pl | sk, (3 * E + 15) // 16, 0))    # ln_1 + c_attn
                            roles.append((4 * E, E, PRO_LN, EPI_GELU, fold | pl | sk, (4 * E + 15) // 16, 0))   # ln_2 + c_fc
                    for V in (65, 50257):
                        for sk in sks:
                            roles.append((V, E, PRO_LN, EPI_ARGMAX, fold | sk, (V + 15) // 16, 0))             # ln_f + lm_head
                for sk in sks:
                    for t_hi in (0, 100, 1024, 1100):
                        roles.append((E, E, PRO_MERGE, EPI_RESID, sk, (E + 15) // 16, t_hi))                   # merge + attn c_proj
                    for pl in planes(False):
                        roles.append((E, E, PRO_NONE, EPI_RESID, pl | sk, (E + 15) // 16, 0))                  # attn c_proj, merged heads
                        roles.append((E, 4 * E, PRO_NONE, EPI_RESID, pl | sk, (E + 15) // 16, 0))              # mlp c_proj
                    if mc:  # a split-K workspace too small for the matrix
                        roles.append((E, 4 * E, PRO_NONE, EPI_RESID, PLANES_IN | SPLIT_K, (E + 15) // 16 - 1, 0))
                for (N, K, pro, epi, ops, skt, t_hi) in roles:
                    for off in offs:
                        out.append((off, M, N, K, pro, epi, wt, ops, skt if ops & SPLIT_K else 0, t_hi))
    # the op tier's edge shapes (plain Linears, and what must stay unsupported)
    for wt in (F32, BF16, B24):
        for M in (1, 2, 8):
            for (N, K) in ((1000, 8192), (1000, 8184), (1000, 8200), (1000, 16), (1, 768), (70000, 768), (1000, 771), (1000, 6003)):
                for (pro, epi) in ((PRO_NONE, EPI_STORE), (PRO_NONE, EPI_RESID), (PRO_NONE, EPI_GELU), (PRO_LN, EPI_STORE)):
                    out.append((0, M, N, K, pro, epi, wt, 0, 0, 0))
            out.append((0, M, 70000, 768, PRO_NONE, EPI_RESID, wt, PLANES_IN, 0, 0))  # N above the plane-fed kernel's 0xffff
            out.append((0, M, 768, 768, PRO_LN, EPI_GELU, wt, PLANES_IN, 0, 0))       # planes in front of an unfolded LayerNorm
    return out


def plan_all(rows):
    lib = _lib.load()
    out = (C.c_int * len(FIELDS))()
    plans = []
    saved = os.environ.get("ZGPT2_DECODE_PATHS_OFF")
    try:
        for (off, *args) in rows:
            os.environ["ZGPT2_DECODE_PATHS_OFF"] = str(off)  # (os.environ calls putenv: the library's getenv sees it)
            _lib.check(lib.zg_debug_gemv_plan(*args, out, len(FIELDS)))
            plans.append(list(out))
    finally:
        if saved is None:
            del os.environ["ZGPT2_DECODE_PATHS_OFF"]
        else:
            os.environ["ZGPT2_DECODE_PATHS_OFF"] = saved
    return plans


def recorded(gold):
    """The fixture keeps each distinct plan once and, for the rows in order, runs of (plan number, how many rows)."""
    runs = gold["runs"]
    return [gold["plans"][p] for p, n in zip(runs[0::2], runs[1::2]) for _ in range(n)]


def test_every_plan_is_what_the_parent_decided():
    gold = json.load(open(GOLDEN))
    assert gold["fields"] == FIELDS
    rows = cases()
    assert len(rows) > 10000
    assert hashlib.sha256(repr(rows).encode()).hexdigest() == gold["cases_sha256"], "the fixture was recorded for another list of launches"
    want_all = recorded(gold)
    assert len(want_all) == len(rows)
    routes = set()
    for row, want, got in zip(rows, want_all, plan_all(rows)):
        routes.add(got[0])
        if got != want:
            diff = {f: (w, g) for f, w, g in zip(FIELDS, want, got) if w != g}
            raise AssertionError(f"(off, M, N, K, prologue, epilogue, weight_type, operands, sk_tiles, t_hi) = {row}: (recorded, planned) {diff}")
    assert routes == set(range(10)), routes  # the list reaches every route
