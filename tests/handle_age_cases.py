"""The handles of the handle-age tests, and a model of the rule that keeps a decode tag from meeting itself, without a GPU.

The hand-over protocol has state that changes only over a handle's lifetime: the device step counter whose low 24 bits a decode
tag carries, the host's count of enqueued steps that zeroes the tagged words every 2^23 of them (note_steps, api_gpt.hip), and the
32-bit epoch of the whole-prompt c_attn GEMM's stream-K flags.  test_handle_age_gpu.py sets a handle's age (zg_debug_gpt_age) and
runs these handles at the wrap points; test_handle_age_cases_cpu.py asserts from plan_case that they have the modes named here."""
import pass_stage_cases as pc
from decode_stage_cases import Case

E24, E23, E32 = 1 << 24, 1 << 23, 1 << 32

# decode handles (decode_stage_cases.Case; seq_len is the long step's: 257 = one key in the second attention split)
FUSED = Case(128, 1, seq_len=257, ctx=320, layers=2)          # one sequence: the fused launch (qkv_tag; partials merged by attn c_proj)
TAGS = Case(128, 3, seq_len=257, ctx=320, layers=2)           # lock step: planes, part_tag merged by the last split
TICKETS = Case(128, 2, off=4, seq_len=257, ctx=320, layers=2)  # lock step with the tagged hand-overs off: nothing ages
SIX_SPLITS = Case(128, 2, seq_len=1300, ctx=1536)             # planes + tags above four splits: the one-at-a-time polling loop
PL4_KS = Case(512, 2, seq_len=257, ctx=320)                   # mlp c_proj K-sliced on the four-wave kernel: sk_tag
MFMA16_KS = Case(1600, 2, seq_len=257, ctx=320)               # mlp c_proj K-sliced on the matrix cores: slices meet by ticket
DECODE = {"fused": FUSED, "tags": TAGS, "tickets": TICKETS, "six-splits": SIX_SPLITS, "pl4-ks": PL4_KS, "mfma16-ks": MFMA16_KS}

# the whole-prompt pass whose c_attn hands half tiles over between workgroups (pass_stage_cases: the only stream-K case there;
# tests/golden/prefill_plan.json holds no smaller one: stream-K needs tiles > workgroups, which takes ZGPT2_GEMM_WGS below 24 tiles)
STREAM_K = pc.Case(384, 4, 256, pin=(1, 0), wgs=16, twice=True)  # (as pass_stage_cases lists it)


def clear_positions(calls, clear=True):
    """note_steps over a schedule of calls [(device steps the call runs, steps the host counts for it)]: the device steps in front
    of which the tagged words are zeroed (the clear is enqueued in front of the steps of the call that crosses 2^23 counted)."""
    since, step, out = 0, 0, []
    for dev, counted in calls:
        since += counted
        if since >= E23:
            since = counted
            if clear:
                out.append(step)
        step += dev
    return out, step


def stale_match(clears, i, j):
    """A slot written at device step i (tag epoch i mod 2^24), next read at step j, written by no step in between: does the
    reader take the old word for its own?  It does when the tags are equal and no clear fell in (i, j]."""
    return j > i and (j - i) % E24 == 0 and not any(i < c <= j for c in clears)


def first_stale_pair(clears, end):
    """The first (i, j) below `end` with a stale match, over every write step: the worst writes are the first step behind a
    clear (and step 0), and the first read that can match is 2^24 steps on."""
    for i in [0] + list(clears):
        if i + E24 < end and stale_match(clears, i, i + E24):
            return i, i + E24
    return None
