"""What test_handle_age_gpu.py claims about its handles, asserted without a GPU, and the tag rule as a model.

The handles (handle_age_cases.py) have the modes the GPU file names — from plan_case, which test_decode_stages_gpu.py holds the
library's own report to, and from zg_debug_prefill_plan.  The model runs note_steps' rule over schedules of calls: under the rule
no slot written at step i and next read at step j can carry the reader's tag, and with the clear absent, or with the host counting
too few of the steps the device runs, one can — which is what makes the GPU file's "device epoch advanced by no more than the
host counted" and "at least one clear" necessary conditions.

Where the rule ends: between two clears the device runs at most f x 2^23 - n steps when it runs f steps per counted one (n: the
steps counted for the call that crossed the mark, which run behind the clear).  At f = 2 that is still below 2^24, by those n
steps and nothing else; beyond it — launches beside it that are not counted at all, f = 2.5 — a stale match exists.  zg_gpt_time_kernel of
class 0 ran 64 (1 + ceil(iters / 64)) embed launches and counted iters + 8: f = 14 at iters = 1 (fixed with these tests)."""
import numpy as np
import pytest

import handle_age_cases as hc
import pass_stage_cases as pc
from decode_stage_cases import ROUTES, plan_case
from handle_age_cases import E23, E24, E32

route = lambda case, cls: ROUTES[plan_case(case)[1][cls]["route"]]


def test_the_decode_handles_have_the_modes_the_gpu_tests_name():
    want = {"fused": dict(planes=0, stats=0, tags=0, fused=1), "tags": dict(planes=1, stats=1, tags=1, fused=0),
            "tickets": dict(planes=1, stats=1, tags=0, fused=0), "six-splits": dict(planes=1, stats=1, tags=1, fused=0),
            "pl4-ks": dict(planes=1, stats=1, tags=1, fused=0), "mfma16-ks": dict(planes=1, stats=0, tags=1, fused=0)}
    assert {k: plan_case(c)[0] for k, c in hc.DECODE.items()} == want
    # every handle the aging touches has a tagged hand-over or the fused launch; the ticket handle has neither
    assert all((m["tags"] or m["fused"]) == (k != "tickets") for k, m in want.items())


def test_the_k_sliced_linears_and_the_split_counts():
    # the K-sliced routes the planner offers: mlp c_proj of the lock-step batch on the four-wave kernel from E = 512 (tagged: sk_tag
    # is polled in gemv_pl4.hip alone) and on the matrix cores at E = 1600 (its slices meet by ticket, on a handle whose attention
    # is tagged); one sequence splits K on the vector ALUs (GR_KSPLIT), with no tag: the fused handle's attn c_proj is one
    assert route(hc.PL4_KS, 5) == "GR_PL4_KS" and plan_case(hc.PL4_KS)[1][5]["kslices"] == 4
    assert route(hc.MFMA16_KS, 5) == "GR_MFMA16_KS" and plan_case(hc.MFMA16_KS)[1][5]["kslices"] == 4
    assert route(hc.FUSED, 3) == "GR_KSPLIT" and route(hc.FUSED, 1) == "GR_LNK"
    assert not any(route(hc.DECODE[k], cls).endswith("_KS") for k in ("fused", "tags", "tickets", "six-splits") for cls in (1, 3, 4, 5))
    splits = lambda c: (min((c.seq_len + 63) // 64 * 64, c.ctx) + 255) // 256
    assert [splits(hc.DECODE[k]) for k in ("fused", "tags", "tickets", "pl4-ks", "mfma16-ks")] == [2] * 5
    assert splits(hc.SIX_SPLITS) == 6 > 4  # beyond the four slots polled at once
    # a generation from position 250 over 24 tokens crosses the split boundary at 256 in every 320-context handle
    assert all(c.ctx >= 274 for c in hc.DECODE.values())


def test_the_whole_prompt_case_is_stream_k():
    plans, _ = pc.plan_case(hc.STREAM_K)
    c_attn = [p for cls, l, role, p in plans if role == "c_attn"]
    assert len(c_attn) == hc.STREAM_K.layers == 1 and all(p["stream_k"] == 1 and p["family"] == 1 for p in c_attn)
    assert c_attn[0]["grid_x"] == 16 and c_attn[0]["grid_x"] // 2 * 4 <= 512  # 8 shared tiles x 4 flag words of the 512
    assert hc.STREAM_K in pc.CASES  # ... and it is a case test_pass_stages_gpu.py measures its float64 bounds on
    others = [c for c in pc.CASES if c != hc.STREAM_K and any(p["stream_k"] for cls, l, role, p in pc.plan_case(c)[0])]
    assert not others, "a smaller stream-K case exists: " + ", ".join(c.id for c in others if c.M * c.E < hc.STREAM_K.M * hc.STREAM_K.E)


# ------------------------------------------------------------------ the tag rule as a model
def schedule(rng, total, per_counted=1.0, largest=1 << 16):
    """Calls of 1 .. `largest` counted steps until the device has run `total`: [(device steps, counted steps)]."""
    calls, done = [], 0
    while done < total:
        n = int(rng.integers(1, largest + 1))
        dev = max(int(n * per_counted), 1)
        calls.append((dev, n))
        done += dev
    return calls


def patterns(rng, clears, end, n=4000):
    """'Slot written at step i, next read at step j': the writes around every clear and at random, the reads 1, 2 and 3 tag
    periods on and at random."""
    around = [c + d for c in [0] + clears for d in (-2, -1, 0, 1, 2)]
    writes = [i for i in around if 0 <= i < end] + [int(v) for v in rng.integers(0, end, n)]
    for i in writes:
        for j in [i + k * E24 for k in (1, 2, 3)] + [int(v) for v in rng.integers(i + 1, end + 1, 2)]:
            if j < end:
                yield i, j


@pytest.mark.parametrize("largest", [1, 64, 1 << 16, (1 << 22) + 12345])
def test_no_stale_match_under_the_rule(largest):
    rng = np.random.default_rng(largest)
    # (largest 1: every call one step, as zg_gpt_forward — run as 2^12 such calls at a time, which the rule cannot tell apart
    # unless a block crosses the mark, and 2^23 is a multiple of 2^12)
    calls = schedule(rng, 4 * E24, largest=largest) if largest > 1 else [(1 << 12, 1 << 12)] * (4 * E24 >> 12)
    clears, end = hc.clear_positions(calls)
    assert len(clears) >= 7 and max(b - a for a, b in zip([0] + clears, clears)) < E24
    assert not any(hc.stale_match(clears, i, j) for i, j in patterns(rng, clears, end))
    assert hc.first_stale_pair(clears, end) is None


def test_a_stale_match_exists_without_the_clear_or_with_too_few_steps_counted():
    rng = np.random.default_rng(5)
    calls = schedule(rng, 4 * E24)
    clears, end = hc.clear_positions(calls, clear=False)
    assert clears == [] and hc.first_stale_pair(clears, end) == (0, E24) and hc.stale_match(clears, 12345, 12345 + E24)
    # two device steps per counted step: the gap between clears is 2^24 - 2 n, below 2^24 by the crossing call's own steps alone
    even = [(2 * n, n) for _, n in calls]
    clears, end = hc.clear_positions(even)
    gaps = [b - a for a, b in zip(clears, clears[1:])]
    assert max(gaps) < E24 and min(E24 - g for g in gaps) <= 2 * (1 << 16) and hc.first_stale_pair(clears, end) is None
    # ... so launches beside it that are not counted at all are enough (here 1024 steps per call), as is any factor beyond two
    beside = [c for dev, n in even for c in ((dev, n), (1024, 0))]
    clears, end = hc.clear_positions(beside)
    pair = hc.first_stale_pair(clears, end)
    assert max(b - a for a, b in zip(clears, clears[1:])) > E24 and pair is not None and hc.stale_match(clears, *pair)
    for f in (2.5, 3.0, 14.0):  # (14: zg_gpt_time_kernel of class 0 as it counted before: 128 launches for 9)
        clears, end = hc.clear_positions(schedule(rng, 8 * E24, per_counted=f))
        pair = hc.first_stale_pair(clears, end)
        assert pair is not None and hc.stale_match(clears, *pair), f


def test_the_tag_is_never_zero_and_the_epoch_field_is_24_bits():
    """tag = epoch << 8 | launch id in 32 bits: at epoch = 0 (mod 2^24) the tag is the launch id, which starts at 1; the census
    counts a word only with a launch id."""
    tag = lambda epoch, launch: ((epoch << 8) | launch) & (E32 - 1)
    for epoch in (0, E24, E32 - E24, 5 * E24):
        assert all(tag(epoch, l) == l != 0 for l in (1, 2, 255))
    assert tag(E24 - 1, 7) >> 8 == E24 - 1 and tag(E32 - 1, 7) >> 8 == E24 - 1 and tag(E32, 7) == 7
