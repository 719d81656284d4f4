"""The hand-over tags and epochs at their wrap points, on handles whose age is set (zg_debug_gpt_age).

What ages ("What ages"): the device step counter the embed kernel advances — a decode tag carries its low 24 bits, and
the host zeroes the tagged words every 2^23 steps IT counts (note_steps) —, the 32-bit epoch of the whole-prompt c_attn GEMM's
stream-K flags, and the op tier's 32-bit completion number.  No test can run 2^24 steps; zg_debug_gpt_age runs the production
counting rule for n steps and adds n to the device word, zg_debug_gpt_age_state reads the counters, and zg_debug_gpt_tag_census
counts on the host the words that carry an epoch, so that "no stale word is left to match" is a fact, not a race won.

A  every call that runs decode steps moves the device epoch by no more than the host counted (four handle kinds), and a
   whole-prompt pass never moves it;
B  the stale high-split slot: a long step at epoch e, short steps, 2^24 steps of age, the long step again at e (mod 2^24) — at
   least one clear, no word of epoch e left in front of the step, logits and token bitwise the un-aged twin's, and the tapped
   step inside the float64 bounds of test_decode_stages_gpu.py (its checker, its bounds);
C  generations of 24 tokens from position 250 (across the split boundary at 256) that cross host count 2^23, device epoch 2^24
   (the tag's epoch field becomes 0: the launch id keeps the tag valid) and device epoch 2^32: tokens and log-probabilities
   bitwise the twin's, every fetch ZG_OK;
D  the stream-K epoch across 2^32 on a fresh handle: 0 is never handed to a launch, the flags are zeroed where the count begins
   again, no flag word holds the epoch a launch is about to get, every pass bitwise the twin's, the pass behind the wrap inside
   the float64 bounds of test_pass_stages_gpu.py;
E  the op tier's completion number across 2^32: results at test_ops_gpu.py's tolerance, no call that polled to the end.

The handles and what the library plans for them: handle_age_cases.py, asserted on the CPU in test_handle_age_cases_cpu.py.
Widths found with plan_case: mlp c_proj is K-sliced on the four-wave kernel (GR_PL4_KS, 4 slices, the only Linear that polls
sk_tag) from E = 512 in lock step, and on the matrix cores (GR_MFMA16_KS, 4 slices, by ticket) at E = 1600; one sequence splits K
on the vector ALUs (GR_KSPLIT) with no tag.  The fused launch hands over through qkv_tag alone, which every step rewrites: the
words that outlive short steps are part_tag's (splits above 0) and sk_tag's.  Stream-K: E 384, 4 x 256 rows on 16 workgroups
(24 tiles, 8 shared; 32 of the 512 flag words).

Measured on one MI355X (16 tests, 3.3 s together, the slowest 0.4 s): the long step leaves 384 words of its epoch in qkv_tag
(fused; none three short steps later), 396 in part_tag at batch 3 and 1320 at six splits, all still there three short steps
later, and none behind the clear the 2^24 - 4 steps of age enqueue; a generation of 5 + 21 columns advances the device epoch by
21 for 26 counted, a stop request that ends early by 3 .. 11 for 60; the stream-K passes are handed 2^32 - 1, 1, 2, each found in
32 flag words afterwards; the op tier takes one number per call through 2^32 - 1, 0, 1 and no call polls to the end.

Found by these tests' reading of the code, fixed in the same change: zg_gpt_time_kernel of class 0 replays the embed kernel, which
advances the epoch at each of its 64 (1 + ceil(iters / 64)) launches, and counted iters + 8 steps (128 against 9 at iters = 1);
the stream-K epoch wrapped to 0, the value of every flag word no launch has written, and then to values early launches left."""
import functools
from contextlib import contextmanager

import numpy as np
import pytest

import handle_age_cases as hc
import oracle
import pass_stage_cases as pc
import test_decode_stages_gpu as dstage
import test_pass_stages_gpu as pstage
from decode_stage_cases import Case, TOK_LO, VOCAB, make_tokens, make_weights, plan_case
from golden_io import assert_ref_close
from handle_age_cases import E23, E24, E32
from zig_gpt2_amd import _lib, ops, synth
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd.synth import GPTConfig

pytestmark = pytest.mark.gpu


def config(case):
    return GPTConfig(VOCAB, case.ctx, case.layers, case.heads, case.E)


@functools.lru_cache(maxsize=2)
def weights(case):
    return make_weights(case, config(case))


@contextmanager
def handles(case, monkeypatch, twin=True, use_graph=True, **kw):
    """A handle of the case (and an un-aged twin on the same weights); a fault or a timed-out hand-over ends the session."""
    monkeypatch.setenv("ZGPT2_DECODE_PATHS_OFF", str(case.off))
    m = zgpt.GPT(config(case), batch=case.batch, use_graph=use_graph, **kw)
    t = zgpt.GPT(config(case), batch=case.batch, use_graph=use_graph, share_weights_with=m, **kw) if twin else None
    try:
        m.load_weights(weights(case))
        yield m, t
    except _lib.ZgError as e:
        if e.code == -3:  # ZG_ERR_HIP: nothing more is started on this GPU by this session
            pytest.exit(f"{case.id}: {e}", returncode=3)
        raise
    finally:
        if t is not None:
            t.close()
        m.close()


def draw(rng, *shape):
    return rng.integers(TOK_LO, VOCAB - 1, size=shape).astype(np.uint64)


def modes_as_planned(m, case):
    _, info = m.step_taps(2, draw(np.random.default_rng(1), case.batch))
    want = plan_case(case)[0]
    assert {k: info[k] for k in want} == want, (info, want)
    return want


# ------------------------------------------------------------------ A: every epoch advance is counted
KINDS = {"fused batch 1": (Case(128, 1, layers=2), True, None), "lock step, tags": (Case(128, 3, layers=2), True, None),
         "no graph": (Case(128, 3, layers=2), False, None), "graph steps 8": (Case(128, 1, layers=2), True, "8")}


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.replace(" ", "-").replace(",", ""))
def test_every_epoch_advance_is_counted(zg, monkeypatch, kind):
    case, use_graph, graph_steps = KINDS[kind]
    if graph_steps:
        monkeypatch.setenv("ZGPT2_GRAPH_STEPS", graph_steps)
    B, rng = case.batch, np.random.default_rng(11)
    prompts = [draw(rng, 5) for _ in range(B)]
    toks = draw(rng, B)
    rows = draw(rng, B, 12)
    log = []

    def watch(what, steps, fn):
        s0 = m.age_state()
        out = fn()
        s1 = m.age_state()
        dev, host = (s1["device_epoch"] - s0["device_epoch"]) % E32, s1["steps_total"] - s0["steps_total"]
        print(f"AGE {kind} | {what} | device epoch +{dev} host count +{host}")
        log.append((what, steps, dev, host))
        return out

    with handles(case, monkeypatch, twin=False, use_graph=use_graph, score=True) as (m, _):
        modes = modes_as_planned(m, case)
        assert modes["tags"] or modes["fused"]
        watch("forward", True, lambda: [m.forward(t, toks) for t in (1, 2, 3)])
        greedy = watch("generate (26 = 5 prompt + 21: not a multiple of 8)", True, lambda: m.generate(prompts, 26))
        watch("generate_sample, top-k and top-p", True, lambda: m.generate_sample(prompts, 26, 0.9, seed=3, top_k=20, top_p=0.9))
        watch("prefill", False, lambda: m.prefill(rows[:, :6]))
        watch("extend", False, lambda: m.extend(6, rows[:, 6:10]))
        watch("generate_from behind extend", True, lambda: m.generate_from(10, [r[10:12] for r in rows], 13))
        watch("penalised request", True, lambda: m.generate_sample(prompts, 26, 1.0, seed=1, repetition_penalty=1.3, presence_penalty=0.2))
        watch("logprobs request", True, lambda: m.generate(prompts, 26, logprobs=3))
        stop_ids = sorted({int(greedy[b, 9]) for b in range(B)})
        watch("stop request", True, lambda: m.generate(prompts, 60, stop_token_ids=stop_ids, lookahead=2))
        end = m.stop_result()[0]
        assert end < 60, f"the stop request did not end early (end {end})"
        watch("zg_debug_gpt_step_taps", True, lambda: m.step_taps(7, toks))
        watch("zg_gpt_time_kernel, class 0 (the embed kernel advances the epoch itself)", True, lambda: m.time_kernel(0, 1))
        watch("zg_gpt_time_kernel, class 2 (one bump per replay)", True, lambda: m.time_kernel(2, 1))
        watch("zg_gpt_time_kernel, class 5, layers walked, 70 launches", True, lambda: m.time_kernel(5, 70, walk_layers=True))
        watch("zg_gpt_profile_step", True, lambda: m.profile_step(3, 2))
        watch("score", False, lambda: m.score(rows[:, :8]))
    for what, steps, dev, host in log:
        assert dev <= host, f"{kind}: {what} advanced the device epoch by {dev} and counted {host}"
        assert (dev >= 1) if steps else (dev == 0), f"{kind}: {what} advanced the device epoch by {dev}"


# ------------------------------------------------------------------ B: the stale high-split slot
@pytest.mark.parametrize("name", ["fused", "tags", "six-splits"])
def test_the_stale_high_split_slot(zg, monkeypatch, name):
    case = hc.DECODE[name]
    B, T = case.batch, case.seq_len
    prompt, toks = make_tokens(case)
    rng = np.random.default_rng(5)
    total = lambda c: c["sk_tag"] + c["part_tag"] + c["qkv_tag"]
    with handles(case, monkeypatch) as (m, twin):
        for g in (m, twin):
            g.prefill(prompt[:, :T - 1], compute_logits=False)
            g.forward(T, toks)  # the long step, at epoch e
        e = m.age_state()["device_epoch"]
        seen = m.tag_census(e % E24)
        print(f"AGE {case.id} | the long step ran at epoch {e}: words of that epoch {seen}")
        assert total(seen) > 0, "positive control: the census sees the tags of the step that just ran"
        for t in (2, 3, 4):  # short contexts, other tokens: one split, the high-split slots keep what the long step left
            short = draw(rng, B)
            for g in (m, twin):
                g.forward(t, short)
        left = m.tag_census(e % E24)
        print(f"AGE {case.id} | three short steps later: words of epoch {e} {left}")
        if plan_case(case)[0]["tags"]:
            assert left["part_tag"] > 0, "the partials of the splits above 0 outlive short steps: the words a reader 2^24 steps on would take"
        st = m.age_state()
        m.age(E24 - (st["device_epoch"] - e) - 1)  # the next step runs at e (mod 2^24)
        aged = m.age_state()
        print(f"AGE {case.id} | aged: {aged}")
        assert (aged["device_epoch"] + 1 - e) % E24 == 0 and aged["device_epoch"] > e
        assert aged["clears"] >= 1 and aged["clears"] > st["clears"], "2^24 - 4 counted steps must have enqueued a clear"
        assert total(m.tag_census(e % E24)) == 0, "a word of epoch e is left in front of the step that runs at e again"
        toks2 = draw(rng, B)
        taps, info = m.step_taps(T, toks2)
        token = m.argmax()
        lg_twin = twin.forward(T, toks2)
        assert m.age_state()["device_epoch"] % E24 == e % E24
        assert np.array_equal(token, twin.argmax())
        rep = dstage.Report(case)
        dstage.check_step(rep, case, config(case), weights(case), toks2, taps, info, token, lg_twin)  # (its last check: logits bitwise the twin's)
    assert not rep.failed, "\n".join([case.id] + rep.failed)


# ------------------------------------------------------------------ C: crossing the marks inside one call
MARKS = [("host count 2^23 - 3", "steps_since_clear", E23 - 3, None), ("device epoch 2^24 - 5", "device_epoch", E24 - 5, E24),
         ("device epoch 2^32 - 5", "device_epoch", E32 - 5, E32)]
CROSSINGS = [(n, True) for n in ("fused", "tags", "tickets", "pl4-ks", "mfma16-ks")] + [("fused", False), ("tags", False)]


def same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name,use_graph", CROSSINGS, ids=lambda v: v if isinstance(v, str) else ("graphs" if v else "no-graph"))
def test_a_generation_crosses_each_mark(zg, monkeypatch, name, use_graph):
    case = hc.DECODE[name]
    B, N, steps = case.batch, 274, 24
    prompts = [draw(np.random.default_rng(40 + b), 250) for b in range(B)]
    with handles(case, monkeypatch, use_graph=use_graph) as (m, twin):
        modes = modes_as_planned(m, case)
        ages = bool(modes["tags"] or modes["fused"])
        assert ages == (name != "tickets")
        want = twin.generate(prompts, N), twin.generate(prompts, N, logprobs=2)
        assert np.isfinite(want[1][1][:, 251:]).all()
        decode = lambda st: {k: st[k] for k in ("device_epoch", "steps_since_clear", "steps_total", "clears")}
        fresh = decode(m.age_state())
        for what, field, target, period in MARKS:
            s0 = m.age_state()
            m.age((target - s0[field]) % (period or E32))
            s1 = m.age_state()
            got = m.generate(prompts, N), m.generate(prompts, N, logprobs=2)  # (a timed-out hand-over: ZG_ERR_HIP from the fetch)
            s2 = m.age_state()
            print(f"AGE {case.id} graphs {int(use_graph)} | {what} | aged to {s1} | two generations later {s2}")
            assert np.array_equal(got[0], want[0]), f"{what}: tokens differ from the un-aged twin's"
            assert same(got[1], want[1]), f"{what}: tokens / log-probabilities / alternatives differ from the un-aged twin's"
            if not ages:
                assert decode(s1) == decode(s2) == fresh and not any(fresh.values()), "aging changed a handle without tags"
                continue
            assert s1[field] % (period or E32) == target
            assert (s2["device_epoch"] - s1["device_epoch"]) % E32 == 2 * steps and s2["steps_total"] - s1["steps_total"] == 2 * N
            if period is None:  # the clear goes in front of the steps of the call that crosses the mark: the first generation
                assert s2["clears"] == s1["clears"] + 1 and s2["steps_since_clear"] == 2 * N
            else:
                assert s2["device_epoch"] % period == 2 * steps - 5, "the generations did not cross the mark"


# ------------------------------------------------------------------ D: the stream-K epoch
def epochs_after(cur, n):
    """The epochs the next n stream-K launches must be handed: the count goes on, and 0 is left out."""
    out = []
    for _ in range(n):
        cur = (cur + 1) % E32 or 1
        out.append(cur)
    return out


def test_the_stream_k_epoch_crosses_2_32(zg, monkeypatch):
    case = hc.STREAM_K
    cfg = GPTConfig(pc.VOCAB, case.context, case.layers, case.heads, case.E)
    w = pc.make_weights(case, cfg)
    toks, _ = pc.make_tokens(case)
    monkeypatch.setenv("ZGPT2_GEMM_WGS", str(case.wgs))
    _lib.check(zg.zg_debug_prefill_route(*case.pin))
    m = zgpt.GPT(cfg, batch=case.batch)
    twin = zgpt.GPT(cfg, batch=case.batch, share_weights_with=m)
    rep = pstage.Report(case)
    try:
        m.load_weights(w)
        want = twin.extend(0, toks)
        assert m.tag_census(0, 0)["sk_flags"] == 512, "a fresh handle: every flag word is 0, the value the epoch must never take"
        m.age(sk_epoch=E32 - 2 * case.layers)
        handed = []
        for i in range(3):
            nxt = epochs_after(m.age_state()["sk_epoch"], case.layers)
            held = {v: m.tag_census(0, v)["sk_flags"] for v in nxt}
            assert not any(held.values()), f"pass {i}: flag words already hold an epoch this pass will be handed: {held}"
            if i == 1:  # the pass whose c_attn launch restarts the count: through the float64 stage check
                taps, info, lg = m.pass_taps(toks, compute_logits=True)
                pstage.check_pass(rep, case, w, toks, taps, info, lg)
            else:
                lg = m.extend(0, toks)
            st = m.age_state()
            print(f"AGE {case.id} | pass {i} | {st} | flag words holding it {m.tag_census(0, st['sk_epoch'])['sk_flags']}")
            handed.append(st["sk_epoch"])
            assert st["sk_epoch"] == nxt[-1] != 0
            assert m.tag_census(0, st["sk_epoch"])["sk_flags"] > 0, "positive control: the shared tiles' flag words hold the epoch just handed"
            assert lg.tobytes() == want.tobytes(), f"pass {i}: logits differ from the un-aged twin's"
        assert handed == [E32 - 1, 1, 2] and m.age_state()["sk_restarts"] == 1
        assert m.tag_census(0, 0)["sk_flags"] + m.tag_census(0, 2)["sk_flags"] == 512, "the flag words were zeroed where the count began again: they hold 0 or the last epoch"
    except _lib.ZgError as e:
        if e.code == -3:
            pytest.exit(f"{case.id}: {e}", returncode=3)
        raise
    finally:
        twin.close()
        m.close()
        zg.zg_debug_prefill_route(0, 0)
    assert not rep.failed, "\n".join([case.id] + rep.failed)


# ------------------------------------------------------------------ E: the op tier's completion number
def ops_state(zg):
    out = np.zeros(3, np.uint64)
    _lib.check(zg.zg_debug_ops_done_state(_lib.ptr(out), out.size))
    return dict(zip(("seq", "word", "missed"), (int(v) for v in out)))


def test_the_op_tier_completion_number_crosses_2_32(zg):
    """LayerNorm of <= 4 rows, gelu of <= 4096 elements and softmax announce their own completion; a Linear with a host output
    takes the separate completion launch behind its copy (elementwise.hip, api_ops.hip Call::finish)."""
    k, n, rows = 768, 3072, 3
    W = synth.fill_normal(100 + n, n * k, 0, 0.05).reshape(n, k)
    b = synth.fill_normal(200 + n, n, 0, 0.05)
    x = synth.fill_normal(300 + rows, rows * k, 0, 1.0).reshape(rows, k)
    gam, bet = synth.fill_normal(5, k, 1.0, 0.1), synth.fill_normal(6, k, 0.0, 0.1)
    v = synth.fill_normal(9, 3000, 0, 2.0)
    lin = ops.Linear(k, n, W, b)
    want_lin = oracle.linear_forward(k, n, W, b, x)

    def linear(i):
        y = np.zeros((rows, n), np.float32)
        lin.forward(x, y)
        assert_ref_close(want_lin, y, f"call {i}: Linear {rows}x{k}x{n}", scale_floor=2e-6)

    def layernorm(i):
        y = x.copy()
        ops.LayerNorm(k, gam, bet).forward(y)
        assert_ref_close(oracle.layernorm_forward(k, gam, bet, x), y, f"call {i}: LayerNorm")

    def gelu(i):
        y = v.copy()
        ops.gelu(y)
        assert_ref_close(oracle.gelu(v), y, f"call {i}: gelu")

    def softmax(i):
        y = v[:768].copy()
        ops.softmax(y)
        assert_ref_close(oracle.softmax(v[:768]), y, f"call {i}: softmax")

    linear(-1)  # (warm: the weight's staging is not part of what is counted below)
    before = ops_state(zg)
    _lib.check(zg.zg_debug_ops_set_done_seq(E32 - 3))
    assert ops_state(zg)["seq"] == E32 - 3
    for i, call in enumerate([layernorm, linear, gelu, linear, softmax, linear, layernorm, linear]):
        call(i)
        st = ops_state(zg)
        print(f"AGE op tier | call {i} {call.__name__} | {st}")
        assert st["missed"] == before["missed"], f"call {i} ({call.__name__}) polled to the end without seeing its number and drained the stream"
    assert 1 <= st["seq"] <= 16, "eight calls from 2^32 - 3 take at most two numbers each: the count is past 2^32"
