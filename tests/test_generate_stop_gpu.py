"""zg_gpt_generate_stop_enqueue: stop tokens and stop sequences in the device loop, with an early end (include/zgpt2.h).

Every case first runs the twin without conditions, then chooses its conditions FROM THE TWIN'S OWN TOKENS, so that a match is
certain; the expected finish columns and reasons come from tests/stop_ref.py on the twin's tokens.  The model has gpt_tiny's shapes
with a context of 96, so that 80 steps cross a 64-position bucket; ragged prompts of 1 + 2 (b mod 3) tokens make the loop leave and
re-enter the alignment of its multi-step graphs."""
import ctypes as C

import numpy as np
import pytest

import stop_ref
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu
CFG = synth.GPTConfig(257, 96, 2, 2, 128)
N_STEPS = 80
LOOKAHEAD = 8
ERR_ARG, ERR_SHAPE = -6, -2
PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.15)
TAILS = {
    "greedy": dict(),
    "temp": dict(temp=0.8, seed=5),
    "topk_topp_pen_lp": dict(temp=0.8, seed=9, top_k=12, top_p=0.8, logprobs=5, **PEN),
}


@pytest.fixture(scope="module")
def weights():
    return synth.make_weights(CFG, seed=81, bf16=True)


def make(w, batch, **kw):
    m = zgpt.GPT(CFG, batch=batch, **kw)
    m.load_weights(w)
    return m


def ragged(batch, seed):
    return [synth.rand_tokens(seed + b, 1 + 2 * (b % 3), CFG.vocab_size) for b in range(batch)]


def split(out):
    """(tokens, log-probability record or None) of what a generate call returned"""
    return (out[0], out[1:]) if isinstance(out, tuple) else (out, None)


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


def conditions_from(twin, prompts):
    """Conditions every row is certain to meet before column 25: the token row b picks at column 9 + 4 b, and the three tokens row 0
    holds at columns 20 .. 22 as a sequence."""
    ids = [int(twin[b, 9 + 4 * b]) for b in range(len(prompts))]
    return ids, [[int(t) for t in twin[0, 20:23]]]


def check_stopped(m, got, twin, twin_lp, first_cols, ids, seqs, lookahead, past=0):
    """got: what the stop generation returned (cut at end); twin: the same call's tokens without conditions, columns past .. ."""
    end, cols, reasons = m.stop_result()
    tok, lp = split(got)
    want_cols, want_reasons = stop_ref.finish(twin, [f - past for f in first_cols], ids, seqs)
    want_cols = [None if c is None else c + past for c in want_cols]
    print(f"stop: end {end}, finish columns {cols} (reference {want_cols}), reasons {reasons}")
    assert cols == want_cols and reasons == want_reasons
    if all(c is not None for c in want_cols):
        f = max(want_cols)
        assert f + 1 <= end <= min(past + twin.shape[1], f + 1 + lookahead + 64), (end, f)
    else:
        assert end == past + twin.shape[1]
    assert m.cached_len() == end
    assert tok.shape == (twin.shape[0], end - past) and np.array_equal(tok, twin[:, : end - past]), np.argwhere(tok != twin[:, : end - past])[:4]
    if twin_lp is not None:
        assert same_bits(lp, [a[:, : end - past] for a in twin_lp]), "log-probability columns below end differ from the twin's"
    return end, cols, reasons


@pytest.mark.parametrize("tail", list(TAILS))
@pytest.mark.parametrize("batch,graph", [(1, True), (1, False), (3, True)])
def test_stops_early_with_the_twins_tokens(zg, weights, batch, graph, tail):
    prompts = ragged(batch, 810)
    mode = TAILS[tail]
    m = make(weights, batch, use_graph=graph)
    twin, twin_lp = split(m.generate_from(0, prompts, N_STEPS, **mode))
    ids, seqs = conditions_from(twin, prompts)
    first_cols = [len(p) for p in prompts]
    got = m.generate_from(0, prompts, N_STEPS, stop_token_ids=ids, stop=seqs, lookahead=LOOKAHEAD, **mode)
    end, cols, reasons = check_stopped(m, got, twin, twin_lp, first_cols, ids, seqs, LOOKAHEAD)
    assert all(c is not None and c < 25 for c in cols) and end < N_STEPS  # the early end happened
    again = m.generate_from(0, prompts, N_STEPS, stop_token_ids=ids, stop=seqs, lookahead=LOOKAHEAD, **mode)
    end2, cols2, reasons2 = m.stop_result()
    n = min(end, end2)
    assert cols2 == cols and reasons2 == reasons and np.array_equal(split(again)[0][:, :n], split(got)[0][:, :n])
    behind, behind_lp = split(m.generate_from(0, prompts, N_STEPS, **mode))
    assert np.array_equal(behind, twin), "an ordinary generation behind a stopped one"
    assert twin_lp is None or same_bits(behind_lp, twin_lp)
    assert m.cached_len() == N_STEPS
    m.close()


def test_prompts_through_the_whole_prompt_pass(zg, weights):
    B = 2
    prompts = [synth.rand_tokens(840 + b, 6 + b, CFG.vocab_size) for b in range(B)]  # >= 4 tokens each: the whole-prompt pass feeds them
    mode = TAILS["temp"]
    m = make(weights, B)
    twin = m.generate_from(0, prompts, N_STEPS, **mode)
    # row 0's first pick (column 6, right behind the whole-prompt pass) is a stop token; row 1 finishes at column 15 at the latest
    ids = [int(twin[0, 6]), int(twin[1, 15])]
    seqs = [[int(t) for t in twin[1, 5:8]]]  # reaches into row 1's prompt (columns 0 .. 6): never a match there
    got = m.generate_from(0, prompts, N_STEPS, stop_token_ids=ids, stop=seqs, lookahead=LOOKAHEAD, **mode)
    end, cols, _ = check_stopped(m, got, twin, None, [6, 7], ids, seqs, LOOKAHEAD)
    m.close()
    assert cols[0] == 6 and cols[1] is not None and 7 <= cols[1] <= 15 and end < N_STEPS


def test_a_lookahead_beyond_the_context_never_waits(zg, weights):
    prompts = ragged(3, 845)
    m = make(weights, 3)
    twin = m.generate(prompts, N_STEPS)
    ids, seqs = conditions_from(twin, prompts)
    for lookahead in (CFG.context_size, (1 << 64) - 1):
        got = m.generate(prompts, N_STEPS, stop_token_ids=ids, stop=seqs, lookahead=lookahead)
        end, cols, _ = check_stopped(m, got, twin, None, [len(p) for p in prompts], ids, seqs, CFG.context_size)
        assert all(c is not None for c in cols) and max(cols) + 1 <= end <= N_STEPS
    m.close()


def unpicked_id(twin):
    """a token no row of the twin holds anywhere"""
    return next(t for t in range(CFG.vocab_size) if not (twin == t).any())


@pytest.mark.parametrize("tail", ["greedy", "topk_topp_pen_lp"])
def test_conditions_that_never_match_run_to_the_end(zg, weights, tail):
    prompts = ragged(3, 850)
    mode = TAILS[tail]
    m = make(weights, 3)
    twin, twin_lp = split(m.generate_from(0, prompts, N_STEPS, **mode))
    absent = unpicked_id(twin)
    ids, seqs = [absent], [[int(twin[0, 30]), absent]]
    got = m.generate_from(0, prompts, N_STEPS, stop_token_ids=ids, stop=seqs, lookahead=LOOKAHEAD, **mode)
    end, cols, reasons = check_stopped(m, got, twin, twin_lp, [len(p) for p in prompts], ids, seqs, LOOKAHEAD)
    m.close()
    assert end == N_STEPS and cols == [None] * 3 and reasons == [-1] * 3


def test_one_row_of_three_never_finishes(zg, weights):
    prompts = ragged(3, 860)
    m = make(weights, 3)
    twin = m.generate(prompts, N_STEPS)
    # tokens rows 0 and 2 pick early which row 1 never holds (searched on the twin)
    ids = []
    for b in (0, 2):
        ids.append(next(int(twin[b, c]) for c in range(len(prompts[b]), N_STEPS) if not (twin[1] == twin[b, c]).any()))
    got = m.generate(prompts, N_STEPS, stop_token_ids=ids, lookahead=LOOKAHEAD)
    end, cols, reasons = check_stopped(m, got, twin, None, [len(p) for p in prompts], ids, [], LOOKAHEAD)
    m.close()
    assert end == N_STEPS and cols[1] is None and cols[0] is not None and cols[2] is not None and reasons[1] == -1


def test_graphs_at_create_lazily_or_not_at_all(zg, weights):
    prompts = ragged(3, 870)
    results = []
    ids = seqs = None
    for kw in (dict(stop_generate=True, sampled_generate=True), dict(), dict(use_graph=False)):
        m = make(weights, 3, **kw)
        if ids is None:
            ids, seqs = conditions_from(m.generate_sample(prompts, N_STEPS, 0.8, seed=7), prompts)
        rec = []
        for mode in (dict(temp=0.8, seed=7), dict()):
            tok = m.generate_from(0, prompts, N_STEPS, stop_token_ids=ids, stop=seqs, lookahead=LOOKAHEAD, **mode)
            rec.append((tok,) + m.stop_result())
        m.close()
        results.append(rec)
    for other in results[1:]:
        for (tok, end, cols, reasons), (tok0, end0, cols0, reasons0) in zip(other, results[0]):
            n = min(end, end0)
            assert cols == cols0 and reasons == reasons0 and np.array_equal(tok[:, :n], tok0[:, :n])
    assert all(c is not None for c in results[0][0][2]) and results[0][0][1] < N_STEPS


def test_behind_an_extend_columns_are_absolute_and_nothing_matches_across_the_turn(zg, weights):
    B, past, n = 2, 13, 60
    first = np.stack([synth.rand_tokens(820 + b, past, CFG.vocab_size) for b in range(B)])
    turns = [synth.rand_tokens(830 + b, 1 + 2 * b, CFG.vocab_size) for b in range(B)]  # 1 and 3 new tokens: through the decode loop
    mode = TAILS["temp"]
    m = make(weights, B)
    m.extend(0, first, compute_logits=False)
    twin = m.generate_from(past, turns, n, **mode)
    # sequence 0 ends at row 0's first pick and begins in the cached turn: it must not match; sequence 1 lies wholly in the picks
    seqs = [[int(first[0, past - 1]), int(twin[0, 0]), int(twin[0, 1])], [int(t) for t in twin[0, 12:14]]]
    ids = [int(twin[1, 20])]
    m.generate(list(first), past)  # the record below past_len now holds the cached turn itself: still nothing to match across
    m.extend(0, first, compute_logits=False)
    got = m.generate_from(past, turns, n, stop_token_ids=ids, stop=seqs, lookahead=LOOKAHEAD, **mode)
    end, cols, reasons = check_stopped(m, got, twin, None, [past + len(t) for t in turns], ids, seqs, LOOKAHEAD, past=past)
    assert all(c is not None and c > past for c in cols) and not (cols[0] == past + 1 and reasons[0] == 1) and end < past + n
    # a continuation rolls back below the end as after any other call
    more = m.generate_from(end - 2, [twin[b, end - 2 - past: end - past] for b in range(B)], 6, **mode)
    assert more.shape == (B, 6) and m.cached_len() == end + 4
    m.close()


def test_empty_conditions_are_the_calls_without(zg, weights):
    prompts = ragged(3, 880)
    m = make(weights, 3)
    mat, lens, stride = m._prompts(prompts)
    opt = _lib.SampleOptions(0.8, 12, 0.8)
    pen = _lib.LogitPenalties(1.3, 0.4, 0.15)
    empty = _lib.StopConditions(None, 0, None, 0, None, 0, 8)

    def raw(opt_p, pen_p, logprobs, top_n, stop_p):
        _lib.check(zg.zg_gpt_generate_stop_enqueue(m.h, 0, _lib.ptr(mat), stride, _lib.ptr(lens), N_STEPS, opt_p, pen_p, None, 0, None, 9, logprobs, top_n, stop_p))

    want = m.generate_sample(prompts, N_STEPS, 0.8, seed=9, top_k=12, top_p=0.8, logprobs=5, **PEN)
    for stop_p in (None, C.addressof(empty)):
        raw(C.addressof(opt), C.addressof(pen), 1, 5, stop_p)
        assert m.cached_len() == N_STEPS
        assert np.array_equal(m.generate_fetch(N_STEPS), want[0]) and same_bits(m.generate_fetch_logprobs(0, N_STEPS, 5), want[1:])
        with pytest.raises(_lib.ZgError):
            m.stop_result()  # not a generation with conditions
    want = m.generate_sample(prompts, N_STEPS, 0.8, seed=9, top_k=12, top_p=0.8, **PEN)
    raw(C.addressof(opt), C.addressof(pen), 0, 5, C.addressof(empty))
    assert np.array_equal(m.generate_fetch(N_STEPS), want)
    want = m.generate(prompts, N_STEPS)
    raw(None, None, 0, 0, None)
    assert np.array_equal(m.generate_fetch(N_STEPS), want)
    m.close()


def test_refusals_touch_nothing(zg, weights):
    prompts = ragged(2, 890)
    m = make(weights, 2)
    mat, lens, stride = m._prompts(prompts)
    end, cols, reasons = C.c_size_t(), np.zeros(2, np.uint64), np.zeros(2, np.int32)
    assert zg.zg_gpt_generate_stop_result(m.h, C.byref(end), _lib.ptr(cols), _lib.ptr(reasons)) == ERR_ARG  # before any stop generation
    recorded = m.generate(prompts, 30, logprobs=5)

    def enqueue(ids=None, seqs=None, opt=None, pen=None, raw_conds=None):
        conds, keep = _lib.stop_conditions(ids, seqs)
        if raw_conds is not None:
            conds = raw_conds
        return zg.zg_gpt_generate_stop_enqueue(m.h, 0, _lib.ptr(mat), stride, _lib.ptr(lens), 20, None if opt is None else C.addressof(opt),
                                               None if pen is None else C.addressof(pen), None, 0, None, 1, 1, 5, C.addressof(conds))

    one = np.ascontiguousarray([1, 2], np.uint64)
    lens2 = np.ascontiguousarray([2], np.uint64)
    assert enqueue(ids=list(range(17))) == ERR_ARG
    assert enqueue(seqs=[[1]] * 9) == ERR_ARG
    assert enqueue(seqs=[list(range(17))]) == ERR_ARG
    assert enqueue(raw_conds=_lib.StopConditions(None, 0, _lib.ptr(one), 1, _lib.ptr(lens2), 1, 0)) == ERR_ARG  # longer than the stride
    lens2[0] = 0
    assert enqueue(raw_conds=_lib.StopConditions(None, 0, _lib.ptr(one), 2, _lib.ptr(lens2), 1, 0)) == ERR_ARG  # a sequence of length 0
    assert enqueue(raw_conds=_lib.StopConditions(None, 2, None, 0, None, 0, 0)) == ERR_ARG                      # a NULL array with a count
    assert enqueue(ids=[CFG.vocab_size]) == ERR_SHAPE
    assert enqueue(seqs=[[1, CFG.vocab_size]]) == ERR_SHAPE
    assert enqueue(ids=[1], pen=_lib.LogitPenalties(1.3, 0.0, 0.0)) == ERR_ARG  # greedy with penalties
    assert m.cached_len() == 30
    assert same_bits(m.generate_fetch_logprobs(0, 30, 5), recorded[1:]), "a refused call touched the log-probability record"
    assert zg.zg_gpt_generate_stop_result(m.h, C.byref(end), _lib.ptr(cols), _lib.ptr(reasons)) == ERR_ARG
    assert enqueue(ids=[CFG.vocab_size - 1], seqs=[[1, 2]]) == 0
    assert zg.zg_gpt_generate_stop_result(m.h, C.byref(end), _lib.ptr(cols), _lib.ptr(reasons)) == 0 and end.value == m.cached_len()
    m.close()
