"""Per-row sampling parameters in the device loop and the per-token call (zg_gpt_generate_each_enqueue / zg_gpt_sample_each;
DESIGN §3.11).  The oracle is the existing uniform call on the same handle: sequences never interact, so row b of a per-row call
equals row b of generate_sample / sample given rows[b]'s parameters for every row — tokens, the log-probability record, finish
columns and reasons, probabilities — bit for bit.

The model has gpt_tiny's shapes with a context of 96, so that 80 steps cross a 64-position bucket; ragged prompts of 1 + 2 (b mod 3)
tokens make the loop leave and re-enter the alignment of its multi-step graphs.  The tables mix all five sampler forms, two
distinct penalty sets beside rows without, and distinct seeds."""
import ctypes as C

import numpy as np
import pytest

from penalty_ref import penalize_row
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu
CFG = synth.GPTConfig(257, 96, 2, 2, 128)
V = CFG.vocab_size
N_STEPS = 80
ARG, UNSUPPORTED = -6, -5
PEN_A = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.15)
PEN_B = dict(repetition_penalty=0.8, presence_penalty=-0.2, frequency_penalty=0.3)
ROWS8 = [
    dict(temp=0.8, seed=11),                                  # plain
    dict(temp=0.3, top_k=5, seed=12, **PEN_A),                # top-k, penalised
    dict(temp=1.7, top_p=0.6, seed=13),                       # top-p
    dict(temp=0.8, top_k=12, top_p=0.7, seed=14, **PEN_B),    # both, penalised otherwise
    dict(temp=0.8, min_p=0.05, seed=15),                      # min-p alone
    dict(temp=1.7, top_k=9, min_p=0.1, seed=16, **PEN_A),     # top-k + min-p
    dict(temp=0.8, top_p=0.8, min_p=0.05, seed=17),           # top-p + min-p
    dict(temp=0, seed=18),                                    # the row's greedy: temp 1, top_k 1
]
TABLES = {3: [ROWS8[3], ROWS8[0], ROWS8[4]], 8: ROWS8}
EDITS = dict(logit_bias={3: 2.5, 100: -4.0, 0: 1.0, V - 1: 0.5, 41: 3.0}, banned_token_ids=[7, 41, 200, 7])


@pytest.fixture(scope="module")
def weights():
    return synth.make_weights(CFG, seed=81, bf16=True)


def make(w, batch, **kw):
    m = zgpt.GPT(CFG, batch=batch, **kw)
    m.load_weights(w)
    return m


def ragged(batch, seed):
    return [synth.rand_tokens(seed + b, 1 + 2 * (b % 3), V) for b in range(batch)]


def uniform_kw(row):
    """A row of a table as the keyword arguments of the uniform calls (a row's temp 0 is top_k 1 at temp 1 there too)."""
    kw = {k: v for k, v in row.items() if k != "temp"}
    temp = row.get("temp", 1.0)
    if not temp:
        temp, kw["top_k"] = 1.0, 1
    return temp, kw


def uniform_rows(m, prompts, n, rows, **call):
    """[what generate_sample(rows[b]'s parameters for every row, **call) returns, for every b]"""
    out = []
    for row in rows:
        temp, kw = uniform_kw(row)
        out.append(m.generate_sample(prompts, n, temp, **kw, **call))
    return out


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("batch,graph,at_create", [(3, True, True), (3, False, False), (8, True, False)])
def test_every_row_equals_the_uniform_generation_with_its_parameters(zg, weights, batch, graph, at_create):
    flags = dict(truncated_generate=True, penalized_generate=True, edited_generate=True, logprobs_generate=True, stop_generate=True) if at_create else {}
    m = make(weights, batch, use_graph=graph, **flags)
    prompts, rows = ragged(batch, 910), TABLES[batch]
    before = m.generate_sample(prompts, N_STEPS, 0.8, seed=5, top_k=7, top_p=0.9, **PEN_A)
    got = m.generate_each(prompts, N_STEPS, rows)
    want = uniform_rows(m, prompts, N_STEPS, rows)
    assert np.array_equal(got, m.generate_each(prompts, N_STEPS, rows)), "the same call twice"
    for b in range(batch):
        assert np.array_equal(got[b], want[b][b]), (b, rows[b], np.flatnonzero(got[b] != want[b][b])[:4])
        assert np.array_equal(got[b, : len(prompts[b])], prompts[b])
    # teeth: the rows' own parameters matter — most rows differ from what rows[0]'s parameters give them
    assert sum(not np.array_equal(got[b], want[0][b]) for b in range(1, batch)) >= (batch - 1 + 1) // 2
    # with the log-probability record
    got_lp = m.generate_each(prompts, N_STEPS, rows, logprobs=5)
    want_lp = uniform_rows(m, prompts, N_STEPS, rows, logprobs=5)
    for b in range(batch):
        assert np.array_equal(got_lp[0][b], got[b])
        picked = ~np.isnan(want_lp[b][1][b])
        assert np.array_equal(np.isnan(got_lp[1][b]), ~picked)
        assert np.array_equal(u32(got_lp[1][b][picked]), u32(want_lp[b][1][b][picked])), (b, "logprob")
        assert np.array_equal(got_lp[2][b][picked], want_lp[b][2][b][picked]), (b, "top ids")
        assert np.array_equal(u32(got_lp[3][b][picked]), u32(want_lp[b][3][b][picked])), (b, "top logprobs")
    # with per-call edits
    got_ed = m.generate_each(prompts, N_STEPS, rows, **EDITS)
    want_ed = uniform_rows(m, prompts, N_STEPS, rows, **EDITS)
    for b in range(batch):
        assert np.array_equal(got_ed[b], want_ed[b][b]), (b, "edits")
        assert not set(int(t) for t in got_ed[b, len(prompts[b]):]) & {7, 41, 200}, "a banned token was picked"
    assert not np.array_equal(got_ed, got), "the edits changed nothing"
    # an ordinary uniform generation behind per-row ones returns what it returned before them
    assert np.array_equal(m.generate_sample(prompts, N_STEPS, 0.8, seed=5, top_k=7, top_p=0.9, **PEN_A), before)
    m.close()


def test_stop_conditions_finish_every_row_where_its_uniform_call_does(zg, weights):
    batch = 3
    m = make(weights, batch)
    prompts, rows = ragged(batch, 930), TABLES[batch]
    free = m.generate_each(prompts, N_STEPS, rows)
    stop_ids = [int(free[b, 20 + 7 * b]) for b in range(batch)]
    seqs = [[int(free[1, 30]), int(free[1, 31])]]
    got = m.generate_each(prompts, N_STEPS, rows, stop_token_ids=stop_ids, stop=seqs)
    end, fin, why = m.stop_result()
    assert got.shape[1] == end and np.array_equal(got, free[:, :end])
    assert all(f is not None for f in fin)
    for b in range(batch):
        temp, kw = uniform_kw(rows[b])
        cut = m.generate_sample(prompts, N_STEPS, temp, stop_token_ids=stop_ids, stop=seqs, **kw)
        end_b, fin_b, why_b = m.stop_result()
        e = min(end, end_b)  # (`end` may differ from run to run inside its bound, nothing else may)
        assert np.array_equal(cut[b, :e], got[b, :e]), b
        assert (fin[b], why[b]) == (fin_b[b], why_b[b]), (b, fin, fin_b, why, why_b)
    m.close()


def test_a_continuation_behind_extend_and_on_a_handle_without_prefill(zg, weights):
    batch, past, n = 3, 13, 60
    first = np.stack([synth.rand_tokens(920 + b, past, V) for b in range(batch)])
    turns = [synth.rand_tokens(940 + b, 2 + 3 * (b % 2), V) for b in range(batch)]
    prior = [first[b] for b in range(batch)]  # (the tokens below past_len count only as prior)
    rows = TABLES[batch]
    for kw in (dict(), dict(prefill=False)):
        m = make(weights, batch, **kw)
        feed = (lambda: m.extend(0, first, compute_logits=False)) if not kw else (lambda: m.generate(list(first), past))
        feed()
        got = m.generate_each(turns, n, rows, past_len=past, prior=prior)
        assert m.cached_len() == past + n
        for b in range(batch):
            temp, ukw = uniform_kw(rows[b])
            feed()
            want = m.generate_from(past, turns, n, temp=temp, prior=prior, **ukw)
            assert np.array_equal(got[b], want[b]), (kw, b, np.flatnonzero(got[b] != want[b])[:4])
        m.close()


@pytest.mark.parametrize("entry", [0, 1, 3, 4])
def test_a_table_of_equal_entries_is_the_uniform_call(zg, weights, entry):
    batch = 3
    m = make(weights, batch)
    prompts, row = ragged(batch, 950), ROWS8[entry]
    temp, kw = uniform_kw(row)
    want = m.generate_sample(prompts, N_STEPS, temp, logprobs=3, **kw)
    got = m.generate_each(prompts, N_STEPS, [row] * batch, logprobs=3)
    assert np.array_equal(got[0], want[0])
    picked = ~np.isnan(want[1])
    assert np.array_equal(np.isnan(got[1]), ~picked) and np.array_equal(u32(got[1][picked]), u32(want[1][picked]))
    assert np.array_equal(got[2][picked], want[2][picked]) and np.array_equal(u32(got[3][picked]), u32(want[3][picked]))
    m.close()


def raw_each(zg, m, prompts, n, table, n_rows, opt=None, pen=None, edits=None):
    mat, lens, stride = m._prompts(prompts)
    r = _lib.generate_request(prompts=_lib.ptr(mat), prompt_stride=stride, prompt_lens=_lib.ptr(lens), n_steps=n,
                              options=None if opt is None else C.addressof(opt), penalties=None if pen is None else C.addressof(pen),
                              edits=None if edits is None else C.addressof(edits))
    return zg.zg_gpt_generate_each_enqueue(m.h, C.addressof(r), None if table is None else C.addressof(table), n_rows)


def test_refusals_leave_the_handle_and_the_record_alone(zg, weights):
    batch, n = 3, 24
    m = make(weights, batch)
    prompts, rows = ragged(batch, 970), TABLES[batch]
    got = m.generate_each(prompts, n, rows)
    assert m.cached_len() == n
    good = _lib.row_sampling(rows)
    opt, pen = _lib.SampleOptions(0.8, 5, 1.0), _lib.LogitPenalties(1.3, 0.0, 0.0)
    bad_rows = []
    for at, change in ((0, dict(temp=-1.0)), (1, dict(top_p=0.0)), (2, dict(min_p=1.0)), (1, dict(repetition_penalty=0.0)), (2, dict(frequency_penalty=float("nan")))):
        t = [dict(r) for r in rows]
        t[at] = dict(t[at], **change)
        bad_rows.append((at, _lib.row_sampling(t)))
    for at, table in bad_rows:
        assert raw_each(zg, m, prompts, 30, table, batch) == ARG and f"row {at}" in zg.zg_last_error().decode(), zg.zg_last_error()
        assert m.cached_len() == n
    cases = [
        raw_each(zg, m, prompts, 30, good, batch - 1), raw_each(zg, m, prompts, 30, good, batch + 1), raw_each(zg, m, prompts, 30, None, batch),
        raw_each(zg, m, prompts, 30, good, batch, opt=opt), raw_each(zg, m, prompts, 30, good, batch, pen=pen),
        raw_each(zg, m, prompts, 30, good, batch, edits=_lib.LogitEdits(None, None, 0, None, 0, None, 0, 0.1)),
    ]
    assert cases == [ARG] * len(cases), cases
    r = _lib.generate_request()
    r.size -= 8
    assert zg.zg_gpt_generate_each_enqueue(m.h, C.addressof(r), C.addressof(good), batch) == ARG
    # the per-token twin refuses the same, before the forward
    tok, out = np.array([1, 2, 3], np.uint64), np.zeros(batch, np.uint64)
    assert zg.zg_gpt_sample_each(m.h, n + 1, _lib.ptr(tok), batch, C.addressof(good), batch - 1, None, 0, None, None, None, _lib.ptr(out), None, 0) == ARG
    assert zg.zg_gpt_sample_each(m.h, n + 1, _lib.ptr(tok), batch, None, batch, None, 0, None, None, None, _lib.ptr(out), None, 0) == ARG
    assert zg.zg_gpt_sample_each(m.h, n + 1, _lib.ptr(tok), batch, C.addressof(bad_rows[2][1]), batch, None, 0, None, None, None, _lib.ptr(out), None, 0) == ARG
    assert "row 2" in zg.zg_last_error().decode()
    assert m.cached_len() == n and np.array_equal(m.generate_fetch_range(0, n), got)
    assert np.array_equal(m.generate_each(prompts, n, rows), got)  # and the handle still works
    m.close()


def test_a_penalised_row_on_a_context_beyond_the_cap_is_unsupported(zg):
    cfg = synth.GPTConfig(257, 8192 + 64, 1, 2, 128)
    m = zgpt.GPT(cfg, batch=1, use_graph=False, prefill=False)
    one, out = np.array([3], np.uint64), np.zeros(1, np.uint64)
    pen, off = _lib.row_sampling([dict(temp=0.8, **PEN_A)]), _lib.row_sampling([dict(temp=0.8, top_k=5)])
    assert raw_each(zg, m, [one], 4, pen, 1) == UNSUPPORTED and m.cached_len() == 0
    assert zg.zg_gpt_sample_each(m.h, 1, _lib.ptr(one), 1, C.addressof(pen), 1, None, 0, None, None, None, _lib.ptr(out), None, 0) == UNSUPPORTED
    assert m.cached_len() == 0
    assert raw_each(zg, m, [one], 4, off, 1) == 0  # (no row penalised: nothing knows the cap)
    m.close()


# ---- the per-token call

def test_sample_each_equals_sample_row_by_row(zg, weights):
    batch = 8
    m = make(weights, batch)
    rows = ROWS8
    rng = np.random.default_rng(3)
    hist = [rng.integers(0, V, n) for n in (0, 1, 40, 60, 5, 17, 3, 9)]
    m.generate(ragged(batch, 990), 9)  # positions 0 .. 8 cached
    toks = rng.integers(0, V, batch)
    for uniforms in (rng.random(batch).astype(np.float32), None):
        got, probs = m.sample_each(10, toks, rows, uniforms=uniforms, history=hist, want_probs=True)
        assert np.array_equal(m.sample_each(10, toks, rows, uniforms=uniforms, history=hist), got)
        for b, row in enumerate(rows):
            temp, kw = uniform_kw(row)
            want, wprobs = m.sample(10, toks, temp, uniforms=uniforms, history=hist, want_probs=True, **kw)
            assert int(got[b]) == int(want[b]), (b, row)
            assert np.array_equal(u32(probs[b]), u32(wprobs[b])), (b, row, np.flatnonzero(u32(probs[b]) != u32(wprobs[b]))[:5])
        assert len({int(t) for t in got}) > 1
    # behind a penalised row, argmax() is the argmax of its penalised row; an unpenalised row keeps the raw one
    raw = m.forward(10, toks)
    m.sample_each(10, toks, rows, history=hist)
    top = m.argmax()
    for b, row in enumerate(rows):
        x = penalize_row(raw[b], hist[b], row.get("repetition_penalty", 1.0), row.get("presence_penalty", 0.0), row.get("frequency_penalty", 0.0))[0]
        assert int(top[b]) == int(np.argmax(x)), b
    # with per-call edit lists
    got = m.sample_each(10, toks, rows, history=hist, banned_token_ids=[int(t) for t in top], logit_bias={5: 2.0})
    for b, row in enumerate(rows):
        temp, kw = uniform_kw(row)
        assert int(got[b]) == int(m.sample(10, toks, temp, history=hist, banned_token_ids=[int(t) for t in top], logit_bias={5: 2.0}, **kw)[b]), b
    m.close()
