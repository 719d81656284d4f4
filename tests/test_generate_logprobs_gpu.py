"""zg_gpt_generate_logprobs_enqueue: the device loop with the log-probability stage in its captured step.  The tokens
are bitwise those of the same generation without the stage; every picked column matches a host loop that feeds the same tokens
through GPT.forward, applies the penalties of the mode in numpy float32 (tests/penalty_ref.py) and takes the float64 reference of
tests/logprob_ref.py: ids exactly, values within 1e-5 + 2.5e-7 |ref|; prompt columns read NaN.

Exact ids rest on the host loop's logits being bit for bit the device loop's: the host loop feeds position by position through the
decode kernels, as the device loop does for the ragged prompts of 1 + 2 (b mod 3) tokens, and where the device loop takes the
whole-prompt pass (prompts of 6 and 7 tokens) the host loop fills its caches with GPT.prefill over the same positions first.

The model has gpt_tiny's shapes with a context of 96, so that 80 steps cross a 64-position bucket."""
import ctypes as C

import numpy as np
import pytest

from logprob_ref import check_values, logprob_ref
from penalty_ref import penalize_row, same_bits
from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu
CFG = synth.GPTConfig(257, 96, 2, 2, 128)
N_STEPS = 80
PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.15)  # those of tests/test_generate_pen_gpu.py
ERR_SHAPE, ERR_ARG = -2, -6
# name -> keyword arguments of GPT.generate_from (temp None: greedy)
MODES = {
    "greedy": dict(temp=None),
    "temp": dict(temp=0.8, seed=5),
    "topk_topp": dict(temp=0.8, seed=9, top_k=12, top_p=0.8),
    "topk_pen": dict(temp=0.8, seed=7, top_k=7, **PEN),
}
TOP_NS = [0, 5, 20]


@pytest.fixture(scope="module")
def weights():
    return synth.make_weights(CFG, seed=81, bf16=True)


def make(w, batch, **kw):
    m = zgpt.GPT(CFG, batch=batch, **kw)
    m.load_weights(w)
    return m


def ragged(batch, seed):
    return [synth.rand_tokens(seed + b, 1 + 2 * (b % 3), CFG.vocab_size) for b in range(batch)]


def host_reference(m, prompts, tokens, mode, past=0, prefilled=0, prior=None):
    """The float64 reference of every column of `tokens` [B, n] (the device loop's record of positions past .. past + n - 1): the
    loop feeds what the device loop fed, position by position from `prefilled` on (the caches below hold the same positions
    already), and at every column a row picked takes the logits, penalises them as the mode says and asks logprob_ref about the
    recorded token.  Returns (logprob [B, n] with NaN at prompt columns, top_ids [B, n, 20], top_logprobs [B, n, 20])."""
    B, n = tokens.shape
    pen = {k.split("_")[0]: v for k, v in mode.items() if k.endswith("_penalty")}
    lp = np.full((B, n), np.nan)
    ids = np.zeros((B, n, 20), np.int64)
    top = np.zeros((B, n, 20))
    min_np = min(len(p) for p in prompts)
    for i in range(prefilled, n):
        fed = [int(p[i]) if i < len(p) else (int(p[-1]) if i == len(p) else int(tokens[b, i - 1])) for b, p in enumerate(prompts)]
        if i < min_np:
            m.forward(past + i + 1, fed, compute_logits=False)
            continue
        logits = m.forward(past + i + 1, fed, want_logits=True)
        for b, p in enumerate(prompts):
            if i < len(p):
                continue  # the column records a prompt token
            x = logits[b]
            if pen:  # §3.6: the prior, then what positions past .. i - 1 recorded
                hist = np.r_[np.asarray([] if prior is None else prior[b], np.uint64), tokens[b, :i]]
                x = penalize_row(x, hist, **pen)[0]
            lp[b, i], ids[b, i], top[b, i] = logprob_ref(x, tokens[b, i], 20)
    return lp, ids, top


def check_against(got, ref, prompts, top_n, tag):
    """(tokens, logprobs, top_ids, top_logprobs) of the device against host_reference's: NaN exactly at the prompt columns, ids
    exact, values within the bound.  Returns the largest |got - ref| / bound."""
    _, lp, ids, top = got
    rlp, rids, rtop = ref
    picked = ~np.isnan(rlp)
    for b, p in enumerate(prompts):
        assert not picked[b, : len(p)].any() and picked[b, len(p):].all()
    assert np.array_equal(np.isnan(lp), ~picked), (tag, np.argwhere(np.isnan(lp) == picked)[:4])
    assert ids.shape == picked.shape + (top_n,) and top.shape == ids.shape
    assert np.array_equal(ids[picked].astype(np.int64), rids[picked][:, :top_n]), (tag, np.argwhere(ids[picked].astype(np.int64) != rids[picked][:, :top_n])[:4])
    worst = check_values(lp[picked], rlp[picked])
    return max(worst, check_values(top[picked], rtop[picked][:, :top_n])) if top_n else worst


def same_record(a, b):
    return all(np.array_equal(x, y) if x.dtype.kind in "ui" else same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("batch,graph,modes", [(1, True, list(MODES)), (1, False, list(MODES)), (3, True, list(MODES)), (8, True, ["greedy", "topk_pen"])])
def test_device_loop_against_host_loop(zg, weights, batch, graph, modes):
    prompts = ragged(batch, 910)
    m = make(weights, batch, use_graph=graph)
    worst = 0.0
    for name in modes:
        mode = MODES[name]
        plain = m.generate_from(0, prompts, N_STEPS, **mode)
        ref = None
        for top_n in TOP_NS:
            got = m.generate_from(0, prompts, N_STEPS, logprobs=top_n, **mode)
            assert np.array_equal(got[0], plain), (name, top_n, np.argwhere(got[0] != plain)[:4])
            assert np.array_equal(m.generate_from(0, prompts, N_STEPS, **mode), plain), "an ordinary generation behind one with log-probabilities"
            if ref is None:
                ref = host_reference(m, prompts, plain, mode)
            worst = max(worst, check_against(got, ref, prompts, top_n, (name, batch, graph, top_n)))
            if name == "greedy" and top_n:  # the pick is the first of the row, and reads the same bits
                picked = ~np.isnan(got[1])
                assert np.array_equal(got[2][picked][:, 0], got[0][picked])
                assert np.array_equal(got[3][picked][:, 0].view(np.uint32), got[1][picked].view(np.uint32))
    m.close()
    print(f"generate logprobs batch={batch} graph={graph}: largest |got - ref64| / bound = {worst:.3f}")


def test_top_k_one_with_penalties_lists_its_pick_first(zg, weights):
    prompts = ragged(3, 920)
    mode = dict(temp=1.0, seed=3, top_k=1, **PEN)
    m = make(weights, 3)
    plain = m.generate_from(0, prompts, N_STEPS, **mode)
    got = m.generate_from(0, prompts, N_STEPS, logprobs=5, **mode)
    ref = host_reference(m, prompts, plain, mode)
    m.close()
    assert np.array_equal(got[0], plain)
    check_against(got, ref, prompts, 5, "top_k=1")
    picked = ~np.isnan(got[1])
    assert np.array_equal(got[2][picked][:, 0], got[0][picked])
    assert np.array_equal(got[3][picked][:, 0].view(np.uint32), got[1][picked].view(np.uint32))


def test_behind_an_extend_columns_are_absolute_and_earlier_ones_stay(zg, weights):
    B, past, n = 2, 13, 60
    first = np.stack([synth.rand_tokens(930 + b, past, CFG.vocab_size) for b in range(B)])
    turns = [synth.rand_tokens(940 + b, 1 + 2 * b, CFG.vocab_size) for b in range(B)]  # 1 and 3 new tokens: through the decode loop
    mode = MODES["topk_pen"]
    m = make(weights, B)
    earlier = m.generate([first[b, :2] for b in range(B)], past + 5, logprobs=5)  # records columns 0 .. past + 4
    m.extend(0, first, compute_logits=False)
    got = m.generate_from(past, turns, n, logprobs=5, **mode)
    assert m.cached_len() == past + n
    below = m.generate_fetch_logprobs(0, past, 5)
    m.extend(0, first, compute_logits=False)
    ref = host_reference(m, turns, got[0], mode, past=past)
    m.close()
    assert same_record(below, [a[:, :past] for a in earlier[1:]]), "columns below past_len changed"
    assert not np.isnan(below[0][:, 2:]).any()
    check_against(got, ref, turns, 5, "behind an extend")


def test_prompts_through_the_whole_prompt_pass(zg, weights):
    """Prompts of 6 and 7 tokens: the device loop feeds positions 0 .. 5 in one whole-prompt pass.  The host loop fills its caches the
    same way — GPT.prefill over those positions, then GPT.forward — because exact ids need bit-identical logits, and the pass
    and the decode kernels round differently."""
    B, n = 2, 50
    prompts = [synth.rand_tokens(950 + b, 6 + b, CFG.vocab_size) for b in range(B)]
    mode = MODES["temp"]
    m = make(weights, B)
    plain = m.generate_from(0, prompts, n, **mode)
    got = m.generate_from(0, prompts, n, logprobs=20, **mode)
    m.prefill(np.stack([p[:6] for p in prompts]), compute_logits=False)
    ref = host_reference(m, prompts, plain, mode, prefilled=6)
    m.close()
    assert np.array_equal(got[0], plain)
    assert np.isnan(got[1][:, :6]).all() and np.isnan(got[1][1, 6]) and not np.isnan(got[1][0, 6])
    check_against(got, ref, prompts, 20, "whole-prompt pass")


def test_graphs_at_create_lazily_or_not_at_all(zg, weights):
    prompts = ragged(3, 960)
    records = []
    for kw in (dict(logprobs_generate=True, truncated_generate=True), dict(), dict(use_graph=False)):
        m = make(weights, 3, **kw)
        rec = [m.generate(prompts, N_STEPS, logprobs=20), m.generate_sample(prompts, N_STEPS, 0.8, seed=9, top_k=12, top_p=0.8, logprobs=20)]
        rec.append(m.generate(prompts, N_STEPS, logprobs=20))
        m.close()
        assert same_record(rec[0], rec[2])
        records.append(rec)
    for other in records[1:]:
        assert same_record(records[0][0], other[0]) and same_record(records[0][1], other[1])


def test_fetch_and_argument_errors(zg, weights):
    prompts = ragged(2, 970)
    m = make(weights, 2)
    mat, lens, stride = m._prompts(prompts)
    lp = np.zeros((2, CFG.context_size), np.float32)
    ids = np.zeros((2, CFG.context_size, 20), np.uint64)
    top = np.zeros((2, CFG.context_size, 20), np.float32)

    def fetch(first, n, top_n):
        return zg.zg_gpt_generate_fetch_logprobs(m.h, first, n, top_n, _lib.ptr(lp), lp.size, _lib.ptr(ids), _lib.ptr(top), ids.size)

    def enqueue(top_n, opt=None, pen=None):
        return zg.zg_gpt_generate_logprobs_enqueue(m.h, 0, _lib.ptr(mat), stride, _lib.ptr(lens), 20, None if opt is None else C.addressof(opt),
                                                   None if pen is None else C.addressof(pen), None, 0, None, 1, top_n)

    assert fetch(0, 10, 0) == ERR_ARG                       # nothing recorded yet
    m.generate(prompts, 30, logprobs=5)
    assert m.cached_len() == 30
    assert fetch(0, 30, 5) == 0 and fetch(0, 30, 0) == 0
    assert fetch(0, 30, 6) == ERR_ARG                       # above the recorded top_n
    assert fetch(CFG.context_size - 4, 5, 5) == ERR_SHAPE   # first + n beyond the context
    assert fetch(CFG.context_size - 4, 4, 5) == 0
    assert enqueue(21) == ERR_ARG and enqueue(CFG.vocab_size + 1) == ERR_ARG
    assert enqueue(5, pen=_lib.LogitPenalties(1.3, 0.0, 0.0)) == ERR_ARG  # greedy with penalties
    assert m.cached_len() == 30 and fetch(0, 30, 5) == 0    # the refused calls touched nothing
    m.generate(prompts, 30)
    assert fetch(0, 30, 0) == ERR_ARG                       # a generation without log-probabilities since
    assert enqueue(20, opt=_lib.SampleOptions(0.8, 0, 1.0)) == 0
    assert fetch(0, 20, 20) == 0
    m.close()
