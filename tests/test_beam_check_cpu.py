"""Every refusal of zg_gpt_generate_beam_enqueue (include/zgpt2.h zg_beam_options), through zg_debug_beam_check: the
option checks alone, which need neither a GPU nor zg_init."""
import ctypes as C

import numpy as np

from zig_gpt2_amd import _lib

OK, ERR_SHAPE, ERR_ARG = 0, -2, -6
VOCAB, CTX = 257, 96


def prompts_of(batch, W, n_p=3):
    mat = np.zeros((batch, n_p), np.uint64)
    for b in range(batch):
        mat[b] = 10 + (b // W) + np.arange(n_p)  # equal within a group, different between groups
    return mat, np.full(batch, n_p, np.uint64)


def check(batch=8, W=4, mat=None, lens=None, n_steps=40, past_len=0, cached_len=0, vocab=VOCAB, opt=None, req_fields=None, req_size=None, no_req=False,
          no_opt=False):
    lib = _lib.load()
    if mat is None:
        mat, lens = prompts_of(batch, W)
    fields = dict(past_len=past_len, prompts=_lib.ptr(mat), prompt_stride=mat.shape[1], prompt_lens=_lib.ptr(lens), n_steps=n_steps)
    fields.update(req_fields or {})
    req = _lib.generate_request(**fields)
    if req_size is not None:
        req.size = req_size
    o = opt if opt is not None else _lib.beam_options(W)
    return lib.zg_debug_beam_check(None if no_req else C.addressof(req), None if no_opt else C.addressof(o), batch, vocab, CTX, cached_len)


def test_good_calls_pass():
    for W, batch in [(1, 1), (2, 2), (3, 3), (4, 8), (8, 8), (1, 8)]:
        assert check(batch, W) == OK, (W, batch)
    assert check(8, 4, opt=_lib.beam_options(4, eos_token_id=VOCAB - 1, length_penalty=0.0, early_stopping=False, lookahead=3)) == OK
    assert check(8, 4, past_len=5, cached_len=9) == OK


def test_sizes_and_null_arguments():
    assert check(no_req=True) == ERR_ARG
    assert check(no_opt=True) == ERR_ARG
    assert check(req_size=8) == ERR_ARG
    o = _lib.beam_options(4)
    o.size -= 8
    assert check(opt=o) == ERR_ARG
    mat, lens = prompts_of(8, 4)
    assert check(mat=mat, lens=lens, req_fields=dict(prompts=None)) == ERR_ARG
    assert check(mat=mat, lens=lens, req_fields=dict(prompt_lens=None)) == ERR_ARG


def test_the_request_carries_nothing_but_the_prompts():
    opts = _lib.SampleOptions(1.0, 0, 1.0)
    pen = _lib.LogitPenalties(1.2, 0.0, 0.0)
    stop, keep = _lib.stop_conditions(stop_token_ids=[5])
    edits, keep2 = _lib.logit_edits(banned_token_ids=[3])
    prior = np.zeros((8, 2), np.uint64)
    for extra in (dict(options=C.addressof(opts)), dict(penalties=C.addressof(pen)), dict(prior=_lib.ptr(prior)), dict(logprobs=1), dict(top_n=4),
                  dict(stop=C.addressof(stop)), dict(edits=C.addressof(edits))):
        assert check(req_fields=extra) == ERR_ARG, extra


def test_num_beams_batch_and_vocabulary():
    for W in (0, 9, 100):
        assert check(8, 4, opt=_lib.beam_options(W)) == ERR_ARG, W
    assert check(8, 3, *prompts_of(8, 1)) == ERR_ARG        # 8 % 3 != 0
    assert check(3, 2, *prompts_of(3, 1)) == ERR_ARG
    assert check(8, 8, vocab=15) == ERR_ARG                 # 2 W > vocab
    assert check(8, 8, vocab=16) == OK


def test_length_penalty_and_eos():
    for lp in (float("nan"), float("inf"), float("-inf")):
        assert check(opt=_lib.beam_options(4, length_penalty=lp)) == ERR_ARG, lp
    assert check(opt=_lib.beam_options(4, eos_token_id=VOCAB)) == ERR_SHAPE
    assert check(opt=_lib.beam_options(4, eos_token_id=1 << 40)) == ERR_SHAPE
    assert check(opt=_lib.beam_options(4, eos_token_id=None)) == OK


def test_prompts_of_a_beam_call():
    mat, lens = prompts_of(8, 4)
    lens2 = lens.copy()
    lens2[5] = 2
    assert check(mat=mat, lens=lens2) == ERR_ARG             # unequal lengths
    mat2 = mat.copy()
    mat2[6, 1] += 1
    assert check(mat=mat2, lens=lens) == ERR_ARG             # unequal within group 1
    mat3 = mat.copy()
    mat3[4:] += 7
    assert check(mat=mat3, lens=lens) == OK                  # groups may differ from each other
    assert check(mat=mat, lens=lens, n_steps=3) == ERR_ARG   # nothing would be picked
    assert check(mat=mat, lens=lens, n_steps=4) == OK
    assert check(mat=mat, lens=lens, past_len=4, cached_len=3) == ERR_ARG
    assert check(mat=mat, lens=np.full(8, 4, np.uint64)) == ERR_SHAPE  # longer than the rows they lie in
