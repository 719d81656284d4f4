"""zg_gpt_hidden against its contract: "ln_f output of the last forward, [batch, n_embed] (state.x, main.zig:189)".

ln_f exists on the device only folded into lm_head, and a whole-prompt pass without logits stops its last Block behind the cache
append, so nothing a step or a pass launches writes that vector: zg_gpt_hidden computes it.  Before this module the call returned
the residual stream in front of ln_f — after a pass without logits the row of some earlier call — and the one test of it asked for
finite values.  test_hidden_is_ln_f_of_the_last_forward fails on that library in all 12 cases at its first check (forward(1)
with logits: 1e6 .. 8e6 Y against the bound of 3 Y); the fix is zg_gpt_hidden itself (api_gpt.hip) and a resume entry of the pass's
enqueue_prefill; it adds no launch, copy or graph node to a step or a pass.

After each of forward with and without logits, sample, prefill and extend with and without logits, extend behind a rollback,
generate, and a generate whose steps all lie inside its prompt pass, every row is held two ways:

* stage: against float64 ln_f of the DEVICE'S OWN residual row, within 3 Y of the float32 evaluation of the same formula
  (stage_ref.layernorm_stage(single_pass=True), the rule of test_op_stages_gpu.py::test_layernorm_stage: the call runs that
  kernel).  The residual is the last `x` tap of the same call repeated with taps (step_taps / pass_taps with logits: a repeated
  position rewrites its cache row with the same values).
* end to end: against oracle.GPT.hidden() after the same calls, under golden_io.assert_model_close (1e-3).

x must stay what it was: argmax / the logits of the next forward after zg_gpt_hidden equal those of a twin that never asked.

Measured on one MI355X (12 handles x 9 calls = 108 stage checks, bound 3 Y; the module 5 s; xl-slice 1.0 .. 1.2 s a test, the
others below 0.05 s):

| config | weights | batch | stage worst / Y | end to end worst (bound 1e-3) |
|---|---|---|---|---|
| tiny | bf16, fp32 | 1, 3 | 1.08 .. 1.53 | 5.5e-5 .. 7.3e-5 |
| tiny3 | bf16, fp32 | 1, 3 | 0.99 .. 1.32 | 8.1e-5 .. 1.6e-4 |
| xl-slice | bf16, fp32 | 1, 3 | 1.15 .. 2.29 | 2.8e-4 .. 2.9e-4 |
"""
import numpy as np
import pytest

import oracle
import stage_ref as sr
from golden_io import assert_model_close
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu


def last_x(taps, cls):
    return [t for t in taps if t["name"] == "x" and t["cls"] == cls][-1]["data"]


def oracle_hidden(cfg, w, fed):
    """hidden() of a fresh oracle after forward(i + 1, fed[i]) for every i."""
    ref = oracle.GPT(cfg, w)
    for i, t in enumerate(fed):
        ref.forward(i + 1, int(t), compute_logits=False)
    return ref.hidden()


class Checker:
    def __init__(self, cfg, w, m, name):
        self.cfg, self.w, self.m, self.name = cfg, w, m, name
        self.worst_y = self.worst_e2e = 0.0

    def check(self, what, got, resid, fed_rows):
        """got [B][E] from zg_gpt_hidden; resid [B][E] the device's residual rows; fed_rows[b]: every token row b was fed, in order."""
        g, b = self.w["ln_f_g"], self.w["ln_f_b"]
        ref, s, y32 = sr.layernorm_stage(resid, g, b, single_pass=True)
        Y, worst = sr.metric(y32, ref, s), sr.metric(got, ref, s)
        print(f"STAGE hidden {self.name} {what} | LN registers | launches 1 | Y {Y:.3e} worst {worst:.3e} = {worst / Y:.2f} Y, bound 3 Y")
        assert worst <= 3.0 * Y, (self.name, what, worst, Y)
        self.worst_y = max(self.worst_y, worst / Y)
        for r, fed in enumerate(fed_rows):
            self.worst_e2e = max(self.worst_e2e, assert_model_close(oracle_hidden(self.cfg, self.w, fed), got[r], f"{self.name} {what} row {r}"))


@pytest.mark.parametrize("weights_f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", ["tiny", "tiny3", "xl-slice"])
def test_hidden_is_ln_f_of_the_last_forward(zg, name, batch, weights_f32):
    cfg = synth.CONFIGS[name]
    E, L, B = cfg.n_embed, cfg.n_layer, batch
    w = synth.make_weights(cfg, seed=17, bf16=not weights_f32)
    m = zgpt.GPT(cfg, batch=B, weights_f32=weights_f32)
    m.load_weights(w)
    ck = Checker(cfg, w, m, f"{name} b{B} {'fp32' if weights_f32 else 'bf16'}")
    toks = np.stack([synth.rand_tokens(50 + b, 14, cfg.vocab_size) for b in range(B)])
    rows = lambda n: [list(toks[b, :n]) for b in range(B)]
    step_resid = lambda T, t: last_x(m.step_taps(T, t)[0], 5).reshape(B, E)

    def pass_resid(past, n):
        taps, _, _ = m.pass_taps(toks[:, past: past + n], past_len=past, compute_logits=True)
        return last_x(taps, 6).reshape(B, n, E)[:, n - 1]

    # ---- decode steps: with logits, without, and the per-token sampler
    m.forward(1, toks[:, 0])
    ck.check("forward(1) with logits", m.hidden(), step_resid(1, toks[:, 0]), rows(1))
    m.forward(2, toks[:, 1], compute_logits=False)
    ck.check("forward(2) without logits", m.hidden(), step_resid(2, toks[:, 1]), rows(2))
    m.sample(3, toks[:, 2], 0.8, seed=3)
    ck.check("sample(3)", m.hidden(), step_resid(3, toks[:, 2]), rows(3))
    # ---- whole-prompt passes (7 rows: above the 4 from which generate takes the pass; not a multiple of anything)
    m.prefill(toks[:, :7])
    ck.check("prefill(7) with logits", m.hidden(), pass_resid(0, 7), rows(7))
    m.forward(1, toks[:, 3])  # x now holds another row: a pass without logits must not return it
    m.prefill(toks[:, :7], compute_logits=False)
    h = m.hidden()
    assert np.array_equal(h, m.hidden()), "a second call (the Block is finished by now) returns the same bits"
    ck.check("prefill(7) without logits", h, pass_resid(0, 7), rows(7))
    m.extend(7, toks[:, 7:12])
    ck.check("extend(7, 5) with logits", m.hidden(), pass_resid(7, 5), rows(12))
    m.extend(7, toks[:, 7:10], compute_logits=False)  # a rollback to 7, then three rows
    ck.check("extend(7, 3) without logits", m.hidden(), pass_resid(7, 3), rows(10))
    # ---- generate: the last step fed the pick before the last at position n
    prompts = [toks[b, :5] for b in range(B)]
    ids = m.generate(prompts, 11)
    h = m.hidden()
    ck.check("generate(5 + 6)", h, step_resid(11, ids[:, 9]), [list(ids[b, :5]) + list(ids[b, 4:10]) for b in range(B)])
    # ---- ... and one that ends inside its prompt pass: no step follows the pass, whose last Block stopped early
    m.forward(1, toks[:, 3])
    ids = m.generate(prompts, 5)
    assert np.array_equal(ids, toks[:, :5])
    ck.check("generate(5 of 5)", m.hidden(), pass_resid(0, 5), rows(5))
    print(f"HIDDEN {ck.name}: stage worst {ck.worst_y:.2f} Y, end to end worst {ck.worst_e2e:.2e}")
    m.close()


@pytest.mark.parametrize("name,batch", [("tiny", 1), ("tiny3", 3)])
def test_hidden_leaves_the_residual_stream_alone(zg, name, batch):
    """zg_gpt_hidden between a forward and what reads its state next — argmax, the next forward, a continuation behind a pass without
    logits (whose last Block the call finishes) — changes none of it: bit-equal with a twin handle that never asked."""
    cfg = synth.CONFIGS[name]
    w = synth.make_weights(cfg, seed=23, bf16=True)
    toks = np.stack([synth.rand_tokens(70 + b, 9, cfg.vocab_size) for b in range(batch)])
    out = []
    for ask in (False, True):
        m = zgpt.GPT(cfg, batch=batch)
        m.load_weights(w)
        rec = [m.forward(1, toks[:, 0])]
        if ask:
            m.hidden()
        rec += [m.argmax(), m.forward(2, toks[:, 1])]
        m.prefill(toks[:, :6], compute_logits=False)
        if ask:
            m.hidden()
        rec += [m.forward(7, toks[:, 6]), m.extend(7, toks[:, 7:9])]
        if ask:
            m.hidden()
        rec.append(m.generate_from(9, [toks[b, :1] for b in range(batch)], 4))
        out.append(rec)
        m.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
