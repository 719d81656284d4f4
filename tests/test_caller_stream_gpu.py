"""The library on a caller's stream (zg_set_stream), the mode bench.py and every tool measure in and no test entered: every other
GPU test runs the library on its own stream behind a device-wide torch.cuda.synchronize().

Ground rules: the `zg` fixture is the session's, so every test restores zg_set_stream(None) in a `finally`, keeps its torch stream
alive until then, and an autouse fixture checks after every test that a fresh handle reports the library's own stream again.
Streams are side streams (torch.cuda.Stream()): torch's DEFAULT stream has handle 0, which zg_set_stream reads as "restore the own
stream" (test_the_default_stream_is_the_null_handle).

1. Ordered with the caller's work, no host synchronisation in between (test_*_is_ordered_*).  On stream S: a chain of FRONT_REPS
   6144^3 fp32 matmuls (measured: 24 .. 28 ms; the event behind it must not have completed when the library call is issued — a
   hard assert), a copy that overwrites a NaN-poisoned device buffer with the real operand, the library call on device pointers,
   a torch op on S that consumes the output, one synchronise at the end.  Compared with float64 under the bound the project
   already has for the op: op_stage_cases' smallest device cases of the GEMV and the matrix-core Linear under assert_stage
   (3 Y / 6 Y), zg_gemm_bf16_nt (which does not drain) at test_gemm_gpu.py's smallest shape under its two bounds, LayerNorm in
   place under 3 Y, zg_f32_to_bf16 bit for bit, and `tiny` loaded from device sources: logits bit-equal to a twin loaded from
   host memory.  Each case prints a CONTROL line: whether the same sequence with the library left on its own stream gave another
   result (it read the poison).  Not asserted — two streams may share a hardware queue and serialise — it records whether the
   test had teeth on that machine.
2. A stream change on a live handle (test_stream_change_on_a_live_handle): nano-char (4 buckets) and medium-slice (2), batch 1
   and 2, graphs on and off, plain handles and handles created with the sampled, penalty, logprob, stop and guided flags (35
   tails: capture_all re-captures every one on the first call that sees a new stream).  Generate on the own stream to position
   40, switch to S and continue across the bucket boundary at 64, restore and continue.  Tokens, log-probabilities, finish
   columns and the logits of a final forward are those of a twin that never switched, bit for bit.  zg_gpt_stream reports S after
   the switch and the own stream after the restore, and never changes for a handle with a private stream.
3. Op-tier state across a switch, bit-equal with the same calls without one: the device twin of a host buffer (LayerNorm on one
   stream, Linear on the same buffer on the other), the mirrors of host KV caches (positions 1 .. 3 and 4 .. 6), a registered
   weight.
4. The prefetcher's events are re-wired to the new stream: no stall the twin does not report.

Out of scope, both caller errors whose test would be a fault on purpose: destroying a stream the library still holds, and
switching from another thread.

Measured on one MI355X (27 tests, the module 8 s including 2 s for the front work's first matmul; the slowest test 0.7 s — the
flagged nano-char handles with graphs —, an ordered case 0.05 .. 0.2 s, a plain live handle 0.13 .. 0.3 s).  No defect was found:
every case passed on the library as it was.

| ordered case | front work | worst / bound | CONTROL: library on its own stream |
|---|---|---|---|
| Linear 2x4108x37 GR_GENERIC | 27.4 ms | 1.03 Y / 3 Y | another result (it read the poison) |
| Linear 128x768x260 OP_S4 six pairs | 24.5 ms | 2.07 Y / 6 Y | another result |
| zg_gemm_bf16_nt 16x8x1600 | 24.6 ms | 3.52 Y / 6 Y | another result |
| LayerNorm 3x768 in place | 27.3 ms | 1.00 Y / 3 Y | another result |
| zg_f32_to_bf16 257 | 24.7 ms | bit-equal | another result |
| load_tensor, tiny | 26.6 ms | bit-equal | another result |

The 16 live-handle cases, the three op-tier sequences and the prefetcher (exit [1] x 8 on both handles, no stall) are bit-equal
with their twins.
"""
import ctypes as C

import numpy as np
import pytest

import bf16_ref
import op_stage_cases as oc
import oracle
import stage_ref as sr
from golden_io import assert_ref_close
from zig_gpt2_amd import _lib, ops, synth
from zig_gpt2_amd import gpt as zgpt

pytestmark = pytest.mark.gpu
FRONT_N, FRONT_REPS = 6144, 8


def stream_of(zg, m):
    p = C.c_void_p()
    _lib.check(zg.zg_gpt_stream(m.h, C.byref(p)))
    return p.value or 0


def probe_stream(zg):
    """The stream a fresh handle reports: the library stream of the moment."""
    m = zgpt.GPT(synth.CONFIGS["tiny"], use_graph=False)
    try:
        return stream_of(zg, m)
    finally:
        m.close()


@pytest.fixture(scope="module")
def own(zg):
    _lib.check(zg.zg_set_stream(None))
    return probe_stream(zg)


@pytest.fixture(autouse=True)
def restored(zg, own):
    yield
    _lib.check(zg.zg_set_stream(None))  # (a test that failed before its own restore must not leave the session on a dead stream)
    assert probe_stream(zg) == own


class Front:
    """Work that keeps a stream busy for tens of milliseconds: the launches behind it are issued long before it ends."""

    def __init__(self):
        import torch

        self.a = torch.randn(FRONT_N, FRONT_N, device="cuda") / FRONT_N ** 0.5
        self.b = torch.empty_like(self.a)
        torch.matmul(self.a, self.a, out=self.b)
        torch.cuda.synchronize()

    def queue(self):
        import torch

        for _ in range(FRONT_REPS):
            torch.matmul(self.a, self.a, out=self.b)


@pytest.fixture(scope="module")
def front(zg):
    return Front()


def ordered(zg, front, on_caller_stream, make):
    """make() -> (stage, call, consume), called once the library is on the stream it will run on: front work, stage(), call(),
    consume() on a side stream, one synchronise at the end.  on_caller_stream False: the control — the library stays on its own
    stream.  Returns (what consume returned, ms of front work)."""
    import torch

    S = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        if on_caller_stream:
            _lib.check(zg.zg_set_stream(S.cuda_stream))
        stage, call, consume = make()
        torch.cuda.synchronize()  # make() fills the poisoned buffers on torch's default stream, which nothing orders with S
        with torch.cuda.stream(S):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            front.queue()
            t1.record()
            stage()
            if on_caller_stream:
                assert not t1.query(), "the front work had ended before the library call was issued: the test proves nothing"
            call()
            out = consume()
        S.synchronize()
        _lib.check(zg.zg_synchronize())
    finally:
        _lib.check(zg.zg_set_stream(None))
    torch.cuda.synchronize()
    return out, t0.elapsed_time(t1)


def with_control(zg, front, what, make):
    """make() -> (stage, call, consume) on fresh buffers.  Runs the control (library on its own stream), then the test; prints the
    CONTROL line; returns the test's output as numpy."""
    outs = {}
    for on in (False, True):
        out, ms = ordered(zg, front, on, make)
        outs[on] = out.cpu().numpy() if hasattr(out, "cpu") else out
    differs = outs[False].tobytes() != outs[True].tobytes()
    print(f"CONTROL {what} | front work {ms:.1f} ms | library on its own stream: {'another result (it read the poison)' if differs else 'the same result'}")
    return outs[True]


def dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.array(a, copy=True, order="C")).cuda()  # (a copy: the shared references are read-only)


# ---------------------------------------------------------------------------------------------- 1. ordered with the caller's work
def smallest_device_case(mfma):
    cs = [c for c in oc.LINEAR_CASES if c.place == "device" and c.K <= oc.K_CHUNK and oc.mfma_ok(c.M, c.K, c.N) == mfma]
    return min(cs, key=lambda c: c.M * c.K * c.N)


@pytest.mark.parametrize("mfma", [False, True], ids=["gemv", "matrix-core"])
def test_linear_is_ordered_on_the_callers_stream(zg, front, monkeypatch, mfma):
    import torch

    from test_op_stages_gpu import assert_stage, last_kernel, linear_reference

    case = smallest_device_case(mfma)
    assert (case.M >= 16) == mfma
    for name in ("ZGPT2_GEMM_KERNEL", "ZGPT2_GEMM_WGS"):
        monkeypatch.delenv(name, raising=False)
    M, K, N = case.M, case.K, case.N
    x, w, b, ref, s, y32 = linear_reference(M, K, N, case.bias)
    route, kernel, gemms = oc.route_of(case)
    wd, bd, xsrc = dev(w), dev(b), dev(x)

    def make():
        xd, yd = torch.full((M, K), float("nan"), device="cuda"), torch.full((M, N), float("nan"), device="cuda")
        return (lambda: xd.copy_(xsrc)), (lambda: ops.Linear(K, N, wd, bd).forward(xd, yd)), (lambda: yd * 1.0)

    before = zg.zg_debug_gemm_launches()
    got = with_control(zg, front, f"Linear {case.id}", make)
    assert zg.zg_debug_gemm_launches() - before == 2 * gemms
    assert last_kernel(zg).startswith(kernel), (last_kernel(zg), kernel)
    assert_stage(f"Linear {case.id} on a caller's stream", route, got, ref, s, y32)


def test_gemm_bf16_nt_is_ordered_without_a_drain(zg, front):
    """zg_gemm_bf16_nt returns without draining: its output is consumed on S with no synchronise between the call and the consumer."""
    import torch

    from test_gemm_gpu import assert_stage_metric

    m, n, k = 16, 8, 1600   # the smallest shape of test_gemm_gpu.py
    a = synth.fill_normal(1000 + m, m * k, 0.0, 1.0, bf16=True).reshape(m, k)
    b = synth.fill_normal(2000 + n, n * k, 0.0, 0.05, bf16=True).reshape(n, k)
    bias = synth.fill_normal(3000 + n, n, 0.0, 0.5)
    asrc = dev(synth.to_bf16_bits(a).view(np.int16).reshape(m, k))
    bd, biasd = dev(synth.to_bf16_bits(b).view(np.int16).reshape(n, k)), dev(bias)

    def make():
        ad = torch.full((m, k), 0x7FC0, dtype=torch.int16, device="cuda")  # bf16 NaN
        cd = torch.full((m, n), float("nan"), device="cuda")
        call = lambda: _lib.check(zg.zg_gemm_bf16_nt(ad.data_ptr(), bd.data_ptr(), biasd.data_ptr(), cd.data_ptr(), m, n, k, 0, 0))
        return (lambda: ad.copy_(asrc)), call, (lambda: cd.clone())

    got = with_control(zg, front, f"zg_gemm_bf16_nt {m}x{n}x{k}", make)
    assert_ref_close(oracle.linear_forward(k, n, b, bias, a), got, "gemm on a caller's stream", scale_floor=4e-6)
    assert_stage_metric(f"gemm {m}x{n}x{k} on a caller's stream", got, a, b, bias, False)


def test_layernorm_in_place_is_ordered(zg, front):
    import torch

    from test_op_stages_gpu import assert_stage

    rows, n = 3, 768
    x, g, b = oc.layernorm_operands(rows, n)
    ref, s, y32 = sr.layernorm_stage(x, g, b, single_pass=True)
    xsrc, gd, bd = dev(x), dev(g), dev(b)

    def make():
        xd = torch.full((rows, n), float("nan"), device="cuda")
        return (lambda: xd.copy_(xsrc)), (lambda: ops.LayerNorm(n, gd, bd).forward(xd)), (lambda: xd + 0.0)

    got = with_control(zg, front, f"LayerNorm {rows}x{n} in place", make)
    assert_stage(f"LayerNorm {rows}x{n} on a caller's stream", "LN registers", got, ref, s, y32)


def test_f32_to_bf16_is_ordered(zg, front):
    import torch

    e = bf16_ref.edge_bits()
    bits = e[np.arange(257) * (e.size // 257)]
    src = dev(bits.view(np.int32))

    def make():
        sd = torch.full((257,), 0x7FC00000, dtype=torch.int32, device="cuda")  # fp32 NaN
        dd = torch.full((257,), 0x5A5A, dtype=torch.int16, device="cuda")
        return (lambda: sd.copy_(src)), (lambda: _lib.check(zg.zg_f32_to_bf16(sd.data_ptr(), dd.data_ptr(), 257))), (lambda: dd.clone())

    got = with_control(zg, front, "zg_f32_to_bf16 257", make)
    assert np.array_equal(got.view(np.uint16), bf16_ref.f32_to_bf16_bits(bits))


def test_weights_load_from_device_sources_in_stream_order(zg, front):
    """zg_gpt_load_tensor / zg_gpt_load_block_tensor from device buffers that S fills behind the front work."""
    import torch

    cfg = synth.CONFIGS["tiny"]
    w = synth.make_weights(cfg, seed=77, bf16=True)
    tok = synth.rand_tokens(78, 1, cfg.vocab_size)
    twin = zgpt.GPT(cfg)
    twin.load_weights(w)
    want = twin.forward(1, tok)
    twin.close()
    srcs = {k: dev(v) for k, v in w.items()}
    handles = []

    def make():
        bufs = {k: torch.full_like(v, float("nan")) for k, v in srcs.items()}
        m = zgpt.GPT(cfg)   # created on the stream it will load and run on: the control's on the own stream, the test's on S
        handles.append(m)
        out = {}

        def stage():
            for k in bufs:
                bufs[k].copy_(srcs[k])

        def call():
            m.load_weights(bufs)
            out["logits"] = m.forward(1, tok)
        return stage, call, (lambda: out["logits"])

    try:
        got = with_control(zg, front, "load_tensor tiny", make)
    finally:
        for m in handles:
            m.close()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------- 2. a stream change on a live handle
FLAGGED = dict(sampled_generate=True, penalized_generate=True, logprobs_generate=True, stop_generate=True, guided=True)


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or isinstance(a, (int, np.integer)):
        return a == b
    return np.array_equal(bits(a), bits(b))


def life(zg, cfg, w, batch, use_graph, flagged, switch, own):
    """Three pieces of one sequence: to position 40, across the bucket boundary at 64, and on.  switch: the middle piece runs with
    the library on a side stream.  Returns everything the pieces returned."""
    import torch

    kw = dict(FLAGGED) if flagged else {}
    m = zgpt.GPT(cfg, batch=batch, use_graph=use_graph, **kw)
    private = zgpt.GPT(cfg, batch=1, use_graph=False, own_stream=True)
    rec = []
    S = torch.cuda.Stream()
    try:
        m.load_weights(w)
        private_stream = stream_of(zg, private)
        assert private_stream not in (0, own)
        prompts = [synth.rand_tokens(300 + b, 5 + 2 * b, cfg.vocab_size) for b in range(batch)]
        n2 = 30 if cfg.context_size <= 80 else 100   # 40 .. 70 of 80, or 40 .. 140: across 64 (and 128)
        n3 = cfg.context_size - 40 - n2 if cfg.context_size <= 80 else 60
        if flagged:
            never = dict(stop=[[0, 1, 2]])   # (a stop generation whose condition does not come: the stop twins run, nothing ends early)
            opts = dict(temp=0.8, seed=5, repetition_penalty=1.2, presence_penalty=0.1, logprobs=3)
            piece = lambda past, p, n, **st: m.generate_from(past, p, n, **opts, **st) if past else m.generate_sample(p, n, **opts, **st)
        else:
            never = {}
            piece = lambda past, p, n, **st: m.generate_from(past, p, n) if past else m.generate(p, n)
        assert stream_of(zg, m) == own
        rec.append(piece(0, prompts, 40, **never))
        assert m.cached_len() == 40
        turn = [synth.rand_tokens(310 + b, 1, cfg.vocab_size) for b in range(batch)]
        if switch:
            _lib.check(zg.zg_set_stream(S.cuda_stream))
            assert stream_of(zg, m) == S.cuda_stream and S.cuda_stream not in (0, own)
            assert stream_of(zg, private) == private_stream
        rec.append(piece(40, turn, n2, **never))
        assert m.cached_len() == 40 + n2
        if switch:
            _lib.check(zg.zg_set_stream(None))
            assert stream_of(zg, m) == own and stream_of(zg, private) == private_stream
        last = dict(stop_token_ids=[3, 7, 11], stop=[[5, 9]]) if flagged else {}   # conditions that do come: real finish columns
        rec.append(piece(40 + n2, turn, n3, **last))
        if flagged:
            rec.append(m.stop_result())
        rec.append(m.forward(m.cached_len() + 1 if m.cached_len() < cfg.context_size else m.cached_len(), [1] * batch))
    finally:
        _lib.check(zg.zg_set_stream(None))
        m.close()
        private.close()
    return rec


@pytest.mark.parametrize("flagged", [False, True], ids=["plain", "flagged"])
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("name", ["nano-char", "medium-slice"])
def test_stream_change_on_a_live_handle(zg, own, name, batch, use_graph, flagged):
    cfg = synth.CONFIGS[name]
    w = synth.make_weights(cfg, seed=61, bf16=True)
    a = life(zg, cfg, w, batch, use_graph, flagged, False, own)
    b = life(zg, cfg, w, batch, use_graph, flagged, True, own)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert same(x, y), f"piece {i} differs after the stream change"


def test_the_default_stream_is_the_null_handle(zg, own):
    """torch's default stream is the legacy null stream: its handle is 0, which zg_set_stream reads as "the library's own stream".
    Work a caller queues there is therefore NOT ordered with the library (include/zgpt2.h says so)."""
    import torch

    h = torch.cuda.default_stream().cuda_stream
    assert h == 0
    try:
        _lib.check(zg.zg_set_stream(h))
        assert probe_stream(zg) == own
    finally:
        _lib.check(zg.zg_set_stream(None))


# ---------------------------------------------------------------------------------------------- 3. op-tier state across a switch
def z(*shape):
    return np.zeros(shape, np.float32)


def on_streams(zg, first, second, switch):
    """first() on the own stream, second() on a side stream (switch) or on the own stream again."""
    import torch

    S = torch.cuda.Stream()
    try:
        first()
        if switch:
            _lib.check(zg.zg_set_stream(S.cuda_stream))
        second()
    finally:
        _lib.check(zg.zg_set_stream(None))
    del S


def test_device_twin_of_a_host_buffer_across_a_switch(zg):
    """LayerNorm leaves a device twin of its host output for the Linear that reads the same buffer next (zg_runtime.h Shadow)."""
    rows, n, out_f = 3, 768, 259
    x, g, b = oc.layernorm_operands(rows, n)
    w = synth.fill_normal(100 + out_f, out_f * n, 0, 0.05).reshape(out_f, n)
    res = []
    for switch in (False, True):
        buf, y = x.copy(), z(rows, out_f)
        on_streams(zg, lambda: ops.LayerNorm(n, g, b).forward(buf), lambda: ops.Linear(n, out_f, w, None).forward(buf, y), switch)
        res.append((buf.copy(), y))
    assert same(res[0], res[1])
    assert np.abs(res[0][1]).max() > 0


def test_kv_mirrors_across_a_switch(zg):
    e, hds, T = 128, 2, 6
    caw = synth.fill_normal(70, 3 * e * e, 0, 0.08).reshape(3 * e, e)
    cab = synth.fill_normal(71, 3 * e, 0, 0.05)
    cpw = synth.fill_normal(72, e * e, 0, 0.08).reshape(e, e)
    cpb = synth.fill_normal(73, e, 0, 0.05)
    xs = synth.fill_normal(74, T * e, 0, 1.0).reshape(T, e)
    res = []
    for switch in (False, True):
        attn = ops.CausalSelfAttention(hds, e, ops.Linear(e, 3 * e, caw, cab), ops.Linear(e, e, cpw, cpb))
        k_cache, v_cache, outs = z(T * e), z(T * e), z(T, e)
        _qkv, _q, _k, _v, _attn = z(3 * e), z(e), z(T * e), z(T * e), z(T)

        def steps(ts):
            for t in ts:
                attn.forward(t, xs[t - 1], k_cache[: t * e], v_cache[: t * e], outs[t - 1], _qkv, _q, _k[: t * e], _v[: t * e], _attn[:t])
        try:
            on_streams(zg, lambda: steps((1, 2, 3)), lambda: steps((4, 5, 6)), switch)
        finally:
            _lib.check(zg.zg_unregister_tensor(k_cache.ctypes.data))
            _lib.check(zg.zg_unregister_tensor(v_cache.ctypes.data))
        res.append((outs, k_cache, v_cache))
    assert same(res[0], res[1])
    ref = oracle.CausalSelfAttention(hds, e, caw, cab, cpw, cpb, T)
    for t in range(1, T + 1):
        assert_ref_close(ref.forward(t, xs[t - 1]), res[1][0][t - 1], f"step {t}", scale_floor=2e-6)


def test_registered_weight_on_both_streams(zg):
    k, n, m = 768, 259, 3
    w = synth.fill_normal(1, n * k, 0, 0.05).reshape(n, k)
    x = synth.fill_normal(2, m * k).reshape(m, k)
    res = []
    _lib.check(zg.zg_register_tensor(w.ctypes.data, w.size))
    try:
        for switch in (False, True):
            y1, y2 = z(m, n), z(m, n)
            on_streams(zg, lambda: ops.Linear(k, n, w, None).forward(x, y1), lambda: ops.Linear(k, n, w, None).forward(x, y2), switch)
            res.append((y1, y2))
    finally:
        _lib.check(zg.zg_unregister_all())
    assert same(res[0], res[1]) and same(res[1][0], res[1][1])
    assert_ref_close(oracle.linear_forward(k, n, w, None, x), res[1][1], "registered weight on a caller's stream")


# ---------------------------------------------------------------------------------------------- 4. the prefetcher
def test_prefetcher_follows_a_stream_change(zg):
    """A batch-1 handle with the prefetcher on by default: not a 124M-shaped one but tiny3, the smallest configuration of
    test_prefetch_gpu.py — the events pf_start records and waits on are the same code at any size."""
    import torch

    cfg = synth.CONFIGS["tiny3"]   # the smallest configuration of test_prefetch_gpu.py
    w = synth.make_weights(cfg, seed=21, bf16=True)
    prompt = synth.rand_tokens(211, 5, cfg.vocab_size)
    stats, ids = {}, {}
    S = torch.cuda.Stream()
    for switch in (False, True):
        m = zgpt.GPT(cfg)
        try:
            m.load_weights(w)
            m.generate([prompt], cfg.context_size)
            if switch:
                _lib.check(zg.zg_set_stream(S.cuda_stream))
            for _ in range(2):  # the second call sees how the first one's prefetcher left
                ids[switch] = m.generate([prompt], cfg.context_size)
            stats[switch] = m.prefetch_stats()
        finally:
            _lib.check(zg.zg_set_stream(None))
            m.close()
    print(f"PREFETCH own stream {stats[False]['exit']} stalled {stats[False]['stalled']} | after the switch {stats[True]['exit']} stalled {stats[True]['stalled']}")
    assert np.array_equal(ids[False], ids[True])
    assert stats[False]["on"] and stats[True]["on"]  # (batch 1, small Linears: on by default — a policy change must not hollow this test)
    assert not stats[True]["stalled"] or stats[False]["stalled"]
    assert (2 in stats[True]["exit"]) <= (2 in stats[False]["exit"])
