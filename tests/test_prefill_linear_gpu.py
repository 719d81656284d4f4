"""One whole-prompt Linear at a time (zg_debug_prefill_linear: Linear.forward of src/ops.zig:21-46 for M = batch x prompt rows, as
zg_gpt_prefill launches it) on both GEMM families — the persistent four-wave kernel of gemm_s4.hip with the three activation
planes in one K loop (K slices + partial slabs for the residual adds, GELU + three-plane split), and the 128-row kernels of
prefill.hip — against a float64 product of the same operands.  The operands are exact (fp32 rows as three bf16 planes, bf16
weights), so the only error is fp32 accumulation order: the reference tolerance of src/tests.zig:4-20 applies.  Beside it every
launch is held to the stage metric of test_pass_stages_gpu.py: |got - ref64| / s within stage_ref.bound_y(route) x Y, Y the
blocked float32 sum's own error (the reference tolerance, 6e-4 relative, is fifty times a lost activation plane).  Also here: what
a model-level pass cannot reach within that test's sizes — the 128 x 256 tiles (ns = 2: 256 tiles and more) and, alone, the
plain fp32 store of the score stage's lm_head (epilogue 0: the planner gives it to the 128-row kernels under either force, the
persistent kernel has no such epilogue)."""
import ctypes

import numpy as np
import pytest
import torch

import stage_ref as sr
from golden_io import assert_ref_close
from pass_stage_cases import pass_route
from test_prefill_plan_cpu import FIELDS
from zig_gpt2_amd import _lib, synth

pytestmark = pytest.mark.gpu


def bf16_round(x):
    return (synth.to_bf16_bits(x).astype(np.uint32) << 16).view(np.float32)


def split3(x):
    """fp32 [M, K] -> bf16 bits [M, 3K] = hi | mid | lo with hi + mid + lo == x exactly."""
    hi = bf16_round(x)
    r = (x - hi).astype(np.float32)
    mid = bf16_round(r)
    lo = bf16_round((r - mid).astype(np.float32))
    assert np.array_equal((hi.astype(np.float64) + mid + lo).astype(np.float32), x)
    return np.concatenate([synth.to_bf16_bits(hi), synth.to_bf16_bits(mid), synth.to_bf16_bits(lo)], axis=1)


def planes_to_f64(bits, n):
    f = (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return f[:, :n] + f[:, n:2 * n] + f[:, 2 * n:]


def gelu64(x):
    return 0.5 * x * (1.0 + np.tanh(x * 0.7978845608 * (1.0 + 0.044715 * x * x)))


def planned(zg, M, N, K, epilogue, ws_floats, kernel, slices):
    plan = (ctypes.c_int * 21)()
    _lib.check(zg.zg_debug_prefill_plan(M, N, K, 0 if epilogue == 2 else N, epilogue, 3, ws_floats, 1, 0, 0, kernel, slices if epilogue == 1 else 0, plan, 21))
    return dict(zip(FIELDS, plan))


def assert_stage_metric(what, got, x, w, bias, plan, resid=None, act=None):
    """The stage metric with the operands as given: printed, then asserted."""
    ref, s, Y = sr.pass_linear_stage(x, w, bias, resid=resid, act=act, n_seq=x.shape[0])
    worst, route = sr.metric(got, ref, s), pass_route(plan)
    print(f"STAGE {what} | {route} | Y {Y:.3e} worst {worst:.3e} = {worst / Y:.2f} Y, bound {sr.bound_y(route):.0f} Y")
    assert worst <= sr.bound_y(route) * Y, (what, route, worst, Y)


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("M,N,K,epilogue,slices,wgs", [
    (600, 768, 256, 1, 1, None), (600, 768, 256, 1, 2, None), (600, 768, 768, 1, 4, None), (300, 320, 768, 1, 3, 2),
    (1030, 384, 1536, 1, 2, 3), (600, 768, 256, 2, 0, None), (520, 1600, 320, 2, 0, 3), (257, 192, 128, 2, 0, None)])
def test_prefill_linear_matches_float64(zg, monkeypatch, kernel, M, N, K, epilogue, slices, wgs):
    if kernel == 2 and slices > 1:
        pytest.skip("K slices are the four-wave kernel's")
    if wgs:
        monkeypatch.setenv("ZGPT2_GEMM_WGS", str(wgs))
    x = synth.fill_normal(11, M * K, 0, 1.0).reshape(M, K)
    w = bf16_round(synth.fill_normal(12, N * K, 0, 0.05).reshape(N, K))
    bias = synth.fill_normal(13, N, 0, 0.1)
    c0 = synth.fill_normal(14, M * N, 0, 1.0).reshape(M, N)
    ref = x.astype(np.float64) @ w.astype(np.float64).T + bias
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a_d, w_d, b_d = dev(split3(x).view(np.int16)), dev(synth.to_bf16_bits(w).view(np.int16)), dev(bias)
    ws = torch.zeros(max(slices, 4) * M * N, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # (the fills above run on torch's stream, the library launches on its own)
    before = zg.zg_debug_gemm_launches()
    if epilogue == 1:
        c_d = dev(c0)
        _lib.check(zg.zg_debug_prefill_linear(a_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), c_d.data_ptr(), M, N, K, 1, kernel, slices, ws.data_ptr(), ws.numel()))
        torch.cuda.synchronize()
        assert_ref_close(ref + c0, c_d.cpu().numpy(), f"resid {M}x{N}x{K} kernel {kernel} slices {slices}", scale_floor=2e-6)
        assert_stage_metric(f"resid {M}x{N}x{K} kernel {kernel} slices {slices}", c_d.cpu().numpy(), x, w, bias, planned(zg, M, N, K, 1, ws.numel(), kernel, slices), resid=c0)
    else:
        c_d = torch.zeros((M, 3 * N), dtype=torch.int16, device="cuda")
        _lib.check(zg.zg_debug_prefill_linear(a_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), c_d.data_ptr(), M, N, K, 2, kernel, 0, ws.data_ptr(), ws.numel()))
        torch.cuda.synchronize()
        got = planes_to_f64(c_d.cpu().numpy().view(np.uint16), N)
        assert_ref_close(gelu64(ref), got, f"gelu-split {M}x{N}x{K} kernel {kernel}", scale_floor=2e-6)
        assert_stage_metric(f"gelu-split {M}x{N}x{K} kernel {kernel}", got, x, w, bias, planned(zg, M, N, K, 2, ws.numel(), kernel, 0), act="gelu")
    took_s4 = zg.zg_debug_gemm_launches() - before
    assert took_s4 == (1 if kernel == 1 else 0), "the forced GEMM family did not run"
    # ... and it is the family the planner reports for the same Linear and force (family 1 = the persistent four-wave GEMM)
    plan = (ctypes.c_int * 21)()
    _lib.check(zg.zg_debug_prefill_plan(M, N, K, N if epilogue == 1 else 0, epilogue, 3, ws.numel(), 1, 0, 0, kernel, slices if epilogue == 1 else 0, plan, 21))
    assert (plan[0], plan[1] == 1) == (0, took_s4 == 1), list(plan)


@pytest.mark.parametrize("epilogue", [1, 2])
def test_prefill_linear_on_the_wide_tiles(zg, epilogue):
    """8192 x 2048 x 128 on the 128-row kernel: 64 x 8 = 512 tiles of 128 x 256 (ns = 2), which no model-level case reaches."""
    M, N, K = 8192, 2048, 128
    x = synth.fill_normal(31, M * K, 0, 1.0).reshape(M, K)
    w = bf16_round(synth.fill_normal(32, N * K, 0, 0.05).reshape(N, K))
    bias = synth.fill_normal(33, N, 0, 0.1)
    c0 = synth.fill_normal(34, M * N, 0, 1.0).reshape(M, N)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a_d, w_d, b_d = dev(split3(x).view(np.int16)), dev(synth.to_bf16_bits(w).view(np.int16)), dev(bias)
    ws = torch.zeros(M * N, dtype=torch.float32, device="cuda")
    plan = planned(zg, M, N, K, epilogue, ws.numel(), 2, 0)
    assert (plan["status"], plan["family"], plan["ns"], plan["partial"], plan["grid_x"]) == (0, 2, 2, 0, 512), plan
    c_d = dev(c0) if epilogue == 1 else torch.zeros((M, 3 * N), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    _lib.check(zg.zg_debug_prefill_linear(a_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), c_d.data_ptr(), M, N, K, epilogue, 2, 0, ws.data_ptr(), ws.numel()))
    torch.cuda.synchronize()
    got = c_d.cpu().numpy() if epilogue == 1 else planes_to_f64(c_d.cpu().numpy().view(np.uint16), N)
    ref = x.astype(np.float64) @ w.astype(np.float64).T + bias
    assert_ref_close(ref + c0 if epilogue == 1 else gelu64(ref), got, f"wide tiles, epilogue {epilogue}", scale_floor=2e-6)
    assert_stage_metric(f"wide tiles {M}x{N}x{K} epilogue {epilogue}", got, x, w, bias, plan, resid=c0 if epilogue == 1 else None, act=None if epilogue == 1 else "gelu")


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("M,N,K", [(256, 320, 384), (13, 64, 128), (260, 384, 768)])
def test_prefill_linear_plain_store(zg, kernel, M, N, K):
    """Epilogue 0, the score stage's lm_head: an fp32 store into rows that must hold nothing else afterwards (no residual add)."""
    x = synth.fill_normal(41, M * K, 0, 1.0).reshape(M, K)
    w = bf16_round(synth.fill_normal(42, N * K, 0, 0.05).reshape(N, K))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a_d, w_d = dev(split3(x).view(np.int16)), dev(synth.to_bf16_bits(w).view(np.int16))
    c_d = dev(synth.fill_normal(43, M * N, 0, 100.0).reshape(M, N))
    ws = torch.zeros(4 * M * N, dtype=torch.float32, device="cuda")
    plan = planned(zg, M, N, K, 0, ws.numel(), kernel, 0)
    assert (plan["status"], plan["family"]) == (0, 2), plan  # (under either force: the persistent kernel has no plain store)
    torch.cuda.synchronize()
    before = zg.zg_debug_gemm_launches()
    _lib.check(zg.zg_debug_prefill_linear(a_d.data_ptr(), w_d.data_ptr(), None, c_d.data_ptr(), M, N, K, 0, kernel, 0, ws.data_ptr(), ws.numel()))
    torch.cuda.synchronize()
    assert zg.zg_debug_gemm_launches() == before, "the planner reported the 128-row kernel; the persistent one ran"
    got = c_d.cpu().numpy()
    assert_ref_close(x.astype(np.float64) @ w.astype(np.float64).T, got, f"plain store {M}x{N}x{K} kernel {kernel}", scale_floor=2e-6)
    assert_stage_metric(f"plain store {M}x{N}x{K} kernel {kernel}", got, x, w, None, plan)
