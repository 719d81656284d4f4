"""zg_f32_to_bf16 and the bf16 weight upload (zg_gpt_load_tensor on a default handle), bit for bit against tests/bf16_ref.py
(integer round to nearest even, itself checked against a float64 nearest-value search in test_bf16_ref_cpu.py).

Inputs: bf16_ref.edge_bits() — every exponent, both signs, both parities of the kept bit, the low halves 0x7FFF / 0x8000 /
0x8001 / 0xFFFF / 1 / 0, subnormals, +-0, +-inf, FLT_MAX (rounds to inf) — with bf16_ref.NAN_BITS spread through them: NaNs of
both signs whose payload lies in the kept bits, in the low bits only, and all ones.  A finite or infinite input must give exactly
the reference's bits; a NaN must stay a NaN of the same sign.

Before this module neither path was called by a test.  Both go through f32_to_bf16_kernel, the one caller of f32_to_bf16_rne
(zg_common.h), which added its rounding increment to the bit pattern of a NaN too: 0x7FFFFFFF became 0x8000 (-0.0), 0xFFFFFFFF
became 0x0000, 0x7F800001 became 0x7F80 (+inf) — 10 of the 18 NaN patterns left their class; the finite and infinite inputs were
right.  f32_to_bf16_rne now keeps a NaN's sign and upper payload and sets the quiet bit; synth.round_bf16 / to_bf16_bits do the
same.  No other kernel is touched: the GEMM and decode epilogues convert through cvt_pk_bf16 (the hardware conversion), which
kept NaNs all along.

Lengths: 1, 255, 256, 257 (one workgroup is 256 lanes) and 2048 x 256 + 257 (the grid is capped at 2048 workgroups: beyond it
the kernel strides); host sources (staged) and device sources.

Measured on one MI355X: 13 tests, all bit-equal / every NaN kept; the module 0.3 s, the slowest test (the strided length from the
host) 0.09 s.  On the tree before the fix the 12 tests against bf16_ref fail, each at its first NaN with low payload bits;
test_synth_agrees_with_the_device passed there, because synth.round_bf16 shared the kernel's arithmetic (it fails for the old
library beside the new synth).
"""
import numpy as np
import pytest

import bf16_ref
from zig_gpt2_amd import _lib, synth
from zig_gpt2_amd import gpt as zgpt

pytestmark = pytest.mark.gpu

GRID_CAP = 2048 * 256   # elementwise.hip grid_for: 2048 workgroups of 256 lanes, then a stride
LENGTHS = [1, 255, 256, 257, GRID_CAP + 257]


def inputs(n, shift=0):
    """n fp32 bit patterns: the edge list with a NaN pattern in front of every 7 of them, rotated by `shift` and repeated to length."""
    e, nan = bf16_ref.edge_bits(), bf16_ref.NAN_BITS
    pool = np.insert(e, np.arange(0, e.size, 7), np.resize(nan, (e.size + 6) // 7))
    return np.resize(np.roll(pool, -shift), n).astype(np.uint32)


def assert_converted(bits, got, what):
    bits, got = np.asarray(bits, np.uint32).ravel(), np.asarray(got, np.uint16).ravel()
    ref = bf16_ref.f32_to_bf16_bits(bits)
    nan = bf16_ref.is_nan_f32(bits)
    bad = np.nonzero(~nan & (got != ref))[0]
    assert bad.size == 0, f"{what}: {bad.size} finite / infinite inputs differ; first 0x{bits[bad[0]]:08X} -> 0x{got[bad[0]]:04X}, reference 0x{ref[bad[0]]:04X}"
    lost = np.nonzero(nan & ~(bf16_ref.is_nan_bf16(got) & ((got >> 15) == (bits >> 31))))[0]
    assert lost.size == 0, f"{what}: {lost.size} of {int(nan.sum())} NaNs left their class or sign; first 0x{bits[lost[0]]:08X} -> 0x{got[lost[0]]:04X}"
    return int(nan.sum())


class _DevMem:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def convert(zg, bits, place):
    import torch

    src = bits.view(np.float32)
    dst = torch.full((bits.size + 8,), 0x5A5A, dtype=torch.int16, device="cuda")  # (8 more: nothing behind the length may be written)
    if place == "device":
        src = torch.from_numpy(bits.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    _lib.check(zg.zg_f32_to_bf16(_lib.ptr(src), dst.data_ptr(), bits.size))
    _lib.check(zg.zg_synchronize())
    out = dst.cpu().numpy().view(np.uint16)
    assert (out[bits.size:] == 0x5A5A).all()
    return out[: bits.size]


@pytest.mark.parametrize("place", ["host", "device"])
@pytest.mark.parametrize("n", LENGTHS)
def test_f32_to_bf16_is_round_to_nearest_even(zg, n, place):
    if n == 1:  # one element per call: a NaN with low payload bits, FLT_MAX, a tie on an odd kept bit, a subnormal
        for b in (0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF, 0x7F7FFFFF, 0x3F818000, 0x00008001):
            bits = np.array([b], np.uint32)
            assert_converted(bits, convert(zg, bits, place), f"0x{b:08X} {place}")
        return
    bits = inputs(n, shift=n % 101)
    nans = assert_converted(bits, convert(zg, bits, place), f"n {n} {place}")
    assert nans >= n // 10
    if n > GRID_CAP:  # every edge pattern passes through this length at least once
        assert n >= bf16_ref.edge_bits().size + bf16_ref.NAN_BITS.size


@pytest.mark.parametrize("place", ["host", "device"])
def test_bf16_weight_upload_rounds_to_nearest_even(zg, place):
    """zg_gpt_load_tensor(ZG_WTE) on a bf16-weight `tiny` handle, read back from the weight region (wte is its first tensor)."""
    import torch

    cfg = synth.CONFIGS["tiny"]
    n = cfg.vocab_size * cfg.n_embed
    bits = inputs(n, shift=13)
    src = bits.view(np.float32) if place == "host" else torch.from_numpy(bits.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    m = zgpt.GPT(cfg)
    try:
        _lib.check(zg.zg_gpt_load_tensor(m.h, 0, _lib.ptr(src), n))
        p, nbytes = m.weight_arena()
        assert nbytes >= 2 * n
        got = torch.as_tensor(_DevMem(p, 2 * n), device="cuda").cpu().numpy().view(np.uint16)
    finally:
        m.close()
    assert assert_converted(bits, got, f"wte upload from {place}") > 0


def test_synth_agrees_with_the_device(zg):
    """The host side of every bf16 weight the suite makes (synth.to_bf16_bits) against the device, NaN payloads included."""
    bits = inputs(4099)
    got = convert(zg, bits, "device")
    assert np.array_equal(got, synth.to_bf16_bits(bits.view(np.float32)))
