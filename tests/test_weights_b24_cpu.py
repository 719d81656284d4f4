"""ZG_GPT_WEIGHTS_B24 on the host side: synth.round_b24 (the numpy mirror of the device's b24_round, zg_common.h), the loader
policy weights_io.flags_for_checkpoint(..., allow_b24=True), and the flag's value in include/zgpt2.h against _lib."""
import os
import re

import numpy as np

from zig_gpt2_amd import _lib, synth, weights_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.finfo(np.float32).max


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def f32(u):
    return np.asarray(u, np.uint32).view(np.float32)


def b24_round_int(u):
    """b24_round (zg_common.h) on one fp32 bit pattern in Python integers, returned as the fp32 bit pattern it stands for."""
    r = ((u + 0x7F + ((u >> 8) & 1)) & 0xFFFFFFFF) >> 8
    if (r & 0x7F8000) == 0x7F8000 and (u & 0x7F800000) != 0x7F800000:
        r -= 1
    return (r << 8) & 0xFFFFFFFF


def test_round_b24_matches_the_integer_definition():
    rng = np.random.default_rng(3)
    u = rng.integers(0, 2**32, size=20000, dtype=np.uint64).astype(np.uint32)
    u = u[(u & 0x7F800000) != 0x7F800000]  # finite patterns (inf / NaN below)
    got = bits(synth.round_b24(f32(u)))
    want = np.array([b24_round_int(int(x)) for x in u], np.uint32)
    assert np.array_equal(got, want)


def test_round_b24_ties_to_even():
    one = 0x3F800000
    # 16 significant bits kept: the last kept bit is bit 8.  Exactly half an ulp (bit 7) rounds to the even neighbour.
    assert bits(synth.round_b24(f32(one | 0x80))) == one                      # 1 + half ulp -> 1 (even)
    assert bits(synth.round_b24(f32(one | 0x180))) == one + 0x200             # 1 + 1.5 ulp -> 1 + 2 ulp (even)
    assert bits(synth.round_b24(f32(one | 0x81))) == one + 0x100              # just above half: up
    assert bits(synth.round_b24(f32(one | 0x7F))) == one                      # just below half: down
    assert bits(synth.round_b24(f32(0x80000000 | one | 0x80))) == 0x80000000 | one  # sign-symmetric
    x = np.float32(1.0) + np.float32(3 * 2.0**-17)
    assert synth.round_b24(x) == np.float32(1.0) + np.float32(2.0**-15)


def test_round_b24_never_rounds_a_finite_value_to_inf():
    near = f32(np.array([0x7F7FFFFF, 0x7F7FFF80, 0x7F7FFF7F, 0xFF7FFFFF, 0xFF7FFF80], np.uint32))
    r = synth.round_b24(near)
    assert np.isfinite(r).all(), r
    assert r[0] == f32(0x7F7FFF00) and r[3] == -f32(0x7F7FFF00)
    assert synth.round_b24(np.float32(FLT_MAX)) <= FLT_MAX
    special = np.array([np.inf, -np.inf, np.nan, -np.nan, f32(0x7FC00001), f32(0x7F800100)], np.float32)
    r = synth.round_b24(special)
    assert r[0] == np.inf and r[1] == -np.inf
    assert np.isnan(r[2:]).all(), r
    assert np.signbit(r[1]) and not np.signbit(r[0])


def test_round_b24_is_idempotent_and_keeps_bf16_values():
    w = synth.make_weights(synth.CONFIGS["tiny"], seed=9, bf16=False)["h0.c_fc_w"]
    once = synth.round_b24(w)
    assert once.shape == w.shape and once.dtype == np.float32
    assert np.array_equal(bits(synth.round_b24(once)), bits(once))
    assert not np.array_equal(bits(once), bits(w))                      # the source really had more bits
    assert not np.any(bits(once) & 0xFF)                                # 24 bits kept
    rel = np.abs(once - w) / np.maximum(np.abs(w), np.float32(1e-30))
    assert float(rel.max()) <= 2.0**-16                                 # half an ulp of 16 significant bits
    b = synth.round_bf16(w)
    assert np.array_equal(bits(synth.round_b24(b)), bits(b))            # bf16 values are b24 values


def test_flags_for_checkpoint_with_b24():
    cfg = synth.CONFIGS["tiny"]
    rounded = synth.make_weights(cfg, seed=1, bf16=True)
    raw = synth.make_weights(cfg, seed=1, bf16=False)
    assert weights_io.flags_for_checkpoint(rounded, allow_b24=True) == {"weights_f32": False, "weights_b24": False}
    assert weights_io.flags_for_checkpoint(raw, allow_b24=True) == {"weights_f32": False, "weights_b24": True}
    # the default policy is unchanged
    assert weights_io.flags_for_checkpoint(raw) == {"weights_f32": True}
    assert weights_io.flags_for_checkpoint(rounded) == {"weights_f32": False}


def test_header_flag_matches_the_binding():
    with open(os.path.join(ROOT, "include", "zgpt2.h")) as f:
        text = f.read()
    m = re.search(r"ZG_GPT_WEIGHTS_B24\s*=\s*1\s*<<\s*(\d+)", text)
    assert m, "ZG_GPT_WEIGHTS_B24 missing from include/zgpt2.h"
    assert (1 << int(m.group(1))) == _lib.GPT_WEIGHTS_B24 == 256
    used = [int(v) for v in re.findall(r"ZG_GPT_\w+\s*=\s*1\s*<<\s*(\d+)", text)]
    assert len(used) == len(set(used)), "two creation flags share a bit"
