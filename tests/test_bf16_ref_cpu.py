"""tests/bf16_ref.py — the fp32 -> bf16 rule the GPU tests hold zg_f32_to_bf16 and the bf16 weight upload to — checked against
a nearest-value search in float64, pinned on bit patterns written by hand, and compared with synth.round_bf16 / to_bf16_bits
(the host side of every bf16 weight the suite makes)."""
import numpy as np

import bf16_ref
from zig_gpt2_amd import synth


def test_integer_rule_equals_the_float64_search_on_every_edge():
    b = bf16_ref.edge_bits()
    assert b.size > 15000
    assert np.array_equal(bf16_ref.f32_to_bf16_bits(b), bf16_ref.nearest_search(b))


def test_integer_rule_equals_the_search_on_random_patterns():
    rng = np.random.default_rng(5)
    b = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)
    b = b[~bf16_ref.is_nan_f32(b)]
    assert np.array_equal(bf16_ref.f32_to_bf16_bits(b), bf16_ref.nearest_search(b))


def test_by_hand():
    cases = {
        0x00000000: 0x0000, 0x80000000: 0x8000, 0x7F800000: 0x7F80, 0xFF800000: 0xFF80,
        0x3F800000: 0x3F80,  # 1.0
        0x3F807FFF: 0x3F80, 0x3F808000: 0x3F80, 0x3F808001: 0x3F81,  # even kept bit: the tie goes down
        0x3F817FFF: 0x3F81, 0x3F818000: 0x3F82, 0x3F818001: 0x3F82,  # odd kept bit: the tie goes up
        0x3FFF8000: 0x4000,  # the carry crosses into the exponent
        0x7F7FFFFF: 0x7F80, 0xFF7FFFFF: 0xFF80,  # FLT_MAX rounds to inf
        0x7F7F7FFF: 0x7F7F, 0x7F7F8000: 0x7F80,
        0x00000001: 0x0000, 0x00008000: 0x0000, 0x00008001: 0x0001, 0x00018000: 0x0002,  # subnormals
        0x007FFFFF: 0x0080,  # the largest subnormal rounds to the smallest normal
        0x807FFFFF: 0x8080,
    }
    b = np.array(list(cases.keys()), dtype=np.uint32)
    assert np.array_equal(bf16_ref.f32_to_bf16_bits(b), np.array(list(cases.values()), dtype=np.uint16))


def test_a_nan_stays_a_nan_of_its_sign():
    h = bf16_ref.f32_to_bf16_bits(bf16_ref.NAN_BITS)
    assert bf16_ref.is_nan_bf16(h).all()
    assert np.array_equal(h >> 15, (bf16_ref.NAN_BITS >> 31).astype(np.uint16))
    # the three patterns a bare rounding increment turns into -0.0, +0.0 and +inf
    assert list(bf16_ref.f32_to_bf16_bits(np.array([0x7FFFFFFF, 0xFFFFFFFF, 0x7F800001], np.uint32))) == [0x7FFF, 0xFFFF, 0x7FC0]


def test_synth_rounds_as_the_reference_does():
    b = np.concatenate([bf16_ref.edge_bits(), bf16_ref.NAN_BITS])
    x = b.view(np.float32)
    assert np.array_equal(synth.to_bf16_bits(x), bf16_ref.f32_to_bf16_bits(b))
    r = synth.round_bf16(x)
    assert r.dtype == np.float32 and r.shape == x.shape
    assert np.array_equal(r.view(np.uint32), bf16_ref.f32_to_bf16_bits(b).astype(np.uint32) << 16)
