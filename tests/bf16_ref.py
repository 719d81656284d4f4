"""Bit-exact reference of fp32 -> bf16 (round to nearest, ties to even) in integer numpy, and the bit patterns a conversion
must be held at.  Independent of zig_gpt2_amd.synth (whose round_bf16 the tests check against it).

f32_to_bf16_bits never adds into the exponent field of a NaN: a NaN stays a NaN of its sign, with its upper payload and the
quiet bit.  Everything else is the integer form of "the nearest of the two neighbouring bf16 values, the even one at a tie":
kept = bits >> 16, rest = bits & 0xFFFF; up when rest > 0x8000 or rest == 0x8000 with an odd kept.  A carry out of the mantissa
moves into the exponent, which is what the value does too (0x7F7FFFFF, FLT_MAX, rounds to inf; the largest subnormal rounds to
the smallest normal)."""
import numpy as np


def f32_to_bf16_bits(bits):
    """uint32 fp32 bit patterns -> uint16 bf16 bit patterns."""
    b = np.ascontiguousarray(bits, dtype=np.uint32).astype(np.uint64)
    kept, rest = b >> np.uint64(16), b & np.uint64(0xFFFF)
    up = (rest > np.uint64(0x8000)) | ((rest == np.uint64(0x8000)) & ((kept & np.uint64(1)) == np.uint64(1)))
    out = kept + up.astype(np.uint64)
    nan = (b & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    out = np.where(nan, kept | np.uint64(0x0040), out)
    return out.astype(np.uint16)


def is_nan_bf16(h):
    return (np.asarray(h, dtype=np.uint16) & np.uint16(0x7FFF)) > np.uint16(0x7F80)


def is_nan_f32(bits):
    return (np.asarray(bits, dtype=np.uint32) & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def nearest_search(bits):
    """The same conversion for non-NaN inputs by a search in float64: of the bf16 value below (toward zero) and the one above
    (away from zero; the one above the largest finite bf16 counts as 2^128, which is how IEEE rounding decides an overflow), the
    nearer one, the one with the even bit pattern at a tie.  Every fp32 and bf16 value, and their differences, are exact in
    float64."""
    b = np.ascontiguousarray(bits, dtype=np.uint32)
    assert not is_nan_f32(b).any()
    lo = b & np.uint32(0xFFFF0000)  # truncation: toward zero
    hi = (lo.astype(np.uint64) + np.uint64(0x10000)).astype(np.uint32)  # the next bf16 away from zero (never wraps: exponent <= 0xFF)

    def val(u):
        u = np.asarray(u, dtype=np.uint32)
        inf = (u & np.uint32(0x7FFFFFFF)) == np.uint32(0x7F800000)
        with np.errstate(invalid="ignore"):
            v = np.where(inf, np.float32(0), u.view(np.float32)).astype(np.float64)
        sign = np.where((u >> np.uint32(31)) == 1, -1.0, 1.0)
        return np.where(inf, sign * 2.0 ** 128, v)

    x, vlo, vhi = val(b), val(lo), val(hi)
    inf_in = (b & np.uint32(0x7FFFFFFF)) == np.uint32(0x7F800000)
    dlo, dhi = np.abs(x - vlo), np.abs(vhi - x)
    lo_even = ((lo >> np.uint32(16)) & np.uint32(1)) == 0
    take_hi = (dhi < dlo) | ((dhi == dlo) & ~lo_even)
    out = np.where(take_hi & ~inf_in, hi, lo)
    return (out >> np.uint32(16)).astype(np.uint16)


# NaNs of both signs: payload in the bits bf16 keeps, in the low bits only (the ones a bare rounding increment carries into the
# exponent), all ones, and the quiet bit alone
NAN_BITS = np.array([s | p for s in (0x00000000, 0x80000000)
                     for p in (0x7FC00000, 0x7FA50000, 0x7F800001, 0x7F80FFFF, 0x7F808000, 0x7F807FFF, 0x7FFFFFFF, 0x7FFF8000, 0x7FBFFFFF)], dtype=np.uint32)


def edge_bits():
    """fp32 bit patterns (no NaN): every exponent (0 = subnormals, 255 only as inf) x both signs x both parities of the kept bit x
    the low halves 0x7FFF, 0x8000, 0x8001 (below, at and above the tie) and 0 (exact), with the upper mantissa bits clear and
    set; +-0, +-inf, the smallest and largest subnormals, FLT_MAX (rounds to inf) and the largest value that stays finite."""
    out = []
    for sign in (0, 0x80000000):
        for e in range(255):
            for upper in (0x00, 0x01, 0x3E, 0x7E, 0x7F):  # kept mantissa bits: even and odd, 0x7F + a round-up carries into the exponent
                for rest in (0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x0001):
                    out.append(sign | (e << 23) | (upper << 16) | rest)
        out += [sign | 0x00000000, sign | 0x7F800000, sign | 0x00000001, sign | 0x007FFFFF, sign | 0x7F7FFFFF, sign | 0x7F7F7FFF, sign | 0x7F7F8000]
    return np.array(out, dtype=np.uint32)
