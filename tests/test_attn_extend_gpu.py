"""The causal prompt attention of a continuation alone (zg_debug_attn_prefill_at): the n new rows of every sequence, positions
past .. past + n - 1, against `past` cached positions plus themselves.  Reference: a float64 softmax(q k^T / 8) v per head with
the rectangular causal mask (query t sees keys 0 .. past + t), metric and bound of tests/test_attn_prefill_gpu.py.

The kernel reads EVERY key, cached and new, from the head-major caches in their storage format (fp32, fp16, B24) and expands it
exactly into bf16 planes, so the reference is built from the stored (rounded) values and the fp32 bound 2e-6 holds for all three
formats.  It never reads the k / v columns of the qkv rows: they are NaN here, and so is every cache row behind the last valid key."""
import numpy as np
import pytest
import torch

from zig_gpt2_amd import _lib, synth

pytestmark = pytest.mark.gpu

FORMATS = {"f32": 0, "f16": 1, "b24": 2}


def b24_bits(x):
    """zg_common.h b24_round: fp32 rounded (nearest even) to 16 mantissa bits, the 24 bits right-aligned."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7F + ((b >> 8) & 1)) >> 8).astype(np.uint32)


def stored(x, fmt):
    """What a cache of format fmt holds for the fp32 values x, as fp32."""
    if fmt == "f16":
        return x.astype(np.float16).astype(np.float32)
    if fmt == "b24":
        return (b24_bits(x) << 8).view(np.float32)
    return x


def cache_image(rows, fmt, ctx):
    """Device image of one head-major cache [B][H][ctx][64] holding rows [B][T][H][64] at positions 0 .. T - 1, NaN behind them."""
    B, T, H, _ = rows.shape
    r = rows.transpose(0, 2, 1, 3)
    if fmt == "b24":
        bits = b24_bits(r).reshape(B, H, T, 64)
        hi = np.full((B, H, ctx, 64), 0x7FC0, np.uint16)  # a NaN: exponent all ones, mantissa != 0
        lo = np.zeros((B, H, ctx, 64), np.uint8)
        hi[:, :, :T] = (bits >> 8).astype(np.uint16)
        lo[:, :, :T] = (bits & 0xFF).astype(np.uint8)
        return np.concatenate([hi.view(np.uint8).ravel(), lo.ravel()])
    full = np.full((B, H, ctx, 64), np.nan, np.float16 if fmt == "f16" else np.float32)
    full[:, :, :T] = r
    return full


def ref_attention(q, k, v, past):
    """q [B][n][H][64], k / v [B][past + n][H][64] -> [B n][H 64]"""
    B, n, H, _ = q.shape
    T = k.shape[1]
    s = np.einsum("bqhd,bkhd->bhqk", q.astype(np.float64), k.astype(np.float64)) / 8.0
    mask = np.arange(T)[None, :] <= past + np.arange(n)[:, None]
    s = np.where(mask[None, None], s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bhqk,bkhd->bqhd", p, v.astype(np.float64)).reshape(B * n, H * 64)


def planes_to_f64(bits, n):
    f = (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return f[:, :n] + f[:, n:2 * n] + f[:, 2 * n:]


# (B, past, n, H, key_tiles, spike): one boundary each — a single row behind a single key; one row behind a short past; two rows
# across the first tile edge; a tile-aligned past; an unaligned one with forced one-tile ranges; a rectangle that ends exactly on a
# tile; two query groups with split ranges and a merge; a batch whose first group has a padded wave; a long past cut into ranges of
# five tiles; a dominant key inside the past (the deferred rescale must fire); 33 rows behind an empty past, across one tile edge (the
# launcher's choice at past 0: the whole-prompt kernel on an fp32 cache, the continuation kernels at 0 on an fp16 / B24 one)
CASES = [(1, 0, 33, 2, 0, False),
         (1, 1, 1, 2, 0, False), (2, 5, 1, 2, 0, False), (1, 31, 2, 2, 0, False), (1, 32, 32, 3, 0, False), (2, 33, 31, 2, 1, False),
         (1, 7, 25, 2, 0, False), (1, 100, 130, 2, 2, False), (3, 130, 126, 2, 0, False), (1, 900, 123, 2, 5, False),
         (1, 150, 107, 2, 3, True)]


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("B,past,n,H,tiles,spike", CASES)
def test_attn_extend_matches_float64(zg, B, past, n, H, tiles, spike, fmt):
    E, T = 64 * H, past + n
    ctx = ((T + 63) // 64) * 64 + 64
    x = synth.fill_normal(31 + past + n, B * T * 3 * E, 0, 1.0).reshape(B, T, 3, H, 64)
    q, k, v = x[:, past:, 0].copy(), x[:, :, 1].copy(), x[:, :, 2].copy()
    if spike:  # one cached key far above the rest for every new query
        k[:, past // 2] *= 9.0
        q += 3.0 * np.sign(k[:, past // 2])[:, None]
    k, v = stored(k, fmt), stored(v, fmt)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    qkv = np.full((B * n, 3 * E), np.nan, np.float32)  # the k / v columns must not be read
    qkv[:, :E] = q.reshape(B * n, E)
    qkv_d, kc, vc = dev(qkv), dev(cache_image(k, fmt, ctx)), dev(cache_image(v, fmt, ctx))
    out_d = torch.zeros((B * n, 3 * E), dtype=torch.int16, device="cuda")
    ws = torch.zeros(B * H * n * 40 * 66 + 16, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # (the fills above run on torch's stream, the library launches on its own)
    _lib.check(zg.zg_debug_attn_prefill_at(qkv_d.data_ptr(), out_d.data_ptr(), B, past, n, E, H, kc.data_ptr(), vc.data_ptr(), FORMATS[fmt], ctx,
                                           ws.data_ptr(), ws.numel(), tiles))
    torch.cuda.synchronize()
    got = planes_to_f64(out_d.cpu().numpy().view(np.uint16), E)
    ref = ref_attention(q, k, v, past)
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} non-finite outputs"
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"attention at past {past}, {n} rows, {fmt} cache: {err:.2e}")
    assert err < 2e-6, err


def test_attn_extend_argument_checks(zg):
    d = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p = d.data_ptr()
    for bad in [dict(ctx=3), dict(kv_mode=3), dict(n=0), dict(E=96)]:
        a = dict(past=2, n=2, E=128, kv_mode=0, ctx=64)
        a.update(bad)
        r = zg.zg_debug_attn_prefill_at(p, p, 1, a["past"], a["n"], a["E"], 2, p, p, a["kv_mode"], a["ctx"], None, 0, 0)
        assert r != 0, bad
