"""zg_gpt_kv_fork: row b's KV caches over the cached positions become byte for byte those of row src[b]; rows that are
their own source and every position at or beyond the cached length stay as they were.  Compared through zg_debug_gpt_kv_rows, the
raw cache bytes, in all three cache formats, at batch 3 and 8, at cached lengths around the 64-position bucket bound and at the
full context.

The bytes behind the cached length are made non-trivial first: a run over the whole context fills every position of every row with
its own values, and zg_gpt_forward(len, ...) — which rewrites position len - 1 and sets the cached length to len without clearing
anything behind it — rolls the handle back.  (len 1 is the one exception: a forward at position 0 starts a new sequence and clears
the caches, so there the bytes behind are zero in every row.)"""
import numpy as np
import pytest

from zig_gpt2_amd import _lib
from zig_gpt2_amd import gpt as zgpt
from zig_gpt2_amd import synth

pytestmark = pytest.mark.gpu
CFG = synth.GPTConfig(257, 96, 2, 2, 128)
LENS = [1, 63, 64, 65, 96]
FORMATS = {"fp32": dict(), "fp16": dict(kv_f16=True), "b24": dict(kv_b24=True)}
SRC = {3: [2, 1, 2], 8: [0, 0, 5, 5, 0, 5, 6, 0]}  # rows 1 (batch 3) and 6 (batch 8) are fixed points nobody copies
ERR_SHAPE, ERR_ARG = -2, -6


@pytest.fixture(scope="module")
def weights():
    return synth.make_weights(CFG, seed=81, bf16=True)


def snapshot(m):
    """Every cache byte of the handle: [layer][K / V][row] -> uint8 [n_heads * context * 64 * element bytes] as kv_rows returns it."""
    return [[[m.kv_rows(l, w, b, 0, CFG.context_size) for b in range(m.batch)] for w in range(2)] for l in range(CFG.n_layer)]


def split(buf, eb):
    """kv_rows' bytes as (plane [H][ctx][64 * eb], byte plane [H][ctx][64] or None)."""
    H, C = CFG.n_heads, CFG.context_size
    main = buf[: H * C * 64 * (4 if eb == 4 else 2)].reshape(H, C, -1)
    lo = buf[H * C * 64 * 2:].reshape(H, C, 64) if eb == 3 else None
    return main, lo


@pytest.mark.parametrize("batch", [3, 8])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_fork_copies_the_cached_positions_and_nothing_else(zg, weights, fmt, batch):
    m = zgpt.GPT(CFG, batch=batch, **FORMATS[fmt])
    m.load_weights(weights)
    eb = m._kv_bytes
    C = CFG.context_size
    src = SRC[batch]
    tokens = np.stack([synth.rand_tokens(300 + b, C, CFG.vocab_size) for b in range(batch)])
    for n in LENS:
        m.prefill(tokens, compute_logits=False)       # every position of every row holds the row's own values
        if n < C:
            m.forward(n, (tokens[:, n - 1] + 1) % CFG.vocab_size, compute_logits=False)  # the rollback
        assert m.cached_len() == n
        before = snapshot(m)
        m.fork_rows(src)
        assert m.cached_len() == n
        after = snapshot(m)
        for l in range(CFG.n_layer):
            for w in range(2):
                for b in range(batch):
                    planes_a, planes_s, planes_b = split(after[l][w][b], eb), split(before[l][w][src[b]], eb), split(before[l][w][b], eb)
                    for a, s, d in zip(planes_a, planes_s, planes_b):
                        if a is None:
                            continue
                        tag = (fmt, batch, n, l, w, b)
                        if src[b] == b:
                            assert np.array_equal(a, d), tag
                            continue
                        assert np.array_equal(a[:, :n], s[:, :n]), tag            # the source's bytes over [0, len)
                        assert np.array_equal(a[:, n:], d[:, n:]), tag            # its own bytes at and beyond len
                        assert not np.array_equal(d[:, :n], s[:, :n]), tag        # (the copy changed something)
                        if 1 < n < C:
                            assert d[:, n:].any() and not np.array_equal(d[:, n:], s[:, n:]), tag  # (and "unchanged" had something to lose)
    m.close()


def test_refusals_touch_nothing(zg, weights):
    m = zgpt.GPT(CFG, batch=3)
    m.load_weights(weights)
    tokens = np.stack([synth.rand_tokens(320 + b, 20, CFG.vocab_size) for b in range(3)])
    m.prefill(tokens, compute_logits=False)
    before = snapshot(m)

    def fork(src, n=None):
        a = np.asarray(src, np.uint64)
        return zg.zg_gpt_kv_fork(m.h, _lib.ptr(a), a.size if n is None else n)

    assert fork([0, 1], 2) == ERR_ARG          # n_rows != batch
    assert fork([0, 1, 2, 0]) == ERR_ARG
    assert zg.zg_gpt_kv_fork(m.h, None, 3) == ERR_ARG
    assert zg.zg_gpt_kv_fork(None, None, 3) == ERR_ARG
    assert fork([0, 3, 2]) == ERR_SHAPE        # a source beyond the batch
    assert fork([1, 2, 2]) == ERR_ARG          # row 0 copies row 1, which is itself overwritten
    assert fork([1, 0, 2]) == ERR_ARG          # a swap
    assert fork([0, 1, 2]) == 0                # the identity: nothing to do
    after = snapshot(m)
    assert all(np.array_equal(after[l][w][b], before[l][w][b]) for l in range(CFG.n_layer) for w in range(2) for b in range(3))
    assert fork([2, 2, 2]) == 0
    m.close()
