"""tests/logprob_ref.py, the float64 reference the GPU tests of the log-probability stage compare against: against
torch.log_softmax in float64, and its order on a hand-made row with ties, +-0.0 and -inf."""
import numpy as np
import torch

from logprob_ref import bound, check_values, logprob_all, logprob_ref, top_order


def test_against_torch_log_softmax_in_float64():
    rng = np.random.default_rng(3)
    for V, scale in ((1, 3.0), (65, 3.0), (4097, 3.0), (50257, 3.0), (50257, 30.0)):
        x = (scale * rng.standard_normal(V)).astype(np.float32)
        if V > 8:
            x[5] = -np.inf
            x[V // 2] = x.max() + 80.0
        want = torch.log_softmax(torch.from_numpy(x).double(), dim=0).numpy()
        got = logprob_all(x)
        fin = np.isfinite(want)
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        assert np.max(np.abs(got[fin] - want[fin])) <= 1e-12 * max(1.0, np.abs(want[fin]).max())
        tok = int(np.argmin(np.where(np.isfinite(x), x, np.inf)))
        lp, ids, top = logprob_ref(x, tok, min(5, V))
        assert lp == got[tok] and np.array_equal(top, got[ids])
        assert abs(np.exp(got[fin]).sum() - 1.0) < 1e-9


def test_order_with_ties_signed_zeros_and_minus_infinity():
    x = np.array([1.0, -np.inf, 0.0, 7.0, -0.0, 7.0, -np.inf, 1.0, -3.0, 0.0], np.float32)
    assert top_order(x, 10).tolist() == [3, 5, 0, 7, 2, 4, 9, 8, 1, 6]
    assert top_order(x, 3).tolist() == [3, 5, 0]
    assert top_order(x, 0).tolist() == []
    lp, ids, top = logprob_ref(x, 6, 10)
    assert lp == -np.inf and np.isneginf(top[-2:]).all() and np.all(top[1:] <= top[:-1])
    assert top[0] == top[1] and top[4] == top[5] == top[6]


def test_check_values_holds_the_bound_and_minus_infinity():
    ref = np.array([-1.0, -np.inf, -100.0])
    ok = np.array([-1.0 + 0.9 * bound(-1.0), -np.inf, -100.0 - 0.9 * bound(-100.0)])
    assert 0.5 < check_values(ok, ref) <= 1.0
    for bad in (np.array([-1.0 + 3e-5, -np.inf, -100.0]), np.array([-1.0, -1e30, -100.0]), np.array([-1.0, -np.inf, np.nan])):
        try:
            check_values(bad, ref)
        except AssertionError:
            continue
        raise AssertionError("check_values let %r pass" % (bad,))
