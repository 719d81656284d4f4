"""float64 restatement of what zg_gpt_score records (include/zgpt2.h), built on tests/logprob_ref.py and shared by the
test_score_*.py files.  logits [n, V] float32 are the rows of one sequence's pass over tokens [n]: row p holds the logits that
predict position p + 1, so column p + 1 is logprob_ref(logits[p], tokens[p + 1]); column 0 has no predicting row and reads NaN."""
import numpy as np

from logprob_ref import logprob_ref


def score_ref(logits, tokens, top_n):
    """-> (logprobs float64 [n] with NaN first, top_ids int64 [n, top_n], top_logprobs float64 [n, top_n]); the first column's ids
    and values mean nothing (zeros)."""
    logits = np.asarray(logits, np.float32)
    tokens = np.asarray(tokens).astype(np.int64)
    n = tokens.size
    assert logits.shape[0] == n
    lp = np.full(n, np.nan)
    ids = np.zeros((n, top_n), np.int64)
    top = np.zeros((n, top_n))
    for p in range(n - 1):
        lp[p + 1], ids[p + 1], top[p + 1] = logprob_ref(logits[p], tokens[p + 1], top_n)
    return lp, ids, top
