"""tests/stop_ref.py, the Python restatement of the stop conditions' matching rules, pinned on hand-written cases (the same cases
the kernel is held to in test_stop_rows_gpu.py)."""
import pytest

import stop_ref


@pytest.mark.parametrize("case", stop_ref.CASES, ids=[c[0] for c in stop_ref.CASES])
def test_hand_written_case(case):
    _, tokens, first_cols, ids, seqs, want_cols, want_reasons = case
    cols, reasons = stop_ref.finish(tokens, first_cols, ids, seqs)
    assert cols == want_cols and reasons == want_reasons


def test_the_cases_cover_what_they_are_there_for():
    names = " | ".join(c[0] for c in stop_ref.CASES)
    for what in ("lowest column", "lowest condition", "into the prompt", "overlapping prefix", "suffix of another", "one-token sequence"):
        assert what in names, what


def test_matches_at_lists_every_condition_ascending():
    assert stop_ref.matches_at([0, 1, 2, 3], 0, 3, [9, 3], [[2, 3], [3], [1, 3]]) == [1, 2, 3]
    assert stop_ref.matches_at([0, 1, 2, 3], 3, 3, [9, 3], [[2, 3], [3]]) == [1, 3]
    assert stop_ref.matches_at([0, 1, 2, 3], 4, 3, [3], [[3]]) == []


def test_columns_limit_and_done_col():
    tokens, first = [[1, 2, 3, 4], [4, 3, 2, 1]], [0, 0]
    assert stop_ref.finish(tokens, first, [4]) == ([3, 0], [0, 0])
    assert stop_ref.finish(tokens, first, [4], n_cols=3) == ([None, 0], [-1, 0])
    assert stop_ref.done_col([3, 0]) == 4 and stop_ref.done_col([None, 0]) == 0
