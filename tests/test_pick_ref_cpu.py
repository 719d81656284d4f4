"""tests/pick_ref.py — the rule the GPU tests hold the greedy pick to — pinned on rows written by hand."""
import numpy as np

from pick_ref import pick_row, pick_rows

NAN, INF = float("nan"), float("inf")


def test_greater_value_first():
    assert pick_row([1.0, 3.0, 2.0], [10, 20, 30], 100) == 20
    assert pick_row([-5.0], [7], 100) == 7


def test_lower_index_on_ties_wherever_it_sits():
    assert pick_row([2.0, 2.0, 2.0], [30, 10, 20], 100) == 10
    assert pick_row([1.0, 2.0, 0.0, 2.0], [1, 9, 2, 4], 100) == 4
    assert pick_row([0.0, -0.0], [8, 3], 100) == 3  # one value
    assert pick_row([-0.0, 0.0], [3, 8], 100) == 3


def test_nan_never_takes_over():
    assert pick_row([NAN, 1.0, NAN, 0.5], [1, 2, 3, 4], 100) == 2
    assert pick_row([NAN, NAN], [5, 6], 100) == 0  # the start index stands and is clamped


def test_the_start_value_stands_against_what_is_not_above_it():
    assert pick_row([-INF, -INF], [5, 6], 100) == 0
    assert pick_row([-3.0e38, -INF], [5, 6], 100) == 5  # equal to the start value, lower index than 2^31 - 1
    assert pick_row([INF, 1.0], [5, 6], 100) == 5


def test_an_index_outside_the_vocabulary_gives_zero():
    assert pick_row([1.0, 9.0], [3, 100], 100) == 0
    assert pick_row([1.0, 9.0], [3, 99], 100) == 99
    assert pick_row([1.0, 9.0], [3, -1], 100) == 0  # (a negative index wins the tie-break too, and is clamped)
    assert pick_row([9.0, 9.0], [3, -7], 100) == 0


def test_rows():
    assert pick_rows(np.array([[1.0, 2.0], [2.0, 1.0]], np.float32), np.array([[4, 5], [6, 7]], np.int32), 10) == [5, 6]
