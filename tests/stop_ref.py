"""The matching rules of stop tokens and stop sequences (include/zgpt2.h zg_stop_conditions), restated in plain Python.

tokens [rows][cols]: what every column of a row records; first_cols[b]: the first column row b PICKED (columns below it record
prompt tokens).  Conditions are numbered over the concatenated list: j < len(ids) is stop token ids[j], len(ids) + k is stop
sequence seqs[k].  Condition j matches at column p of row b when p is a picked column and either it is a stop token equal to the
token at p, or it is a sequence of L tokens, columns p - L + 1 .. p are all picked columns and hold the sequence.  A row finishes
at the lowest column at which anything matches, with the lowest condition matching there."""


def matches_at(row, first_col, p, ids, seqs):
    """The indices of the conditions that match at column p of `row`, ascending."""
    if p < first_col:
        return []
    out = [j for j, t in enumerate(ids) if int(row[p]) == int(t)]
    for k, q in enumerate(seqs):
        L = len(q)
        if L >= 1 and p - L + 1 >= first_col and [int(t) for t in row[p - L + 1: p + 1]] == [int(t) for t in q]:
            out.append(len(ids) + k)
    return out


def finish(tokens, first_cols, ids=(), seqs=(), n_cols=None):
    """(finish_cols, reasons) of every row over columns < n_cols (all of them by default): the column is None and the reason -1 for a
    row that never matches."""
    ids, seqs = list(ids or []), [list(q) for q in (seqs or [])]
    cols, reasons = [], []
    for row, first in zip(tokens, first_cols):
        n = len(row) if n_cols is None else n_cols
        col, why = None, -1
        for p in range(n):
            m = matches_at(row, int(first), p, ids, seqs)
            if m:
                col, why = p, m[0]
                break
        cols.append(col)
        reasons.append(why)
    return cols, reasons


def done_col(finish_cols):
    """The highest finish column + 1 once every row has one, else 0 (what the kernel tells the host)."""
    return 0 if any(c is None for c in finish_cols) else max(finish_cols) + 1


# Hand-written cases: (name, tokens, first_cols, ids, seqs, finish_cols, reasons)
CASES = [
    ("the lowest column wins", [[5, 1, 2, 3, 2, 1]], [1], [3, 2], [], [2], [1]),
    ("the lowest condition wins a tie at one column", [[0, 1, 2, 3]], [0], [9, 3], [[2, 3], [3]], [3], [1]),
    ("a tie between a sequence and a later stop token", [[0, 1, 2, 3]], [0], [], [[1, 2, 3], [2, 3], [3]], [3], [0]),
    ("a sequence reaching into the prompt does not match", [[7, 8, 9, 7, 8, 9]], [1], [], [[7, 8, 9]], [5], [0]),
    ("... and never matches when only the prompt completes it", [[7, 8, 9, 1, 1, 1]], [2], [], [[7, 8, 9], [8, 9]], [None], [-1]),
    ("an overlapping prefix: a a b in a a a b", [[4, 4, 4, 6]], [0], [], [[4, 4, 6]], [3], [0]),
    ("a sequence that is a suffix of another", [[1, 2, 3, 4]], [0], [], [[2, 3, 4], [3, 4]], [3], [0]),
    ("... the shorter one alone matches where the longer is cut by the prompt", [[1, 2, 3, 4]], [2], [], [[2, 3, 4], [3, 4]], [3], [1]),
    ("a one-token sequence equals the stop token", [[1, 2, 3], [1, 2, 3]], [0, 0], [3], [[2]], [1, 1], [1, 1]),
    ("a stop token in the prompt is not a pick", [[3, 3, 1, 3]], [2], [3], [], [3], [0]),
    ("a match at the first picked column and at the last column", [[0, 5, 1, 1], [0, 0, 0, 5]], [1, 3], [5], [], [1, 3], [0, 0]),
    ("a sequence longer than what the row has picked so far", [[1, 2, 1, 2, 1, 2]], [3], [], [[1, 2, 1, 2], [2, 1, 2]], [5], [1]),
    ("one row never matches", [[1, 2, 3], [4, 4, 4]], [0, 0], [2], [], [1, None], [0, -1]),
]
