"""The greedy pick from a row's argmax partials, restated: from (-3.0e38, 0x7fffffff), partial p takes over iff its value is greater,
or equal with a lower index; an index outside [0, vocab) gives token 0.  float32 compares, so NaN never takes over and -0.0 == +0.0."""
import numpy as np


def pick_row(part_val, part_idx, vocab):
    bv, bi = np.float32(-3.0e38), 0x7FFFFFFF
    for v, i in zip(np.asarray(part_val, np.float32), np.asarray(part_idx, np.int64)):
        if v > bv or (v == bv and int(i) < bi):
            bv, bi = v, int(i)
    return bi if 0 <= bi < vocab else 0


def pick_rows(part_val, part_idx, vocab):
    return [pick_row(v, i, vocab) for v, i in zip(part_val, part_idx)]
