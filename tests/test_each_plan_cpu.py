"""zg_debug_each_plan (include/zgpt2.h): what a table of per-row sampling parameters is launched as — the form of
every row by its own parameters, the union the chain is launched in, whether the penalty stage runs — and the refusals of a
table, with the row named.  Needs neither a GPU nor zg_init."""
import ctypes as C

import pytest

from zig_gpt2_amd import _lib

PLAIN, ONE, TWO, MINP = 1, 2, 3, 4  # the SamplerMode numbering
ARG = -6
V = 257
# one row of each kind, by generate_sample's keyword names
KINDS = {
    "plain": (dict(temp=0.8), PLAIN),
    "top_k": (dict(temp=0.8, top_k=40), ONE),
    "top_p": (dict(temp=1.7, top_p=0.9), ONE),
    "both": (dict(temp=0.3, top_k=5, top_p=0.5), TWO),
    "min_p": (dict(temp=0.8, min_p=0.05), MINP),
    "top_k >= vocab": (dict(temp=0.8, top_k=V), PLAIN),
    "top_k > vocab, top_p == 1": (dict(temp=0.8, top_k=10 * V, top_p=1.0), PLAIN),
    "top_k off by size + min_p": (dict(temp=0.8, top_k=V + 1, min_p=0.5), MINP),
    "top_k = vocab - 1": (dict(temp=0.8, top_k=V - 1), ONE),
    "top_k + min_p": (dict(temp=0.8, top_k=3, min_p=0.1), ONE),
    "top_p + min_p": (dict(temp=0.8, top_p=0.5, min_p=0.1), ONE),
    "greedy (temp 0)": (dict(temp=0), ONE),
    "greedy (temp None)": (dict(temp=None, top_p=0.9), TWO),
}
PEN = dict(repetition_penalty=1.3)


def plan(rows, vocab=V, n_out=None):
    """(rc, chain form, penalty stage, [row forms]) of a list of row dicts, or of a prepared ctypes array."""
    lib = _lib.load()
    table = rows if not isinstance(rows, list) else _lib.row_sampling(rows)
    n = len(rows)
    out = (C.c_int * (2 + n))()
    rc = lib.zg_debug_each_plan(C.addressof(table), n, vocab, out, 2 + n if n_out is None else n_out)
    return rc, out[0], out[1], list(out[2:])


@pytest.mark.parametrize("kind", list(KINDS))
def test_form_of_each_kind_of_row(kind):
    row, form = KINDS[kind]
    assert plan([row]) == (0, form, 0, [form])
    # beside plain neighbours the row keeps its form and the chain takes it
    assert plan([KINDS["plain"][0], row, KINDS["plain"][0]]) == (0, form, 0, [PLAIN, form, PLAIN])


def test_union_over_mixed_tables():
    k = {name: row for name, (row, _) in KINDS.items()}
    assert plan([k["plain"], k["min_p"]])[:2] == (0, MINP)
    assert plan([k["min_p"], k["plain"]])[:2] == (0, MINP)
    assert plan([k["top_k"], k["top_p"]]) == (0, ONE, 0, [ONE, ONE])
    assert plan([k["top_p"], k["min_p"], k["plain"]]) == (0, ONE, 0, [ONE, MINP, PLAIN])
    for name, row in k.items():  # anything + both
        assert plan([row, k["both"]])[:2] == (0, TWO), name
        assert plan([k["both"], row])[:2] == (0, TWO), name
    eight = [k["plain"], k["top_k"], k["top_p"], k["both"], k["min_p"], k["top_k + min_p"], k["top_p + min_p"], k["plain"]]
    assert plan(eight) == (0, TWO, 0, [PLAIN, ONE, ONE, TWO, MINP, ONE, ONE, PLAIN])


def test_penalty_stage_iff_some_row_is_penalised():
    plain = KINDS["plain"][0]
    off = dict(plain, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)
    assert plan([plain, off, plain])[2] == 0
    for pen in (dict(repetition_penalty=1.3), dict(presence_penalty=0.4), dict(frequency_penalty=-0.15)):
        for at in range(3):
            rows = [dict(plain) for _ in range(3)]
            rows[at].update(pen)
            assert plan(rows) == (0, PLAIN, 1, [PLAIN] * 3), (pen, at)
    assert plan([dict(KINDS["both"][0], **PEN), KINDS["min_p"][0]]) == (0, TWO, 1, [TWO, MINP])


BAD = [
    (dict(temp=-1.0), "temperature"),
    (dict(temp=float("nan")), "temperature"),
    (dict(temp=0.8, top_p=0.0), "top_p"),
    (dict(temp=0.8, top_p=1.5), "top_p"),
    (dict(temp=0.8, top_p=float("nan")), "top_p"),
    (dict(temp=0.8, min_p=1.0), "min_p"),
    (dict(temp=0.8, min_p=-0.1), "min_p"),
    (dict(temp=0.8, min_p=float("nan")), "min_p"),
    (dict(temp=0.8, repetition_penalty=0.0), "repetition"),
    (dict(temp=0.8, repetition_penalty=float("nan")), "repetition"),
    (dict(temp=0.8, presence_penalty=float("inf")), "presence"),
    (dict(temp=0.8, frequency_penalty=float("nan")), "frequency"),
]


@pytest.mark.parametrize("row,word", BAD)
def test_a_bad_row_is_refused_and_named(row, word):
    lib = _lib.load()
    good = KINDS["top_k"][0]
    for at in (0, 2, 7):
        rows = [dict(good) for _ in range(8)]
        rows[at] = row
        rc = plan(rows)[0]
        msg = lib.zg_last_error().decode()
        assert rc == ARG and f"row {at}" in msg and word in msg, (rc, msg)


def test_a_missing_table_or_room_is_refused():
    lib = _lib.load()
    out = (C.c_int * 10)()
    assert lib.zg_debug_each_plan(None, 8, V, out, 10) == ARG and "rows" in lib.zg_last_error().decode()
    table = _lib.row_sampling([KINDS["plain"][0]] * 8)
    assert lib.zg_debug_each_plan(C.addressof(table), 0, V, out, 10) == ARG
    assert lib.zg_debug_each_plan(C.addressof(table), 8, V, out, 9) == ARG  # no room for the last row's form
    assert lib.zg_debug_each_plan(C.addressof(table), 8, V, None, 10) == ARG
    assert lib.zg_debug_each_plan(C.addressof(table), 8, 0, out, 10) == ARG
    assert lib.zg_debug_each_plan(C.addressof(table), 8, V, out, 10) == 0


def test_row_sampling_maps_the_keyword_names():
    t = _lib.row_sampling([dict(temp=0.7, top_k=3, top_p=0.9, min_p=0.1, repetition_penalty=1.2, presence_penalty=0.3, frequency_penalty=0.4, seed=2**63 + 5),
                           dict(temp=0, top_k=9), dict()])
    assert (round(t[0].options.temp, 6), t[0].options.top_k, round(t[0].options.top_p, 6), round(t[0].min_p, 6)) == (0.7, 3, 0.9, 0.1)
    assert (round(t[0].penalties.repetition, 6), round(t[0].penalties.presence, 6), round(t[0].penalties.frequency, 6), t[0].seed) == (1.2, 0.3, 0.4, 2**63 + 5)
    assert (t[1].options.temp, t[1].options.top_k) == (1.0, 1)  # a row's greedy
    assert (t[2].options.temp, t[2].options.top_k, t[2].options.top_p, t[2].min_p, t[2].penalties.repetition, t[2].seed) == (1.0, 0, 1.0, 0.0, 1.0, 0)
    with pytest.raises(TypeError):
        _lib.row_sampling([dict(temperature=0.7)])
