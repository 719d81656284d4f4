"""zg_init_ex, zg_shutdown and initialising again (include/zgpt2.h, runtime section), which no test called.

zg_shutdown frees the arenas every handle of the process stages through, so the sequence runs in a child process of its own
(tests/lifecycle_worker.py, one JSON line back), never in the session's process, where other tests hold handles.  The children
run one after the other: one process has the GPU open at a time beside the session's.

What the child does, and what is asserted on its line:

1. zg_init_ex(0, 1 MiB): a Linear whose host weight (1.44 MB) exceeds the arena returns ZG_ERR_STAGING; the next one, which fits,
   is right against the oracle (here and below: golden_io.assert_ref_close, element by element, with test_ops_gpu.py's floor
   for seeded inputs, evaluated in the child).
2. zg_init(1) while initialised on device 0: ZG_ERR_ARG (zg_init(0): ZG_OK, idempotent).  In a second child, before any init:
   a device index out of range and a negative one are ZG_ERR_ARG, and the library stays uninitialised.
3. A `tiny` handle generates 32 tokens greedily and with temp 0.8 / seed 3 and is destroyed; a weight is registered; three
   positions of zg_attn_forward over host caches; zg_shutdown.
4. Then zg_set_stream, zg_synchronize, zg_register_tensor, zg_linear_forward and zg_gpt_create all return
   ZG_ERR_NOT_INITIALIZED, and a second zg_shutdown ZG_OK.
5. zg_init(0) again: the same generations give the same tokens; the once-registered host weight, changed in place and not
   registered again, is multiplied by its new bytes (the registry did not survive); the host caches, overwritten with another
   sequence's rows, give that sequence's position 4 (the mirror did not survive: the rows were uploaded again).  Both come
   with the error a survivor would have shown (1.5 and 1.1 of the output scale, against 1.1e-7 and 2.3e-7 measured), so the two
   checks have teeth.
6. The same life with the library on a caller's stream at the moment of zg_shutdown: ZG_OK, the caller's stream still works,
   a third init generates the same tokens.

Not tested, because it is a caller error whose test would be a fault on purpose: zg_shutdown with handles alive (the header
says they must be destroyed first).

Measured on one MI355X: 6 tests; the main child 2.3 s (three library initialisations, four handle lives), the second child 1.8 s
(both mostly python and torch starting).  No defect was found: every status and every result was as the header says.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NOT_INITIALIZED, STAGING, ARG = 0, -1, -4, -6


def run_worker(mode):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lifecycle_worker.py"), mode], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"{mode}: exit {out.returncode}\n{out.stderr[-3000:]}"
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def life():
    return run_worker("main")


def test_small_arena_refuses_what_does_not_fit_and_runs_what_does(life):
    assert life["init_ex"] == OK
    assert life["linear_beyond_arena"] == STAGING
    assert life["linear_fits"] == OK and life["linear_fits_close"] == ""


def test_second_init_keeps_the_device(life):
    assert life["init_other_device"] == ARG and life["init_same_device"] == OK


def test_device_out_of_range_before_any_init():
    r = run_worker("bad_device")
    assert r == {"init_ex_device_out_of_range": ARG, "init_negative_device": ARG, "synchronize_uninitialised": NOT_INITIALIZED}


def test_every_entry_refuses_after_shutdown(life):
    assert life["register"] == OK and life["attn_close_before"] == "" and life["shutdown_1"] == OK
    assert life["after_shutdown"] == {n: NOT_INITIALIZED for n in ("zg_set_stream", "zg_synchronize", "zg_register_tensor", "zg_linear_forward", "zg_gpt_create")}
    assert life["shutdown_twice"] == OK


def test_a_second_life_is_a_fresh_one(life):
    assert life["init_again"] == OK
    assert life["tokens_2"] == life["tokens_1"] and len(life["tokens_1"][0]) == 32 and life["tokens_1"][0] != life["tokens_1"][1]
    print(f"LIFECYCLE registry: {life['linear_after_err']:.2e} (a survivor: {life['linear_after_err_if_stale']:.2f}); "
          f"KV mirror: {life['attn_err_after']:.2e} (a survivor: {life['attn_err_if_stale']:.2f})")
    assert life["linear_after_err_if_stale"] > 1.0 and life["attn_rows_differ"] and life["attn_err_if_stale"] > 0.05  # the checks below have teeth
    assert life["linear_after"] == OK and life["linear_after_close"] == ""
    assert life["attn_close_after"] == ""


def test_shutdown_on_a_callers_stream(life):
    assert life["set_stream"] == OK and life["register_3"] == OK
    assert life["tokens_3"] == life["tokens_1"]
    assert life["shutdown_on_caller_stream"] == OK and life["after_shutdown_2"] == NOT_INITIALIZED
    assert life["caller_stream_alive"] == 28
    assert life["init_third"] == OK and life["tokens_4"] == life["tokens_1"] and life["shutdown_3"] == OK
