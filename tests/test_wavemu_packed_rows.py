"""The two row loops of the packed column pass (k_split_cols<.., 1>, simplex_split.inc phases 1b and 6; packed_core.h) under the wave-level host
emulator: one batch per case through fgx_process_batch_device — bytes and the 28 counters against the oracle — and then which loop the families
took (fgx_debug_last_packed_rows) against the batch's own quality bytes.  Cases and checks: tests/packed_rows_cases.py.

c_floor_30: with --min-input-base-quality 30 the emulator shows every depth-8 family in the packed build (the floor asked for; no other was needed)."""
import pytest

from isolated import run_isolated
from test_wavemu import env

CASES = {
    "a_depth8": 400,              # defaults at 150 bp: every packed family reports clean
    "b_length_147": 300,          # the last 16-byte chunk of a quality row: three qualities, then tag text with a NUL — still all clean
    "c_floor_30": 300,            # raw cycles 0 - 4 are below the floor: every packed family reports general
    "d_one_byte_below": 400,      # one byte at floor - 1, at positions 0, 7, 8, 15, 16, l_seq - 1 of the first / last record of either end: exactly those families
    "e_floor_11_byte_11": 300,    # a byte AT the floor stays clean ...
    "e_floor_11_byte_10": 300,    # ... one below it does not
    "f_long_tail": 300,           # 2 .. 50 pairs: clean + general = the packed build's families
}


@pytest.mark.parametrize("name", list(CASES))
def test_row_loops_under_the_emulator(name):
    run_isolated("packed_rows_cases", "check_emulated", name, CASES[name], env=env(), timeout=900)


def test_switched_off_every_family_is_general():
    """FGX_S2_CLEAN_ROWS=0: no clean test, the general loop (qualities read, floor applied without a branch) for every family — same bytes."""
    run_isolated("test_wavemu_packed_rows", "check_switched_off", 300, env=env(FGX_S2_CLEAN_ROWS=0), timeout=900)


def check_switched_off(n_families):
    import packed_rows_cases as pr
    seen = []
    orig = pr.check_rows
    pr.check_rows = lambda name, n, dirty, builds, rows: seen.append((builds, rows))
    try:
        pr.check_emulated("a_depth8", n_families)
    finally:
        pr.check_rows = orig
    (builds, rows), = seen
    assert rows[0] == 0 and rows[1] == builds[0] >= 0.9 * n_families, (builds, rows)
