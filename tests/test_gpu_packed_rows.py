"""The two row loops of the packed column pass (k_split_cols<.., 1>) on the GPU: 2 000 families per case through the device entry, bytes and
counters against the oracle, and which loop the families took (fgx_debug_last_packed_rows) against the batch's own quality bytes.  Cases and
checks: tests/packed_rows_cases.py (a: defaults, all clean; b: 147-base reads, tag text behind the last qualities; c: floor 30, all general;
d: one byte at floor - 1 in chosen families, exactly those general)."""
import pytest

from isolated import run_isolated

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["a_depth8", "b_length_147", "c_floor_30", "d_one_byte_below"])
def test_row_loops_on_the_device(name):
    run_isolated("packed_rows_cases", "check_gpu", name, 2000)
