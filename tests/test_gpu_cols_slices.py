"""The packed column kernel's scalar state and its first LDS slice (k_split_cols<.., 1>) on the GPU: one small batch per case through the device
entry, bytes and counters against the oracle, and which build finished the families and how many the first launch handed on
(fgx_debug_last_split_builds).  Cases and checks: tests/cols_slices_cases.py (a: the benchmark's shape, 64 families; b: a fragment-only family and
a family of 8 + 6 rows among pair families in one workgroup; c: reads of 147 and 151 bases; d: 2 x 100 bases, the generic-stride build; e: families
that fill the first slice to the byte, need one item more, need twice the room; f: ends of 20 rows, two items per column)."""
import pytest

from isolated import run_isolated
from test_wavemu_cols_slices import CASES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", CASES)
def test_cols_slices_on_the_device(name):
    run_isolated("cols_slices_cases", "check_gpu", name)
