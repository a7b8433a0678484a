"""The packed column kernel's scalar state and its first LDS slice (k_split_cols<.., 1>, simplex_split.inc; the slice: s2_first_slice_bytes, fastpath.h)
under the wave-level host emulator: one small batch per case through fgx_process_batch_device — bytes and the 28 counters against the oracle — and
then which build finished the families and how many the first launch handed on (fgx_debug_last_split_builds).  Cases and checks:
tests/cols_slices_cases.py."""
import pytest

from isolated import run_isolated
from test_wavemu import env

CASES = [
    "a_flagship_64",             # 64 depth-8 families of 2 x 150 bases, as the benchmark has them
    "b_unequal_ends",            # a fragment-only family and a family of 8 + 6 rows (two runs of the pass) among pair families in one workgroup
    "c_lengths_147_151",         # the last group of eight pulled back or padded; reverse ends: byte-swapped counters
    "d_length_100",              # strides that are not 160 / 80: the generic packed build
    "e_slice_room",              # descriptors + items that fill the first slice to the byte stay; one item more, or twice the room: the second launch
    "f_two_items_per_column",    # ends of 20 rows: two items per column, the family's items in one list
]


@pytest.mark.parametrize("name", CASES)
def test_cols_slices_under_the_emulator(name):
    run_isolated("cols_slices_cases", "check_emulated", name, env=env(), timeout=900)


@pytest.mark.parametrize("name", ["b_unequal_ends", "e_slice_room", "f_two_items_per_column"])
def test_the_oracle_calls_the_crafted_families(name):
    """The oracle alone: every end of every crafted family gets its consensus record."""
    run_isolated("cols_slices_cases", "check_oracle_accepts", name, env=env(), timeout=300)
