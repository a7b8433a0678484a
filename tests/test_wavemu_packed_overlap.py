"""The overlap step of the packed column kernel on packed words (k_split_cols<.., 1>, simplex_split.inc phase 2a; packed_core.h ov_step) under the
wave-level host emulator: 300 depth-8 families per case through fgx_process_batch_device — bytes and the 28 counters against the oracle — and
then which step corrected the families (fgx_debug_last_packed_overlap) against the batch's own positions and lengths.  Cases and checks:
tests/packed_overlap_cases.py — overlaps of about 1, 7, 63, 148 bases, the whole read and none at read lengths 150, 147 and 151 (insert_sd 3: each
case meets several misalignments), code 15 in shared positions, floors 30 and 7 (the lowest at which a depth-8 family is the packed build's),
shared qualities of 128 and 200 (the guard), the switch off."""
import pytest

from isolated import run_isolated
from packed_overlap_cases import CASES
from test_wavemu import env

N = 300


@pytest.mark.parametrize("name", list(CASES))
def test_overlap_step_under_the_emulator(name):
    run_isolated("packed_overlap_cases", "check_emulated", name, N, env=env(), timeout=900)


@pytest.mark.parametrize("name", ["len150_insert237_overlap_63", "quality_128_and_200_in_shared_positions"])
def test_switched_off_every_family_is_corrected_byte_by_byte(name):
    """FGX_S2_PACKED_OVERLAP=0: the byte-wise steps for every family — same bytes, no family counted as packed or as the guard's."""
    run_isolated("packed_overlap_cases", "check_emulated", name, N, True, env=env(FGX_S2_PACKED_OVERLAP=0), timeout=900)
