"""The overlap step of the packed column kernel on packed words (k_split_cols<.., 1>, simplex_split.inc phase 2a) on the GPU: 2 000 depth-8
families per case through the device entry, bytes and counters against the oracle, and which step corrected the families
(fgx_debug_last_packed_overlap) against the batch's own positions and lengths.  Cases and checks: tests/packed_overlap_cases.py."""
import pytest

from isolated import run_isolated
from packed_overlap_cases import CASES

pytestmark = pytest.mark.gpu

N = 2000


@pytest.mark.parametrize("name", list(CASES))
def test_overlap_step_on_the_device(name):
    run_isolated("packed_overlap_cases", "check_gpu", name, N)


def test_switched_off_on_the_device():
    run_isolated("packed_overlap_cases", "check_gpu", "len150_insert237_overlap_63", N, True, env={"FGX_S2_PACKED_OVERLAP": "0"})
