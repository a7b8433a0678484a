"""k_call_full's result array (fgumi_amd/csrc/fastpath.h, FullResult) on the GPU: 2 000 families per case through the device entry, bytes and the 28
counters against the oracle, and the path the answers took (fgx_debug_last_full_results).  Cases and checks: tests/full_results_cases.py."""
import pytest

from isolated import run_isolated

pytestmark = pytest.mark.gpu

CASES = ["a_defaults", "b_length_8", "b_length_9", "b_length_147", "b_length_149", "b_length_151", "b_length_255", "b_length_256", "c_noisy_2pct", "c_noisy_5pct",
         "d_length_257", "e_long_tail", "f_min_reads_3", "f_min_quality_40"]


@pytest.mark.parametrize("name", CASES)
def test_result_array_on_the_device(name):
    run_isolated("full_results_cases", "check_gpu", name, 2000, env=dict(FGX_FULL_RESULTS="1"))


def test_single_end_families_on_the_device():
    run_isolated("full_results_cases", "check_gpu", "d_fragments", 300, env=dict(FGX_FULL_RESULTS="1"))     # (the records are re-encoded in Python: fewer families)


def test_switched_off_on_the_device():
    run_isolated("full_results_cases", "check_gpu", "g_switched_off", 2000, env=dict(FGX_FULL_RESULTS="0"))


def test_variable_unset_is_the_default_on_the_device():
    import os
    assert "FGX_FULL_RESULTS" not in os.environ      # (the child inherits this environment)
    run_isolated("full_results_cases", "check_gpu", "g_unset", 2000)


def test_ranges_cut_at_a_lists_end_on_the_device():
    run_isolated("full_results_cases", "check_gpu", "h_cut_ranges", 2000, env=dict(FGX_FULL_RESULTS="1", FGX_POOL_DIV=str(1 << 20), FGX_POOL_SLACK="8"))
