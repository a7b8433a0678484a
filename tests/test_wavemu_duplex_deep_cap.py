"""--max-reads-per-strand decided for duplex molecules of more than 64 records by the CAP builds of k_duplex_deep_parse + k_duplex_deep_cols
(fgumi_amd/csrc/duplex_deep.inc), executed on the CPU in 64-lane lock-step (tests/wavemu — a cross-lane operation or a barrier under divergent control flow
faults there).  The checks are those of tests/duplex_deep_cap_cases.py: both entries of the emulation library against the oracle — bytes, count and all 28
counters —, the path of the device batch (deferred, fgx_debug_last_duplex_deep, fgx_debug_last_duplex_deep_capped, no simplex big / deep family), and what the
cap does to each input, read from the input.  Every case runs in a child interpreter with FGX_DUPLEX_DEEP_CAP as the test sets it (the switch is off by
default).  Without the CAP builds every such molecule is deferred and the library has no fgx_debug_last_duplex_deep_capped."""
import pytest

from isolated import run_isolated
from test_wavemu import env

T = 900
M = "duplex_deep_cap_cases"


def on(**more):
    return env(FGX_DUPLEX_DEEP_CAP="1", **more)


def test_two_molecules_under_a_cap_of_5_are_decided():
    run_isolated(M, "check_two_molecules_under_a_cap_of_5", env=on(), timeout=T)


def test_cap_of_1_takes_the_single_read_table():
    run_isolated(M, "check_cap_of_1", env=on(), timeout=T)


def test_edges_of_biting():
    run_isolated(M, "check_edges_of_biting", env=on(), timeout=T)


@pytest.mark.parametrize("min_reads", [None, (3, 2, 1)], ids=["min_reads_default", "min_reads_3_2_1"])
def test_one_strand_capped_the_other_not(min_reads):
    run_isolated(M, "check_one_strand_capped", min_reads, env=on(), timeout=T)


def test_longest_read_dropped():
    run_isolated(M, "check_longest_read_dropped", env=on(), timeout=T)


def test_rank_order_is_the_summation_order():
    run_isolated(M, "check_rank_order_is_the_summation_order", env=on(), timeout=T)


@pytest.mark.parametrize("overlapping", [0, 1], ids=["overlapping_off", "overlapping_on_is_deferred"])
def test_ties(overlapping):
    run_isolated(M, "check_ties", overlapping, env=on(), timeout=T)


def test_consensus_umi_over_all_reads():
    run_isolated(M, "check_umi_over_all_reads", env=on(), timeout=T)


def test_the_bound_under_a_cap():
    run_isolated(M, "check_the_bound_under_a_cap", env=on(), timeout=T)


@pytest.mark.parametrize("name", ["as_it_is", "long_prefix", "per_base_tags_off", "min_input_base_quality_30"])
def test_reverse_set_capped(name):
    run_isolated(M, "check_reverse_set", name, env=on(), timeout=T)


def test_error_rate_20000_under_a_cap_of_3():
    run_isolated(M, "check_error_rate", env=on(), timeout=T)


@pytest.mark.parametrize("value", ["unset", "0"])
def test_switch_off_defers_as_before(value):
    run_isolated(M, "check_switch_off", value, env=env() if value == "unset" else env(FGX_DUPLEX_DEEP_CAP=value), timeout=T)


def test_switch_is_read_per_call():
    run_isolated(M, "check_switch_is_read_per_call_here", env=env(), timeout=T)


def test_caller_without_a_cap_is_unchanged_by_the_switch():
    run_isolated(M, "check_caller_without_a_cap_here", env=env(), timeout=T)


@pytest.mark.parametrize("what", ["cap_of_0", "methylation", "trim"])
def test_still_deferred_with_the_switch_on(what):
    run_isolated(M, "check_still_deferred", what, env=on(), timeout=T)
