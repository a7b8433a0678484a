"""GPU parity: --max-reads-per-strand decided for duplex molecules of more than 64 records by the CAP builds of k_duplex_deep_parse + k_duplex_deep_cols
(fgumi_amd/csrc/duplex_deep.inc).  The checks are those of tests/duplex_deep_cap_cases.py: both entries against the oracle byte for byte, count and all 28
counters included, the path of the device batch (deferred, fgx_debug_last_duplex_deep, fgx_debug_last_duplex_deep_capped, no simplex big / deep family), and
what the cap does to each input, read from the input.  The switch FGX_DUPLEX_DEEP_CAP is off by default: every test sets it.  Without the CAP builds every
such molecule is deferred and the library has no fgx_debug_last_duplex_deep_capped."""
import pytest

import duplex_deep_cap_cases as K
from isolated import run_isolated

pytestmark = pytest.mark.gpu


@pytest.fixture
def on(monkeypatch):
    monkeypatch.delenv("FGX_DUPLEX_DEEP", raising=False)
    monkeypatch.setenv(K.SWITCH, "1")


def test_two_molecules_under_a_cap_of_5_are_decided(on):
    K.check_two_molecules_under_a_cap_of_5()


def test_cap_of_1_takes_the_single_read_table(on):
    K.check_cap_of_1()


def test_edges_of_biting(on):
    K.check_edges_of_biting()


@pytest.mark.parametrize("min_reads", [None, (3, 2, 1)], ids=["min_reads_default", "min_reads_3_2_1"])
def test_one_strand_capped_the_other_not(on, min_reads):
    K.check_one_strand_capped(min_reads)


def test_longest_read_dropped(on):
    K.check_longest_read_dropped()


def test_rank_order_is_the_summation_order(on):
    K.check_rank_order_is_the_summation_order()


@pytest.mark.parametrize("overlapping", [0, 1], ids=["overlapping_off", "overlapping_on_is_deferred"])
def test_ties(on, overlapping):
    K.check_ties(overlapping)


def test_consensus_umi_over_all_reads(on):
    K.check_umi_over_all_reads()


def test_the_bound_under_a_cap(on):
    K.check_the_bound_under_a_cap()


@pytest.mark.parametrize("name", list(K.OPTIONS))
def test_reverse_set_capped(on, name):
    K.check_reverse_set(name)


def test_error_rate_20000_under_a_cap_of_3(on):
    K.check_error_rate()


@pytest.mark.parametrize("value", ["unset", "0"])
def test_switch_off_defers_as_before(monkeypatch, value):
    monkeypatch.delenv("FGX_DUPLEX_DEEP", raising=False)
    if value == "unset":
        monkeypatch.delenv(K.SWITCH, raising=False)
    else:
        monkeypatch.setenv(K.SWITCH, value)
    K.check_switch_off(value)


def test_switch_is_read_per_call(monkeypatch):
    monkeypatch.delenv("FGX_DUPLEX_DEEP", raising=False)
    K.check_switch_is_read_per_call(monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))


def test_caller_without_a_cap_is_unchanged_by_the_switch(monkeypatch):
    monkeypatch.delenv("FGX_DUPLEX_DEEP", raising=False)
    K.check_caller_without_a_cap(monkeypatch.setenv)


@pytest.mark.parametrize("what", ["cap_of_0", "methylation", "trim"])
def test_still_deferred_with_the_switch_on(on, what):
    K.check_still_deferred(what)


def test_mixed_stream_run_bam(tmp_path):
    run_isolated("duplex_deep_cap_cases", "check_run_bam", str(tmp_path), env={K.SWITCH: "1"}, timeout=600)


def test_under_guard_bands():
    run_isolated("duplex_deep_cap_cases", "check_under_guard_bands", env={K.SWITCH: "1", "FGX_GUARD_BAND": "4096"}, timeout=600)
