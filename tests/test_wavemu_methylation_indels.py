"""Indel reads in the methylation-aware mode (EM-Seq / TAPs) of the duplex and the simplex caller through the canonical second pass (FGX_METH_CANON=1), in the wave-level
emulator (tests/wavemu: the real api.cpp, the real launch chain and kernel sources, 64 lanes in lock-step on the CPU): the canonical form with its reference
runs (canon_core.h, reject_core.h, canon_device.hip on the host), k_family_wave<1, 1> and k_deep_parse<.., .., 1> / k_deep_cols<1> looking the reference base up through the
anchor's runs, both entries, against the oracle.

Batches: tests/methsim.py's duplex molecules (`D` and `S` kinds beside `M`); crafted molecules with hand-written MM / ML / cu / ct (tests/methindel_cases.py).
Without this change the library ignores the switch: nothing is canonicalised and the indel molecules stay deferred, so every switch-on test fails there."""
import os

import pytest

import methindel_cases as mi
from isolated import run_isolated
from test_wavemu import env


def check_batch(mode, min_reads, n_groups, seed, entry, switch=True, shared=False):
    mi.check_duplex_batch(mode, min_reads, n_groups, seed, entry, False, switch, shared)


def check_crafted(entry):
    mi.check_crafted(entry, False)


def check_switch_value(is_on):
    """(child interpreter, FGX_METH_CANON as the test set it) a small duplex batch: canonicalised or left deferred."""
    contigs, groups = mi.duplex_batch(120, 61)
    g = mi.GroupedReads_from(groups)
    got = mi.product(mi.mc.options(1, 1), contigs, g, "device", False)
    assert got["first_deferred"] > 0 and (got["canon"] > 0) == is_on, (got["first_deferred"], got["canon"], is_on)
    assert (len(got["deferred"]) == 0) == is_on, got["deferred"]


def check_simplex(mode, n_groups, seed, entry, switch=True, kw=None):
    mi.check_simplex_batch(mode, n_groups, seed, entry, False, switch, kw)


def check_crafted_simplex(entry):
    mi.check_crafted_simplex(entry, False)


def on(**kw):
    return env(FGX_METH_CANON=1, **kw)


def off():
    e = env()
    assert "FGX_METH_CANON" not in os.environ
    return e


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("mode", [1, 2], ids=["em_seq", "taps"])
def test_duplex_indel_molecules_in_the_emulated_kernels(mode, entry):
    """300 molecules, about a seventh of them with a deletion in the forward reads of both strands."""
    run_isolated("test_wavemu_methylation_indels", "check_batch", mode, (1, 1, 0), 300, 60 + mode, entry, env=on(), timeout=1500)


def test_duplex_indel_molecules_under_min_reads_3_2_1():
    """Molecules whose indel reads share ONE deletion or insertion (so that the alignment filter keeps them), depth 2 .. 4 per strand."""
    run_isolated("test_wavemu_methylation_indels", "check_batch", 1, (3, 2, 1), 200, 63, "device", True, True, env=on(), timeout=1500)


def test_duplex_indel_molecules_canonicalised_on_the_host_cores():
    """FGX_CANON_DEVICE=0: the host variant of the pass fills the same runs table."""
    run_isolated("test_wavemu_methylation_indels", "check_batch", 1, (1, 1, 0), 300, 61, "host", env=on(FGX_CANON_DEVICE=0), timeout=1500)


@pytest.mark.parametrize("entry", ["device", "host"])
def test_crafted_duplex_molecules(entry):
    """Forward anchor `10M2D10M`; a reverse anchor with a deletion cut by its mate clip; an insertion column over what a one-block rule takes for a cytosine;
    the LAST of two longest reads; a minority indel read dropped by the filter; an R2 anchor; a contig outside the genome; a run crossing the contig end."""
    run_isolated("test_wavemu_methylation_indels", "check_crafted", entry, env=on(), timeout=900)


@pytest.mark.parametrize("entry", ["device", "host"])
def test_switch_unset_keeps_indel_molecules_deferred(entry):
    run_isolated("test_wavemu_methylation_indels", "check_batch", 1, (1, 1, 0), 300, 61, entry, False, env=off(), timeout=1500)


# ---- simplex --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("mode", [1, 2], ids=["em_seq", "taps"])
def test_simplex_indel_families_in_the_emulated_kernels(mode, entry):
    """400 groups (tests/methsim.py draws `D I S` beside `M`): fragments of both orientations, pairs, overlapping pairs, depth 1 .. 7, a contig outside the header now and then."""
    run_isolated("test_wavemu_methylation_indels", "check_simplex", mode, 400, 70 + mode, entry, env=on(), timeout=1500)


def test_simplex_indel_families_under_max_reads():
    run_isolated("test_wavemu_methylation_indels", "check_simplex", 1, 400, 73, "device", True, dict(max_reads=3), env=on(), timeout=1500)


def test_simplex_indel_families_canonicalised_on_the_host_cores():
    run_isolated("test_wavemu_methylation_indels", "check_simplex", 1, 400, 71, "host", env=on(FGX_CANON_DEVICE=0), timeout=1500)


@pytest.mark.parametrize("entry", ["device", "host"])
def test_crafted_simplex_families(entry):
    run_isolated("test_wavemu_methylation_indels", "check_crafted_simplex", entry, env=on(), timeout=900)


@pytest.mark.parametrize("value,is_on", [("0", False), ("", False), ("00", False), ("yes", True), ("2", True)], ids=["0", "empty", "00", "yes", "2"])
def test_the_switch_is_on_when_set_to_something_not_starting_with_0(value, is_on):
    """Read per call like the other switches: `FGX_METH_CANON` counts as on only when set to something that does not start with `0` (the empty string is off)."""
    run_isolated("test_wavemu_methylation_indels", "check_switch_value", is_on, env=env(FGX_METH_CANON=value), timeout=900)


def test_switch_unset_keeps_indel_families_deferred():
    run_isolated("test_wavemu_methylation_indels", "check_simplex", 1, 400, 71, "device", False, env=off(), timeout=1500)
