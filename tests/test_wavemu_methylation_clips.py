"""Soft- / hard-clipped reads in the methylation-aware mode (EM-Seq / TAPs) decided by the device-resident pipeline, in the wave-level emulator
(tests/wavemu: the real launch chain and kernel sources, 64 lanes in lock-step on the CPU): the clip-taking build of the streaming record kernel
(k_deep_parse<.., .., 1>: CIGAR walk, general mate clip, shared span from the aligned blocks, anchor at pos / pos + T - 1) for the simplex caller,
k_family_wave<1, 1> without its one-op deferral for the duplex caller, against the oracle.

The batches hold `M` and `S` reads only (tests/methclip_cases.py), so every group is the kernels' shape: a deferral here is the new code's.  Before
this change every group with a clipped record was deferred — `n_deferred == 0` and the `fgx_debug_last_meth_clipped` count fail on that code."""
import pytest

import methclip_cases as mc
from isolated import run_isolated
from test_wavemu import env


def check_ms(kind, mode, min_reads, n_groups, seed, kw=None):
    mc.check_ms_batch(kind, mode, min_reads, n_groups, seed, "device", False, kw)


def check_crafted(kind):
    mc.check_crafted(kind, "device", False)


def check_plain(kind):
    mc.check_plain_counts_nothing(kind, "device", False)


@pytest.mark.parametrize("mode", [1, 2], ids=["em_seq", "taps"])
def test_simplex_clipped_families_in_the_emulated_kernels(mode):
    """300 groups, half of them soft-clipped: fragments of both orientations, pairs, overlapping pairs (both mates clipped, MC with S ops), depth 1 .. 7."""
    run_isolated("test_wavemu_methylation_clips", "check_ms", 0, mode, 1, 300, 80 + mode, env=env(), timeout=1500)


def test_simplex_clipped_families_under_max_reads():
    run_isolated("test_wavemu_methylation_clips", "check_ms", 0, 1, 1, 300, 83, dict(max_reads=3), env=env(), timeout=1500)


@pytest.mark.parametrize("min_reads", [(1, 1, 0), (3, 2, 1)], ids=["min_1_1_0", "min_3_2_1"])
def test_duplex_clipped_molecules_in_the_emulated_kernels(min_reads):
    """300 molecules, half of them with soft clips on the forward AND the reverse reads of both strands, every MC the mate's real CIGAR."""
    run_isolated("test_wavemu_methylation_clips", "check_ms", 1, 1, min_reads, 300, 85, env=env(), timeout=1500)


def test_duplex_clipped_molecules_taps():
    run_isolated("test_wavemu_methylation_clips", "check_ms", 1, 2, (1, 1, 0), 300, 86, env=env(), timeout=1500)


def test_crafted_simplex_families():
    """`4S36M` forward and `3H2S30M5S1H` reverse (T != l_seq) with the cu / ct positions worked out by hand; the LAST longest read the only clipped / the
    only plain one; lookups past the contig's ends; a pair of two clipped overlapping mates; depth 1; seven ops through = / X."""
    run_isolated("test_wavemu_methylation_clips", "check_crafted", 0, env=env(), timeout=900)


def test_crafted_duplex_molecules():
    """A clipped (and hard-clipped) reverse anchor on the AB strand, and on a BA-only molecule."""
    run_isolated("test_wavemu_methylation_clips", "check_crafted", 1, env=env(), timeout=900)


@pytest.mark.parametrize("kind", [0, 1], ids=["simplex", "duplex"])
def test_plain_groups_count_no_clipped_family(kind):
    run_isolated("test_wavemu_methylation_clips", "check_plain", kind, env=env(), timeout=900)
