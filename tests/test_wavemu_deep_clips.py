"""FGX_DEEP_CLIPS=1: deep simplex families and deep duplex molecules with soft- / hard-clipped reads decided by the clip-taking builds of the streaming record
kernels (k_deep_parse<.., .., 1> in plain mode, k_duplex_deep_parse<.., .., .., 1>), executed on the CPU in 64-lane lock-step (tests/wavemu — a cross-lane
operation or a barrier under divergent control flow faults there).  Each batch of tests/deep_clip_cases.py goes through fgx_process_batch_device and
fgx_process_batch of the emulation library against the oracle: bytes, count and all 28 counters equal, and the path of the device batch — the deferred count,
the groups the streaming kernels decided and fgx_debug_last_deep_clipped.  Every case runs in a child interpreter.  Without the feature the library has no
fgx_debug_last_deep_clipped and such groups are deferred (or k_family's)."""
import pytest

import deep_clip_cases as K
from isolated import run_isolated
from test_wavemu import env

T = 900
M = "deep_clip_cases"


# ---- duplex ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_soft_clip_molecule_of_the_existing_tests_is_decided():
    run_isolated(M, "check_case", "soft_clip_of_the_existing_tests", env=env(), timeout=T)


@pytest.mark.parametrize("what", ["deletion", "secondary"])
def test_deletion_and_secondary_records_are_still_deferred(what):
    run_isolated(M, "check_case", "still_deferred", what, env=env(), timeout=T)


@pytest.mark.parametrize("n_records", [64, 66, 128, 130, 510, 512])
def test_sizes_with_a_clipped_read_in_each_of_the_four_sets(n_records):
    """64: the wavefront kernel and the canonical pass, nothing of this path; 66 / 128 / 130: the edge between the two builds; 510: decided; 512 with 256 reads
    on a side: deferred for the bound, and the molecule beside it decided."""
    run_isolated(M, "check_size", n_records, env=env(), timeout=T)


@pytest.mark.parametrize("shape", K.TAKEN_SHAPES)
def test_clip_shapes_taken(shape):
    run_isolated(M, "check_case", "shaped", shape, env=env(), timeout=T)


@pytest.mark.parametrize("shape", K.DEFERRED_SHAPES)
def test_clip_shapes_deferred(shape):
    """17 ops, a CIGAR of S only, an MC of 9 ops."""
    run_isolated(M, "check_case", "shaped", shape, env=env(), timeout=T)


def test_overlap_with_leading_clips():
    run_isolated(M, "check_overlap_with_leading_clips", env=env(), timeout=T)


def test_aligned_blocks_apart_although_the_reads_are_not():
    run_isolated(M, "check_blocks_apart", env=env(), timeout=T)


def test_read_through_with_soft_clipped_adapters():
    run_isolated(M, "check_read_through", env=env(), timeout=T)


@pytest.mark.parametrize("name", list(K.OPTION_MATRIX))
def test_option_matrix(name):
    run_isolated(M, "check_case", "option_case", name, env=env(), timeout=T)


def test_strand_cap_with_clipped_reads_among_scoring_and_dropped_reads():
    run_isolated(M, "check_strand_cap", env=env(), timeout=T)


def test_mixed_stream():
    run_isolated(M, "check_case", "mixed_stream", env=env(), timeout=T)


@pytest.mark.parametrize("what", ["trim", "rejects", "methylation"])
def test_options_that_keep_the_duplex_path_off(what):
    run_isolated(M, "check_path_off", what, env=env(), timeout=T)


def test_switch_unset_defers_as_before():
    run_isolated(M, "check_switch_unset", env=env(), timeout=T)


@pytest.mark.parametrize("what", ["shallow", "pairs"])
def test_unchanged_chain(what):
    run_isolated(M, "check_unchanged_chain", what, env=env(), timeout=T)


# ---- simplex, plain mode ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_simplex_sizes(layout):
    run_isolated(M, "check_case", "simplex_sizes", layout, env=env(), timeout=T)


@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_simplex_sizes_with_the_switch_unset(layout):
    run_isolated(M, "check_case", "simplex_sizes_unset", layout, env=env(), timeout=T)


def test_a_family_of_700_records_under_max_reads():
    run_isolated(M, "check_case", "under_max_reads", env=env(), timeout=T)


def test_clipped_r1_with_unmapped_r2():
    run_isolated(M, "check_case", "clipped_r1_unmapped_r2", env=env(), timeout=T)


def test_an_end_of_mapped_and_unmapped_reads_is_handed_on():
    run_isolated(M, "check_case", "mixed_end_beside_a_clipped_read", env=env(), timeout=T)


@pytest.mark.parametrize("n_records", [100, 200])
def test_a_clipped_read_beside_a_deletion_read(n_records):
    """100 records: k_family; 200: the deferred list — as today."""
    run_isolated(M, "check_case", "clip_beside_deletion", n_records, env=env(), timeout=T)


def test_methylation_mode_is_untouched_by_the_switch():
    run_isolated(M, "check_methylation_mode", env=env(), timeout=T)
