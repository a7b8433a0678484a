"""GPU parity under FGX_DEEP_CLIPS=1: deep simplex families and deep duplex molecules with soft- / hard-clipped reads decided by the clip-taking builds of the
streaming record kernels (k_deep_parse<.., .., 1> in plain mode, k_duplex_deep_parse<.., .., .., 1>).  Each test compares both entries with the oracle byte
for byte, count and all 28 counters included, and asserts the path of the device batch: the deferred count, the groups the streaming kernels decided and
fgx_debug_last_deep_clipped.  The batches are those of tests/deep_clip_cases.py (a handful of groups each).  Without the feature the library has no
fgx_debug_last_deep_clipped and such groups are deferred (or k_family's)."""
import pytest

import deep_clip_cases as K
from isolated import run_isolated

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def switches_unset(monkeypatch):
    for k in K.SWITCHES + ("FGX_DUPLEX_DEEP", "FGX_DEEP"):
        monkeypatch.delenv(k, raising=False)


# ---- duplex ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_soft_clip_molecule_of_the_existing_tests_is_decided():
    K.check_case("soft_clip_of_the_existing_tests")


@pytest.mark.parametrize("what", ["deletion", "secondary"])
def test_deletion_and_secondary_records_are_still_deferred(what):
    K.check_case("still_deferred", what)


@pytest.mark.parametrize("n_records", [64, 66, 128, 130, 510, 512])
def test_sizes_with_a_clipped_read_in_each_of_the_four_sets(n_records):
    """64: the wavefront kernel and the canonical pass, nothing of this path; 66 / 128 / 130: the edge between the two builds; 510: decided; 512 with 256 reads
    on a side: deferred for the bound, and the molecule beside it decided."""
    K.check_size(n_records)


@pytest.mark.parametrize("shape", K.TAKEN_SHAPES)
def test_clip_shapes_taken(shape):
    K.check_case("shaped", shape)


@pytest.mark.parametrize("shape", K.DEFERRED_SHAPES)
def test_clip_shapes_deferred(shape):
    """17 ops, a CIGAR of S only, an MC of 9 ops."""
    K.check_case("shaped", shape)


def test_overlap_with_leading_clips():
    K.check_overlap_with_leading_clips()


def test_aligned_blocks_apart_although_the_reads_are_not():
    K.check_blocks_apart()


def test_read_through_with_soft_clipped_adapters():
    K.check_read_through()


@pytest.mark.parametrize("name", list(K.OPTION_MATRIX))
def test_option_matrix(name):
    K.check_case("option_case", name)


def test_strand_cap_with_clipped_reads_among_scoring_and_dropped_reads():
    K.check_strand_cap()


def test_mixed_stream():
    K.check_case("mixed_stream")


@pytest.mark.parametrize("what", ["trim", "rejects", "methylation"])
def test_options_that_keep_the_duplex_path_off(what):
    K.check_path_off(what)


def test_switch_unset_defers_as_before():
    K.check_switch_unset()


@pytest.mark.parametrize("what", ["shallow", "pairs"])
def test_unchanged_chain(what):
    K.check_unchanged_chain(what)


# ---- simplex, plain mode ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_simplex_sizes(layout):
    K.check_case("simplex_sizes", layout)


@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_simplex_sizes_with_the_switch_unset(layout):
    K.check_case("simplex_sizes_unset", layout)


def test_a_family_of_700_records_under_max_reads():
    K.check_case("under_max_reads")


def test_clipped_r1_with_unmapped_r2():
    K.check_case("clipped_r1_unmapped_r2")


def test_an_end_of_mapped_and_unmapped_reads_is_handed_on():
    K.check_case("mixed_end_beside_a_clipped_read")


@pytest.mark.parametrize("n_records", [100, 200])
def test_a_clipped_read_beside_a_deletion_read(n_records):
    """100 records: k_family; 200: the deferred list — as today."""
    K.check_case("clip_beside_deletion", n_records)


def test_methylation_mode_is_untouched_by_the_switch():
    K.check_methylation_mode()


def check_under_guard_bands():
    """(child interpreter, FGX_GUARD_BAND set) a duplex and a simplex batch through the clip builds, then a look at every guarded buffer."""
    import ctypes as C
    from fgumi_amd import lib
    lib.fgx_debug_check_guard_bands.restype = C.c_int
    lib.fgx_debug_check_guard_bands.argtypes = [C.c_char_p, C.c_int]
    K.check_case("option_case", "min_reads_3_2_1")
    K.check_case("simplex_sizes", "pair_overlap")
    msg = C.create_string_buffer(600)
    bad = lib.fgx_debug_check_guard_bands(msg, 600)
    assert bad == 0, f"clip builds: {bad} device buffer(s) written outside their bounds: {msg.value.decode()}"


def test_under_guard_bands():
    run_isolated("test_gpu_deep_clips", "check_under_guard_bands", env={"FGX_GUARD_BAND": "4096"}, timeout=300)
