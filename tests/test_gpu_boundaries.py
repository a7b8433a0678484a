"""GPU: the FindBoundaries kernels of boundaries.hip (a guess per 16 KiB segment, the walks, the mutual check with its repair rounds) on the streams of
tests/boundary_cases.py, through fgx_record_boundaries_device with the stream in a tensor of exactly its length: offsets, lengths, `consumed` and the return
code against each case's constructed answer (which the sequential walk confirms first), and the repair rounds of every call, read through
fgx_debug_last_boundary_rounds — none where no decoy stands, at least one where a decoy takes a segment, never more than segments + 1.  On the host build
(tests/test_apiemu.py) the threads of k_bound_check run in segment order; here a true predecessor and a decoy segment race for the same table entries.
Each group runs in a child process with a time limit."""
import pytest

from isolated import run_isolated

pytestmark = pytest.mark.gpu


def test_segment_geometry_needs_no_repair():
    """Group A: records that end on and start around segment edges, streams of 0 .. 40 bytes, start offsets, segments without a record start."""
    run_isolated("boundary_cases", "check", "A", "device", timeout=120)


def test_decoy_chains_cost_repair_rounds_and_nothing_else():
    """B1 .. B6 and B8: fake chains in front of 70 segments' first records, 600 fake records in one carrier (whole and cut), a far jump, a terminal link, a
    malformed fake link (no error), malformed true records (the error), a fake walk that ends on a true record."""
    run_isolated("boundary_cases", "check", "B", "device", timeout=120)


def test_repairs_across_the_thread_block_edge():
    """B7: 281 segments; a far jump out of segment 250 wipes 251 .. 262, decoys in 255, 256, 257."""
    run_isolated("boundary_cases", "check", "B7", "device", timeout=120)


def test_contract_and_scratch_reuse():
    """C: cap == n_rec, cap > n_rec, cap too small, cap = 0 over poisoned arrays; D: every case on one caller, shuffled, the longest table in front of the shortest."""
    run_isolated("boundary_cases", "check", "CD", "device", timeout=120)
