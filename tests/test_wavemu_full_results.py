"""k_call_full's result array (fgumi_amd/csrc/fastpath.h, FullResult) under the wave-level host emulator: one batch per case through
fgx_process_batch_device — bytes and the 28 counters against the oracle — and then the path the answers took (fgx_debug_last_full_results).
Cases and checks: tests/full_results_cases.py.

What the emulator showed when the cases were written (300 depth-8 families of 2 x 150 bases): the packed build takes all 300, the writer applies all
300 (share 1.000), 989 column answers (3.3 per family) go through the array and none is scattered.  Families of 8- and 9-base reads are not the
packed build's (every answer scattered, bytes equal); at 5 % errors a family holds ~90 items, more than the 64 results a wavefront loads, and 185
of 200 families are refused — a counter of its own, apart from the families whose range a list's end cuts."""
import pytest

from isolated import run_isolated
from test_wavemu import env

CASES = {
    "a_defaults": 300,            # 8 pairs x 150 bp: at least 90 % of the families applied, nothing of an applied family scattered
    "b_length_8": 200, "b_length_9": 200, "b_length_147": 200, "b_length_149": 200, "b_length_151": 200, "b_length_255": 150, "b_length_256": 150,
    "c_noisy_2pct": 200,          # ~40 items per family: column 0, column Lc - 1, the zone the last two lanes of a half both hold
    "c_noisy_5pct": 200,          # ~90 items per family: most families refused (more than 64 results: the counter of its own), the rest applied
    "d_length_257": 100,          # emit_pair refuses the pair: nothing applied, everything scattered
    "d_fragments": 60,            # single-end families: emit_load / emit_store read the planes
    "e_long_tail": 300,           # 2 .. 50 pairs: two items per column with continuation items; the classic builds' and the streaming kernels' items are scattered
    "f_min_reads_3": 300,         # N / quality 0 below --min-reads
    "f_min_quality_40": 200,      # N / quality 2 below --min-consensus-base-quality
}


@pytest.mark.parametrize("name", list(CASES))
def test_result_array_under_the_emulator(name):
    run_isolated("full_results_cases", "check_emulated", name, CASES[name], env=env(FGX_FULL_RESULTS=1), timeout=900)


def test_switched_off_everything_is_scattered():
    """FGX_FULL_RESULTS=0: no answer goes through the array, no family is applied — same bytes."""
    run_isolated("full_results_cases", "check_emulated", "g_switched_off", 200, env=env(FGX_FULL_RESULTS=0), timeout=900)


def test_variable_unset_is_the_default():
    """FGX_FULL_RESULTS not set: what full_results_cases.DEFAULT_ON says — everything through the array for the applied families, or nothing at all."""
    e = env()
    assert "FGX_FULL_RESULTS" not in e
    run_isolated("full_results_cases", "check_emulated", "g_unset", 200, env=e, timeout=900)


def test_ranges_cut_at_a_lists_end():
    """Lists of 8 slots (FGX_POOL_SLACK=8 on a pool of 1 / 2^20 of the column bound): four families of a workgroup bring ~13 items to one list, so ranges
    cross list ends.  Those families are refused as "not in one piece" and scattered, their neighbours are applied — same bytes."""
    run_isolated("full_results_cases", "check_emulated", "h_cut_ranges", 300, env=env(FGX_FULL_RESULTS=1, FGX_POOL_DIV=1 << 20, FGX_POOL_SLACK=8), timeout=900)


def test_in_one_piece_rule():
    """The decision itself (full_range_whole), as the host-callable export of the emulation library."""
    run_isolated("full_results_cases", "check_whole_rule", env=env(), timeout=300)
