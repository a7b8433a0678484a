"""The device kernels on real-world record layouts and hostile groups, in the wave-level emulator (tests/wavemu: the real launch chain and
kernel sources, 64 lanes in lock-step on the CPU): tests/layouts.py's layouts over backgrounds that pick each head of the chain, and the
general-path fuzz's hostile groups spliced into them, through both entries against the oracle (tests/layout_runs.py).  The small version of
tests/test_gpu_layouts.py and tests/test_gpu_hostile.py, where failures are debugged without a GPU.

Not here (the emulator's lock-step model rejects what the hardware runs): k_family_wave<0>'s column loop reads lanes under a lane-divergent
loop bound, so --trim and the records that reach it (soft clips on the split heads, 44-character names of a long-tail batch); the hostile
groups of a depth-3 batch, which desynchronise k_simplex_seg<4>'s per-family cross-lane reads.  The GPU tests run those."""
import pytest

from isolated import run_isolated
from test_wavemu import env

ALL = ["plain", "illumina", "window_edges", "all_types", "duplicates", "long_values", "huge_record", "clipped"]
CASES = {
    "seg4": ALL[:-1],
    "packed": ALL[:-1],
    "pair": ["plain", "illumina", "all_types", "duplicates", "long_values", "huge_record"],
    "deep": ALL,
    "wave2": ALL[:-1],
    "meth": ALL,
    "duplex": ALL,
    "codec": ALL,
}


@pytest.mark.parametrize("head", list(CASES))
def test_layouts_through_the_emulated_kernels(head):
    e = env(**({"FGX_SPLIT": 0} if head == "wave2" else {}))
    run_isolated("layout_runs", "check_layouts", head, 300, CASES[head], env=e, timeout=900)


@pytest.mark.parametrize("head", ["packed", "pair", "deep", "duplex", "codec"])
def test_hostile_groups_through_the_emulated_kernels(head):
    # (fixed seeds: a simplex seed whose hostile groups reach k_family_wave<0> cannot run in the emulator, see above)
    seeds = [7002, 7003, 7004] if head in ("packed", "pair", "deep") else [7001, 7002, 7003, 7004]
    # (CODEC: most hostile molecules are outside the canonical form's scope and go to the host; a smaller share is stated)
    run_isolated("layout_runs", "check_hostile", head, 300, seeds, 10, "host", None, 0.05 if head == "codec" else 0.25, env=env(), timeout=900)


def test_hostile_groups_at_the_chunk_boundaries():
    """FGX_SPLIT_CHUNKS=4 over 400 depth-8 families: hostile groups on both sides of every chunk boundary (placed by the product's chunk
    geometry, asserted in layout_runs.check)."""
    run_isolated("layout_runs", "check_hostile", "packed", 400, [7002, 7004], 14, "host", 4, env=env(FGX_SPLIT_CHUNKS=4), timeout=900)


def test_hostile_records_inside_deep_families():
    """Record 0 secondary or unmapped, a dropped mate, all-Q2 reads, a foreign MC inside families of 70 - 120 records: k_deep_parse /
    k_deep_sizes / k_deep_cols and the --rejects side kernels against the oracle."""
    run_isolated("layout_runs", "check_hostile_deep", 120, [7101, 7102], env=env(), timeout=900)


def test_build_choice_sample_stays_in_the_first_chunk():
    run_isolated("layout_runs", "check_sample_build", env=env(FGX_SPLIT_CHUNKS=8), timeout=900)
