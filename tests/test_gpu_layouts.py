"""GPU: the device kernels on real-world record layouts (tests/layouts.py) over backgrounds that pick each head of the launch chain, through
both entries against the oracle, with tensors in HBM (tests/layout_runs.py).  Each case runs in a child process with a time limit: these
are paths that had not run on hardware.  The routes each batch took are asserted (layout_runs.assert_route) and printed."""
import pytest

from isolated import run_isolated

pytestmark = pytest.mark.gpu

ALL = ["plain", "illumina", "window_edges", "all_types", "duplicates", "long_values", "huge_record", "clipped"]
# families per batch: 20 000 where the head depends on the batch's size or means, fewer where it does not (huge_record: 66 kB per family)
HEADS = {"seg4": 20000, "packed": 20000, "pair": 20000, "deep": 1500, "trim": 5000, "wave2": 5000, "meth": 1500, "duplex": 5000, "codec": 5000}


@pytest.mark.parametrize("head", list(HEADS))
def test_layouts_on_the_gpu(head):
    env = {"FGX_SPLIT": "0"} if head == "wave2" else {}
    big = [x for x in ALL if x != "huge_record"]
    run_isolated("layout_runs", "check_layouts", head, HEADS[head], big, "device", env=env, timeout=600)
    run_isolated("layout_runs", "check_layouts", head, 300, ["huge_record"], "device", env=env, timeout=300)


def test_mi_at_the_name_limit_is_refused():
    """prefix_len + 1 + len(MI) = 255: the consensus name does not fit BAM's 255-byte read name — the reference refuses the batch, so
    must both entries."""
    run_isolated("layout_runs", "check_long_mi_refused", "device", timeout=300)


def test_build_choice_sample_stays_in_the_first_chunk():
    run_isolated("layout_runs", "check_sample_build", 200, "device", env={"FGX_SPLIT_CHUNKS": "8"}, timeout=300)


def test_guard_bands_on_huge_records_all_types_and_hostile_deep_families():
    """FGX_GUARD_BAND=4096: every device buffer between sentinel bands, checked after each batch."""
    env = {"FGX_GUARD_BAND": "4096"}
    run_isolated("layout_runs", "check_guarded", "device", env=env, timeout=600)


def test_illumina_layout_bam_files_at_levels_6_and_0(tmp_path):
    """The file path: find_z_tag_wide (grouping.hip) on 120 - 200-byte aux blocks, device inflate on blocks that are not level 1."""
    run_isolated("layout_runs", "check_file_path", str(tmp_path), timeout=600)
