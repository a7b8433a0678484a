"""GPU: the MI-grouping kernels of grouping.hip (tag walk, keep decision, compaction over the scans, group bounds) on the streams of
tests/grouping_cases.py, through fgx_group_records (host buffers) and fgx_group_records_device (tensors in HBM), against the oracle — which is
first held to each crafted case's hand-written answer.  Each check runs in a child process with a time limit: walks over malformed aux blocks
and over the blob's last bytes had not run on hardware."""
import pytest

import layouts
from grouping_cases import SIZES
from isolated import run_isolated

pytestmark = pytest.mark.gpu


def test_tag_walk_key_compare_suffix_tab_and_flag_cases():
    """Case set A: MI behind every aux type, wrong types and duplicates, malformed entries, the same at the blob's end, keys of 0 .. 300 bytes
    that differ in one place, extract_mi_base, keys equal only as MI + '\\t' + cell, every flag combination."""
    run_isolated("grouping_cases", "check_tag_walk", "device", timeout=120)


def test_drops_and_groups_across_blocks_and_scan_tiles_small_streams():
    """Case set B below 70 000 records: 1 .. 513 records, every drop pattern on every group shape."""
    run_isolated("grouping_cases", "check_scans", [n for n in SIZES if n < 70000], "device", timeout=120)


def test_drops_and_groups_across_blocks_and_scan_tiles_70000_records():
    run_isolated("grouping_cases", "check_scans", [n for n in SIZES if n >= 70000], "device", timeout=120)


def test_scratch_reuse_between_calls_of_different_sizes():
    run_isolated("grouping_cases", "check_scratch_reuse", "device", timeout=120)


@pytest.mark.parametrize("layout", list(layouts.LAYOUTS))
def test_real_layouts_regroup_with_and_without_drops(layout):
    """Case set C: every record layout of tests/layouts.py as a flat stream, simplex and duplex shaped."""
    run_isolated("grouping_cases", "check_layout", layout, "device", timeout=120)


def test_regrouped_layouts_feed_the_caller():
    run_isolated("grouping_cases", "check_regrouped_layouts_feed_the_caller", timeout=120)
