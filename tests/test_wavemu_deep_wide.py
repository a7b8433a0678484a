"""FGX_DEEP_WIDE=1: the wide kernels (k_wide_parse, k_wide_cols, k_wide_finish — fgumi_amd/csrc/simplex_wide.inc) behind the streaming kernels of deep simplex
families, executed on the CPU in 64-lane lock-step (tests/wavemu — a cross-lane operation or a barrier under divergent control flow faults there).  Each batch
of tests/wide_cases.py goes through fgx_process_batch_device of the emulation library against the oracle: bytes, count and all 28 counters equal, nothing
deferred, and every family on the path it was built for (fgx_debug_last_wide_families / fgx_debug_last_deep_families).  Two or three families per case: a
case takes what the 520 - 700-record case of tests/test_wavemu_max_reads.py takes."""
import os

import pytest

from isolated import run_isolated
from test_wavemu import env

ON = dict(FGX_DEEP_WIDE=1)


def check_case(name, *args):
    import wide_cases as W
    case = getattr(W, name)(*args)
    want = W.check_on(case)
    if case.opts.get("max_reads") is not None:
        assert int(want["stats"][3 + W.REJ_DOWNSAMPLED]) > 0                  # the comparison is not empty: the oracle dropped reads


def check_umi_of_unequal_length():
    """Not miscalled: the device entry defers the family (and decides the one beside it); the oracle refuses such a family, and so does the host entry."""
    import wide_cases as W
    case = W.umi_of_unequal_length()
    with pytest.raises(RuntimeError, match="same length"):
        W.want_of(case)
    c = W.Caller()
    try:
        got = c.device(case.g)
        assert got["deferred"] == 1 and got["wide"] == 1 and got["deep"] == 0, got
        with pytest.raises(AssertionError, match="UMIs of unequal length"):
            c.host(case.g)
    finally:
        c.close()


def check_switch_off(value):
    """(child interpreter; FGX_DEEP_WIDE as the test set it, "unset": not in the environment) the library as it was: every such family deferred, the host entry the oracle's bytes."""
    import wide_cases as W
    if value == "unset":
        assert "FGX_DEEP_WIDE" not in os.environ
    else:
        assert os.environ["FGX_DEEP_WIDE"] == value
    W.check_off(W.up_to_1024_records(2))


def check_switch_is_read_per_call():
    import wide_cases as W
    case = W.up_to_1024_records(2)
    want = W.want_of(case)
    c = W.Caller()
    try:
        for value, on in (("1", True), ("0", False), ("yes", True), ("", False)):
            os.environ["FGX_DEEP_WIDE"] = value
            got = c.device(case.g)
            if on:
                assert got["wide"] == 2 and got["deferred"] == 0, (value, got)
                W.assert_equal(got, want, "device entry")
            else:
                assert got["wide"] == 0 and got["deferred"] == 2, (value, got)
    finally:
        c.close()


@pytest.mark.parametrize("err", [5000, 0])
def test_255_pairs_stay_with_the_streaming_kernels_and_256_are_wide(err):
    run_isolated("test_wavemu_deep_wide", "check_case", "byte_edge", err, env=env(**ON), timeout=1500)


@pytest.mark.parametrize("cap", [100, 400])
def test_more_than_1024_records_under_a_cap(cap):
    """About 1 100 records per family: above DEEP_CAP_MAX; after the cut an end keeps 100 (at most 255) or 400 (more) reads."""
    run_isolated("test_wavemu_deep_wide", "check_case", "capped", cap, 2, (550, 560), env=env(**ON), timeout=1500)


def test_equal_ranks_at_the_cut():
    run_isolated("test_wavemu_deep_wide", "check_case", "capped", 100, 2, (550, 560), True, env=env(**ON), timeout=1500)


def test_min_reads_3_on_read_through_inserts():
    run_isolated("test_wavemu_deep_wide", "check_case", "read_through", 2, env=env(**ON), timeout=1500)


def test_umi_characters_with_more_than_255_observations():
    run_isolated("test_wavemu_deep_wide", "check_case", "umi_disagreement", env=env(**ON), timeout=1500)


def test_umi_of_unequal_length_is_deferred():
    run_isolated("test_wavemu_deep_wide", "check_umi_of_unequal_length", env=env(**ON), timeout=1500)


@pytest.mark.parametrize("value", ["unset", "0", ""])
def test_switch_off(value):
    run_isolated("test_wavemu_deep_wide", "check_switch_off", value, env=env(**({} if value == "unset" else dict(FGX_DEEP_WIDE=value))), timeout=1500)


def test_switch_on_takes_the_wide_path():
    run_isolated("test_wavemu_deep_wide", "check_case", "up_to_1024_records", 2, env=env(**ON), timeout=1500)


def test_switch_is_read_per_call():
    run_isolated("test_wavemu_deep_wide", "check_switch_is_read_per_call", env=env(), timeout=1500)


def check_the_bound():
    """A family of exactly WIDE_MAX records is decided (the oracle's bytes for it); one of WIDE_MAX + 2 beside it leaves as before and is deferred."""
    import wide_cases as W
    from fgumi_amd import GroupedReads
    case = W.the_bound()
    want_first = W.want_of(W.Case(GroupedReads.from_groups([case.g.records(0)]), 1, 0))
    c = W.Caller()
    try:
        got = c.device(case.g)
        assert got["deferred"] == 1 and got["wide"] == 1 and got["deep"] == 0, {k: got[k] for k in ("big", "deep", "wide", "deferred")}
        assert got["data"] == want_first["data"] and got["count"] == want_first["count"]
    finally:
        c.close()


def test_the_bound():
    run_isolated("test_wavemu_deep_wide", "check_the_bound", env=env(**ON), timeout=1500)
