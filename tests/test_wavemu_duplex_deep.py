"""Duplex molecules of more than 64 records decided by k_duplex_deep_parse + k_duplex_deep_cols (fgumi_amd/csrc/duplex_deep.inc), executed on the CPU in
64-lane lock-step (tests/wavemu — a cross-lane operation or a barrier under divergent control flow faults there).  Each batch of tests/duplex_deep_cases.py
goes through fgx_process_batch_device and fgx_process_batch of the emulation library against the oracle: bytes, count and all 28 counters equal, and the
path of the device batch — how many molecules were deferred, how many fgx_debug_last_duplex_deep counts, none counted as a simplex big / deep family.
Every case runs in a child interpreter.  Without duplex_deep.inc every such molecule is deferred and the library has no fgx_debug_last_duplex_deep."""
import os

import pytest

from isolated import run_isolated
from test_wavemu import env

T = 900


def check_case(name, *args):
    import duplex_deep_cases as D
    D.check(getattr(D, name)(*args))


def check_lower_edge():
    import duplex_deep_cases as D
    case = D.lower_edge()
    assert D.records_per_family(case.g).tolist() == [64, 66] and case.deep == 1
    D.check(case)


def check_integer_tag_types(n_pairs, ty):
    """The oracle's own cD is type `ty` (c up to 127, C above); the device bytes then equal the oracle's."""
    import duplex_deep_cases as D
    case = D.pairs(n_pairs)
    want = D.want_of(case)
    cd = D.cd_types(want["data"])
    print(f"cD of the oracle's records: {cd}", flush=True)
    assert len(cd) == 2 and all(t == ty for t, _ in cd), cd
    D.check(case, want)


def check_the_bound():
    import duplex_deep_cases as D
    from fgumi_amd import GroupedReads
    case = D.the_bound()
    want_first = D.want_of(D.Case(GroupedReads.from_groups([case.g.records(0)])))
    D.check_deferred_beside_decided(case, want_first)
    D.check(case)


def check_read_through():
    import duplex_deep_cases as D
    case = D.read_through()
    want = D.want_of(case)
    assert int(want["stats"][3 + D.REJ_ZERO_LENGTH]) > 0
    D.check(case, want)


def check_counter(name, args, counter):
    """The case, and the oracle counted reads under `counter`: the comparison is not empty."""
    import duplex_deep_cases as D
    case = getattr(D, name)(*args)
    want = D.want_of(case)
    assert int(want["stats"][3 + counter]) > 0, want["stats"].tolist()
    D.check(case, want)


def check_lone_strand_passes_through():
    import duplex_deep_cases as D
    case = D.only_a_strand((1, 1, 0))
    want = D.want_of(case)
    assert want["count"] == 2
    D.check(case, want)


def check_umi_of_unequal_length():
    """Not miscalled: the device entry defers the molecule and decides the one beside it; the oracle refuses such a molecule, and so does the host entry."""
    import duplex_deep_cases as D
    from fgumi_amd import GroupedReads
    case = D.umi_of_unequal_length()
    with pytest.raises(RuntimeError):
        D.want_of(case)
    want_second = D.want_of(D.Case(GroupedReads.from_groups([case.g.records(1)])))
    c = D.Caller()
    try:
        got = c.device(case.g)
        assert got["deferred"] == 1 and got["duplex_deep"] == 1, {k: got[k] for k in D.PATH_KEYS}
        assert got["data"] == want_second["data"] and got["count"] == want_second["count"]
        with pytest.raises(AssertionError):
            c.host(case.g)
    finally:
        c.close()


def check_path_off(what):
    import duplex_deep_cases as D
    contigs = D.methylation_contigs() if what == "methylation" else None
    case = D.path_off_case(what)
    if what != "rejects":
        D.check(case, contigs=contigs)
        return
    # --rejects: the device entry serves only batches it defers nothing of and refuses this one, as it did; the host entry decides it
    want = D.want_of(case)
    c = D.Caller(**case.opts)
    try:
        with pytest.raises(AssertionError, match="defers"):
            c.device(case.g)
        got = c.host(case.g)
        assert got["duplex_deep"] == 0 and got["big"] == 0 and got["deep"] == 0, got
        D.assert_equal(got, want, "host entry")
    finally:
        c.close()


def check_switch_off(value):
    """(child interpreter; FGX_DUPLEX_DEEP as the test set it) "0": every deep molecule deferred, the host entry the oracle's bytes; unset or "1": the path is on."""
    import duplex_deep_cases as D
    if value == "unset":
        assert "FGX_DUPLEX_DEEP" not in os.environ
    else:
        assert os.environ["FGX_DUPLEX_DEEP"] == value
    case = D.pairs(40, 2)
    if value == "0":
        case = D.Case(case.g, deferred=2)
        assert case.deep == 0
    D.check(case)


def check_switch_is_read_per_call():
    import duplex_deep_cases as D
    case = D.pairs(40, 2)
    want = D.want_of(case)
    c = D.Caller()
    try:
        for value, on in (("1", True), ("0", False), (None, True), ("0", False), ("1", True)):
            if value is None:
                os.environ.pop("FGX_DUPLEX_DEEP", None)
            else:
                os.environ["FGX_DUPLEX_DEEP"] = value
            got = c.device(case.g)
            if on:
                assert got["duplex_deep"] == 2 and got["deferred"] == 0, (value, got)
                D.assert_equal(got, want, "device entry")
            else:
                assert got["duplex_deep"] == 0 and got["deferred"] == 2, (value, got)
    finally:
        c.close()


def check_unchanged_chain():
    """A batch without a deep molecule: the same kernel launches, the same host synchronisations and the same bytes with the switch on and off."""
    import duplex_deep_cases as D
    case = D.shallow()
    want = D.want_of(case)
    c = D.Caller()
    try:
        seen = {}
        c.device(case.g)                                           # (a caller's first batch uploads its table images: not part of the comparison)
        for value in ("1", "0"):
            os.environ["FGX_DUPLEX_DEEP"] = value
            got = c.device(case.g)
            assert got["deferred"] == 0 and got["duplex_deep"] == 0
            D.assert_equal(got, want, f"device entry, switch {value}")
            seen[value] = c.chain()
        print(f"(launches, host synchronisations): {seen}", flush=True)
        assert seen["1"] == seen["0"] and seen["1"][0] > 0, seen
    finally:
        c.close()


def test_32_pairs_stay_with_the_wavefront_kernel_and_33_are_deep():
    run_isolated("test_wavemu_duplex_deep", "check_lower_edge", env=env(), timeout=T)


@pytest.mark.parametrize("n_pairs,ty", [(127, "c"), (128, "C"), (255, "C")])
def test_integer_tag_types(n_pairs, ty):
    run_isolated("test_wavemu_duplex_deep", "check_integer_tag_types", n_pairs, ty, env=env(), timeout=T)


def test_the_bound():
    run_isolated("test_wavemu_duplex_deep", "check_the_bound", env=env(), timeout=T)


@pytest.mark.parametrize("err", [0, 20000])
def test_error_rates(err):
    """0: unanimous columns far above the cap depth; 20 000: many columns and UMI characters through k_call_full."""
    run_isolated("test_wavemu_duplex_deep", "check_case", "pairs", 100, 2, err, env=env(), timeout=T)


@pytest.mark.parametrize("name", ["min_reads_3_2_1", "min_reads_2_1_0", "min_reads_6_3_3", "overlapping_off", "per_base_tags_off", "min_input_base_quality_30",
                                  "error_rates_30_25", "tie_rule_1", "long_prefix", "reads_of_300_bases"])
def test_option_matrix_on_a_long_tail(name):
    run_isolated("test_wavemu_duplex_deep", "check_case", "option_case", name, env=env(), timeout=T)


def test_read_through_inserts_with_masked_input():
    run_isolated("test_wavemu_duplex_deep", "check_read_through", env=env(), timeout=T)


def test_lone_strand_is_passed_through():
    run_isolated("test_wavemu_duplex_deep", "check_lone_strand_passes_through", env=env(), timeout=T)


def test_lone_strand_is_rejected_under_1_1_1():
    import duplex_deep_cases as D
    run_isolated("test_wavemu_duplex_deep", "check_counter", "only_a_strand", ((1, 1, 1),), D.REJ_INSUFFICIENT_READS, env=env(), timeout=T)


def test_single_read_sets():
    run_isolated("test_wavemu_duplex_deep", "check_case", "single_read_sets", env=env(), timeout=T)


def test_stray_fragment_records():
    import duplex_deep_cases as D
    run_isolated("test_wavemu_duplex_deep", "check_counter", "stray_fragments", (), D.REJ_FRAGMENT_READ, env=env(), timeout=T)


def test_strand_collision():
    import duplex_deep_cases as D
    run_isolated("test_wavemu_duplex_deep", "check_counter", "strand_collision", (), D.REJ_POTENTIAL_COLLISION, env=env(), timeout=T)


def test_r1_only_molecule():
    run_isolated("test_wavemu_duplex_deep", "check_case", "r1_only", env=env(), timeout=T)


@pytest.mark.parametrize("name", ["umi_disagreement", "paired_umi", "no_rx"])
def test_umis(name):
    run_isolated("test_wavemu_duplex_deep", "check_case", name, env=env(), timeout=T)


def test_umi_of_unequal_length_is_deferred():
    run_isolated("test_wavemu_duplex_deep", "check_umi_of_unequal_length", env=env(), timeout=T)


@pytest.mark.parametrize("what", ["deletion", "soft_clip", "secondary"])
def test_not_this_paths(what):
    run_isolated("test_wavemu_duplex_deep", "check_case", "not_this_path", what, env=env(), timeout=T)


@pytest.mark.parametrize("what", ["trim", "rejects", "cap", "methylation"])
def test_options_that_keep_the_path_off(what):
    run_isolated("test_wavemu_duplex_deep", "check_path_off", what, env=env(), timeout=T)


@pytest.mark.parametrize("value", ["unset", "1", "0"])
def test_switch(value):
    run_isolated("test_wavemu_duplex_deep", "check_switch_off", value, env=env(**({} if value == "unset" else dict(FGX_DUPLEX_DEEP=value))), timeout=T)


def test_switch_is_read_per_call():
    run_isolated("test_wavemu_duplex_deep", "check_switch_is_read_per_call", env=env(), timeout=T)


def test_unchanged_chain_without_a_deep_molecule():
    run_isolated("test_wavemu_duplex_deep", "check_unchanged_chain", env=env(), timeout=T)


def test_mixed_stream_device_entry():
    run_isolated("test_wavemu_duplex_deep", "check_case", "mixed_stream", env=env(), timeout=T)
