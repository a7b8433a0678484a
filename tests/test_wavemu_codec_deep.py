"""CODEC molecules of more than 64 records decided by k_codec_deep_parse + k_codec_deep_cols (fgumi_amd/csrc/codec_deep.inc), executed on the CPU in
64-lane lock-step (tests/wavemu — a cross-lane operation or a barrier under divergent control flow faults there).  Each batch of tests/codec_deep_cases.py
goes through fgx_process_batch_device and fgx_process_batch of the emulation library against the oracle: bytes, count and all 28 counters equal, and the
path of the device batch — exactly how many molecules were deferred, how many fgx_debug_last_codec_deep and fgx_debug_last_codec_deep_capped count, none
counted as a simplex big / deep family or a deep duplex molecule.  Every case runs in a child interpreter, under FGX_CODEC_DEEP=1 unless the test is about
the switch.  Without codec_deep.inc the library has no fgx_debug_last_codec_deep and every such molecule is deferred."""
import os

import pytest

from isolated import run_isolated
from test_wavemu import env

T = 900
ME = "test_wavemu_codec_deep"


def on(**more):
    return env(FGX_CODEC_DEEP=1, **more)


def check_case(name, *args):
    import codec_deep_cases as D
    D.check(getattr(D, name)(*args))


def check_counter(name, args, counter):
    """The case, and the oracle counted reads under `counter`: the comparison is not empty."""
    import codec_deep_cases as D
    case = getattr(D, name)(*args)
    want = D.want_of(case)
    assert int(want["stats"][3 + counter]) > 0, want["stats"].tolist()
    D.check(case, want)


def check_lower_edge():
    import codec_deep_cases as D
    case = D.lower_edge()
    assert D.records_per_family(case.g).tolist() == [64, 66] and case.deep == 1
    D.check(case)


def check_integer_tag_types(n_pairs, ty):
    """The oracle's own cD is type `ty` (c up to 127, C above) — so some position is covered by both strands —; the device bytes then equal the oracle's."""
    import codec_deep_cases as D
    case = D.pairs(n_pairs)
    want = D.want_of(case)
    cd = D.cd_types(want["data"])
    print(f"cD of the oracle's record: {cd}", flush=True)
    assert len(cd) == 1 and cd[0] == (ty, 2 * n_pairs), (cd, "no position is covered by both strands" if cd and cd[0][1] <= n_pairs else "")
    D.check(case, want)


def check_the_bound():
    import codec_deep_cases as D
    from fgumi_amd import GroupedReads
    case = D.the_bound()
    want_first = D.want_of(D.Case(GroupedReads.from_groups([case.g.records(0)])))
    D.check_deferred_beside_decided(case, want_first)
    D.check(case)


def check_option(name):
    import codec_deep_cases as D
    case = D.option_case(name)
    want = D.want_of(case)
    if name in D.OPTION_COUNTER:
        assert int(want["stats"][3 + D.OPTION_COUNTER[name]]) > 0, want["stats"].tolist()
    D.check(case, want)


def check_lone_iupac_read():
    """The same molecule without the IUPAC code is decided through the single-read table; with it, it is deferred and the host entry has the oracle's bytes."""
    import codec_deep_cases as D
    D.check(D.one_fr_template())
    D.check(D.one_fr_template(True))


def check_umi_of_unequal_length():
    """Not miscalled: the device entry defers the molecule and decides the one beside it."""
    import codec_deep_cases as D
    from fgumi_amd import GroupedReads
    case = D.umi_of_unequal_length()
    want_second = D.want_of(D.Case(GroupedReads.from_groups([case.g.records(1)])))
    D.check_deferred_beside_decided(case, want_second)


def check_cap(n_pairs, cap, n_molecules, bites):
    import codec_deep_cases as D
    case = D.cap(n_pairs, cap, n_molecules)
    want = D.want_of(case)
    down = int(want["stats"][3 + D.REJ_DOWNSAMPLED])
    assert (down > 0) == bites and case.capped == (n_molecules if bites else 0), (down, case.capped)
    if cap == 0:
        assert int(want["stats"][3 + D.REJ_INSUFFICIENT_READS]) > 0
    D.check(case, want)


def check_path_off(what):
    import codec_deep_cases as D
    case = D.path_off_case(what)
    if what != "rejects":
        D.check(case)
        return
    # --rejects: the device entry serves only batches it defers nothing of and refuses this one, as it did; the host entry decides it
    want = D.want_of(case)
    c = D.Caller(**case.opts)
    try:
        with pytest.raises(AssertionError, match="defers"):
            c.device(case.g)
        got = c.host(case.g)
        assert got["codec_deep"] == 0 and got["big"] == 0 and got["deep"] == 0 and got["duplex_deep"] == 0, got
        D.assert_equal(got, want, "host entry")
    finally:
        c.close()


def check_switch(value):
    """(child interpreter; FGX_CODEC_DEEP as the test set it) unset or "0": every deep molecule deferred, as before, the host entry the oracle's bytes; "1": decided."""
    import codec_deep_cases as D
    if value == "unset":
        assert "FGX_CODEC_DEEP" not in os.environ
    else:
        assert os.environ["FGX_CODEC_DEEP"] == value
    case = D.pairs(40, 2)
    if value != "1":
        case = D.Case(case.g, deferred=2)
        assert case.deep == 0
    D.check(case)


def check_switch_is_read_per_call():
    import codec_deep_cases as D
    case = D.pairs(40, 2)
    want = D.want_of(case)
    c = D.Caller()
    try:
        for value, is_on in (("1", True), ("0", False), (None, False), ("1", True)):
            if value is None:
                os.environ.pop("FGX_CODEC_DEEP", None)
            else:
                os.environ["FGX_CODEC_DEEP"] = value
            got = c.device(case.g)
            if is_on:
                D.assert_path(got, 0, 2, 0)
                D.assert_equal(got, want, "device entry")
            else:
                D.assert_path(got, 2, 0, 0)
    finally:
        c.close()


def check_unchanged_chain():
    """A batch without a deep molecule: the same kernel launches, the same host synchronisations and the same bytes with the switch on and off."""
    import codec_deep_cases as D
    case = D.shallow()
    want = D.want_of(case)
    c = D.Caller()
    try:
        seen = {}
        c.device(case.g)                                           # (a caller's first batch uploads its table images: not part of the comparison)
        for value in ("1", "0"):
            os.environ["FGX_CODEC_DEEP"] = value
            got = c.device(case.g)
            D.assert_path(got, 0, 0, 0)
            D.assert_equal(got, want, f"device entry, switch {value}")
            seen[value] = c.chain()
        print(f"(launches, host synchronisations): {seen}", flush=True)
        assert seen["1"] == seen["0"] and seen["1"][0] > 0, seen
    finally:
        c.close()


# ---- 1 / 2 ----
def test_32_pairs_stay_with_the_wavefront_kernel_and_33_are_deep():
    run_isolated(ME, "check_lower_edge", env=on(), timeout=T)


def test_64_and_65_pairs_take_the_two_builds_of_the_record_kernel():
    run_isolated(ME, "check_case", "build_edge", env=on(), timeout=T)


# ---- 3 / 4 ----
@pytest.mark.parametrize("n_pairs,ty", [(63, "c"), (64, "C"), (127, "C")])
def test_integer_tag_types(n_pairs, ty):
    run_isolated(ME, "check_integer_tag_types", n_pairs, ty, env=on(), timeout=T)


def test_the_bound():
    run_isolated(ME, "check_the_bound", env=on(), timeout=T)


# ---- 5 / 6 ----
@pytest.mark.parametrize("err", [0, 20000])
def test_error_rates(err):
    """0: unanimous columns; 20 000: many columns and UMI characters through k_call_full."""
    run_isolated(ME, "check_case", "pairs", 100, 2, err, env=on(), timeout=T)


@pytest.mark.parametrize("name", ["per_base_tags_on", "per_base_tags_off", "cell_tag_off", "min_reads_per_strand_1", "min_reads_per_strand_3", "min_reads_above_the_molecule",
                                  "min_duplex_length_above_the_overlap", "outer_bases_and_single_strand_masks", "min_input_base_quality_30", "poor_3prime_ends", "long_prefix"])
def test_option_matrix_on_a_long_tail(name):
    run_isolated(ME, "check_option", name, env=on(), timeout=T)


# ---- 7 ----
@pytest.mark.parametrize("name", ["read_through", "deepest_clip"])
def test_geometry(name):
    run_isolated(ME, "check_case", name, env=on(), timeout=T)


def test_indel_error_between_strands():
    import codec_deep_cases as D
    run_isolated(ME, "check_counter", "abutting_strands", (), D.REJ_INDEL_ERROR, env=on(), timeout=T)


def test_clip_overlap_failed():
    import codec_deep_cases as D
    run_isolated(ME, "check_counter", "clip_overlap_failed", (), D.REJ_CLIP_OVERLAP_FAILED, env=on(), timeout=T)


# ---- 8 ----
def test_some_templates_are_not_fr_pairs():
    import codec_deep_cases as D
    run_isolated(ME, "check_counter", "some_templates_not_fr", (), D.REJ_NOT_PRIMARY_FR_PAIR, env=on(), timeout=T)


def test_sets_of_one_read_and_an_iupac_code_in_a_lone_read():
    run_isolated(ME, "check_lone_iupac_read", env=on(), timeout=T)


# ---- 9 ----
@pytest.mark.parametrize("what", ["deletion", "soft_clip", "secondary", "fragment", "mates_not_adjacent", "three_records_with_one_name", "both_mates_first",
                                  "unequal_read_lengths"])
def test_not_this_paths(what):
    run_isolated(ME, "check_case", "not_this_path", what, env=on(), timeout=T)


# ---- 10 ----
@pytest.mark.parametrize("name", ["umi_disagreement", "no_rx", "rx_on_some_records", "cell_barcode_only_on_an_r2"])
def test_umis(name):
    run_isolated(ME, "check_case", name, env=on(), timeout=T)


def test_umi_of_unequal_length_is_deferred():
    run_isolated(ME, "check_umi_of_unequal_length", env=on(), timeout=T)


# ---- 11 ----
@pytest.mark.parametrize("n_pairs,cap,n_molecules,bites", [(40, 20, 2, True), (40, 1, 2, True), (40, 0, 2, False), (40, 40, 2, False), (40, 50, 2, False), (127, 30, 1, True)])
def test_cap(n_pairs, cap, n_molecules, bites):
    run_isolated(ME, "check_cap", n_pairs, cap, n_molecules, bites, env=on(), timeout=T)


# ---- 12 ----
@pytest.mark.parametrize("what", ["trim", "rejects"])
def test_options_that_keep_the_path_off(what):
    run_isolated(ME, "check_path_off", what, env=on(), timeout=T)


# ---- 13 ----
@pytest.mark.parametrize("value", ["unset", "0", "1"])
def test_switch(value):
    run_isolated(ME, "check_switch", value, env=env(**({} if value == "unset" else dict(FGX_CODEC_DEEP=value))), timeout=T)


def test_switch_is_read_per_call():
    run_isolated(ME, "check_switch_is_read_per_call", env=env(), timeout=T)


def test_unchanged_chain_without_a_deep_molecule():
    run_isolated(ME, "check_unchanged_chain", env=env(), timeout=T)


# ---- 14 ----
def test_mixed_stream_device_entry():
    run_isolated(ME, "check_case", "mixed_stream", env=on(), timeout=T)
