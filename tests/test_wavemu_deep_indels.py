"""FGX_DEEP_INDELS=1 on the CPU, in 64-lane lock-step (tests/wavemu — a cross-lane operation or a barrier under divergent control flow faults there): duplex
molecules of 65 .. 512 records with indel reads.  k_canon_duplex_deep (fgumi_amd/csrc/canon_deep.inc) against the scalar form at 512 records for every case of
tests/deep_indel_cases.py — status always, and in scope delta, lengths and every byte —, then both entries of the emulation library against the oracle with the
switch on, and the switch itself.  Every case runs in a child interpreter.  Without the feature the library has none of the three exports and the device entry
defers every such molecule."""
import os

import pytest

from isolated import run_isolated
from test_wavemu import env

T = 900
E2E = [n for n in __import__("deep_indel_cases").CASES]


def check_kernel(name, option_set=-1):
    import deep_indel_cases as D
    case = D.CASES[name]()
    if option_set >= 0:
        case = D.with_option_set(case, option_set)
        case.in_scope = D.canonical(D.options_of(case), case.recs)["status"] == 0       # (the option set decides; the comparison is the test)
    D.check_kernel_against_scalar(case)


def check_end_to_end(name, option_set=-1):
    import deep_indel_cases as D
    case = D.CASES[name]()
    if option_set >= 0:
        case = D.with_option_set(case, option_set)
        case.in_scope = D.canonical(D.options_of(case), case.recs)["status"] == 0
    D.check_end_to_end(case)


def _deletion_case():
    import duplex_deep_cases as DD
    return DD.not_this_path("deletion")


def check_switch(value):
    """(FGX_DEEP_INDELS as the test set it) unset or "0": the deletion molecule of tests/duplex_deep_cases.py is deferred as before; "1": decided, the oracle's bytes."""
    import deep_indel_cases as D
    import duplex_deep_cases as DD
    if value == "unset":
        assert "FGX_DEEP_INDELS" not in os.environ
    else:
        assert os.environ["FGX_DEEP_INDELS"] == value
    case = _deletion_case()
    want = DD.want_of(case)
    c = D.Caller(DD.options_of(case))
    try:
        got = c.device(case.g)
        path = {k: got[k] for k in ("deferred", "canon", "deep_indels", "duplex_deep")}
        if value == "1":
            assert path == dict(deferred=0, canon=1, deep_indels=1, duplex_deep=0), path
            D.assert_equal(got, want, "device entry")
        else:
            assert path == dict(deferred=1, canon=0, deep_indels=0, duplex_deep=0), path
        D.assert_equal(c.host(case.g), want, "host entry")
    finally:
        c.close()


def check_switch_is_read_per_call():
    import deep_indel_cases as D
    import duplex_deep_cases as DD
    case = _deletion_case()
    want = DD.want_of(case)
    c = D.Caller(DD.options_of(case))
    try:
        for value, on in (("1", True), ("0", False), (None, False), ("1", True), ("", False), ("01", False), ("yes", True)):
            if value is None:
                os.environ.pop("FGX_DEEP_INDELS", None)
            else:
                os.environ["FGX_DEEP_INDELS"] = value
            got = c.device(case.g)
            if on:
                assert got["deferred"] == 0 and got["deep_indels"] == 1, (value, got["deferred"], got["deep_indels"])
                D.assert_equal(got, want, "device entry")
            else:
                assert got["deferred"] == 1 and got["deep_indels"] == 0, (value, got["deferred"], got["deep_indels"])
    finally:
        os.environ.pop("FGX_DEEP_INDELS", None)
        c.close()


def check_unchanged_chain(which):
    """A shallow batch / a deep batch without indels: the same launches, host synchronisations and bytes with the switch unset and on."""
    import deep_indel_cases as D
    import duplex_deep_cases as DD
    case = DD.shallow() if which == "shallow" else DD.pairs(40, 2)
    want = DD.want_of(case)
    c = D.Caller(DD.options_of(case))
    try:
        seen = {}
        c.device(case.g)                                           # (a caller's first batch uploads its table images)
        for value in (None, "1"):
            if value is None:
                os.environ.pop("FGX_DEEP_INDELS", None)
            else:
                os.environ["FGX_DEEP_INDELS"] = value
            got = c.device(case.g)
            assert got["deferred"] == 0 and got["deep_indels"] == 0 and got["duplex_deep"] == case.deep, got
            D.assert_equal(got, want, f"device entry, switch {value}")
            seen[value] = c.chain()
        print(f"(launches, host synchronisations): {seen}", flush=True)
        assert seen[None] == seen["1"] and seen["1"][0] > 0, seen
    finally:
        os.environ.pop("FGX_DEEP_INDELS", None)
        c.close()


def check_options_that_keep_the_path_off(what):
    """--trim, --rejects (host entry) and the methylation-aware mode with the switch on: the molecule takes the route it took, the bytes are the oracle's."""
    import deep_indel_cases as D
    import duplex_deep_cases as DD
    assert os.environ.get("FGX_DEEP_INDELS") == "1"
    case = D.CASES["66_records"]()
    opts = dict(trim=dict(trim=1), rejects=dict(track_rejects=1), methylation=dict(methylation_mode=1))[what]
    o = D.options_of(case, **opts)
    g = D.grouped(case.recs)
    contigs = DD.methylation_contigs() if what == "methylation" else None
    import orc
    orc.set_reference(contigs)
    try:
        want = D.want_of(o, g)
    finally:
        orc.set_reference(None)
    c = DD.Caller(contigs, **opts)
    try:
        c.lib.fgx_debug_last_deep_indels.restype = __import__("ctypes").c_uint32
        got = c.host(g)
        assert int(c.lib.fgx_debug_last_deep_indels(c.h)) == 0
        D.assert_equal(got, want, "host entry")
    finally:
        c.close()


@pytest.mark.parametrize("name", E2E)
def test_kernel_against_the_scalar_form(name):
    run_isolated("test_wavemu_deep_indels", "check_kernel", name, env=env(), timeout=T)


@pytest.mark.parametrize("name", ["130_records", "prefixes", "nibbles_insert_141", "first_record_dropped_same_cb"])
@pytest.mark.parametrize("option_set", [0, 1, 2])
def test_kernel_against_the_scalar_form_under_the_option_sets(name, option_set):
    run_isolated("test_wavemu_deep_indels", "check_kernel", name, option_set, env=env(), timeout=T)


@pytest.mark.parametrize("name", E2E)
def test_end_to_end(name):
    run_isolated("test_wavemu_deep_indels", "check_end_to_end", name, env=env(FGX_DEEP_INDELS=1), timeout=T)


@pytest.mark.parametrize("name", ["130_records", "nibbles_insert_150", "drops_to_64"])
@pytest.mark.parametrize("option_set", [0, 1, 2])
def test_end_to_end_under_the_option_sets(name, option_set):
    run_isolated("test_wavemu_deep_indels", "check_end_to_end", name, option_set, env=env(FGX_DEEP_INDELS=1), timeout=T)


@pytest.mark.parametrize("value", ["unset", "0", "1"])
def test_switch(value):
    run_isolated("test_wavemu_deep_indels", "check_switch", value, env=env(**({} if value == "unset" else dict(FGX_DEEP_INDELS=value))), timeout=T)


def test_switch_is_read_per_call():
    run_isolated("test_wavemu_deep_indels", "check_switch_is_read_per_call", env=env(), timeout=T)


@pytest.mark.parametrize("which", ["shallow", "deep_without_indels"])
def test_unchanged_chain(which):
    run_isolated("test_wavemu_deep_indels", "check_unchanged_chain", which, env=env(), timeout=T)


@pytest.mark.parametrize("what", ["trim", "rejects", "methylation"])
def test_options_that_keep_the_path_off(what):
    run_isolated("test_wavemu_deep_indels", "check_options_that_keep_the_path_off", what, env=env(FGX_DEEP_INDELS=1), timeout=T)
