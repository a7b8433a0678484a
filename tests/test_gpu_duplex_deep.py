"""GPU parity: duplex molecules of more than 64 records decided by k_duplex_deep_parse + k_duplex_deep_cols (fgumi_amd/csrc/duplex_deep.inc) — up to 512
records, at most 255 retained reads per record side.  Each test compares both entries with the oracle byte for byte, count and all 28 counters included, and
asserts the path of the device batch: how many molecules were deferred, fgx_debug_last_duplex_deep = the molecules above 64 records that were not, none of them
counted as a simplex big / deep family.  The batches are those of tests/duplex_deep_cases.py (a handful of molecules each); each is built once and never
modified.  Without duplex_deep.inc every such molecule is deferred and the library has no fgx_debug_last_duplex_deep."""
import os

import numpy as np
import pytest

import duplex_deep_cases as D
from isolated import run_isolated

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name, *args, want=True):
    key = (name,) + args
    if key not in _CASES:
        case = getattr(D, name)(*args)
        _CASES[key] = (case, D.want_of(case) if want else None)
    return _CASES[key]


@pytest.fixture(autouse=True)
def switch_unset(monkeypatch):
    monkeypatch.delenv("FGX_DUPLEX_DEEP", raising=False)


def test_32_pairs_stay_with_the_wavefront_kernel_and_33_are_deep():
    case, want = _case("lower_edge")
    assert D.records_per_family(case.g).tolist() == [64, 66] and case.deep == 1
    D.check(case, want)


@pytest.mark.parametrize("n_pairs,ty", [(127, "c"), (128, "C"), (255, "C")])
def test_integer_tag_types(n_pairs, ty):
    """The oracle's own cD is type c at 127 pairs and type C at 128 and at 255; the device bytes then equal the oracle's."""
    case, want = _case("pairs", n_pairs)
    cd = D.cd_types(want["data"])
    assert len(cd) == 2 and all(t == ty for t, _ in cd), cd
    D.check(case, want)


def test_the_bound():
    """255 pairs are decided, 256 pairs are deferred: the device entry's bytes are the oracle's for the first molecule alone, the host entry's for both."""
    from fgumi_amd import GroupedReads
    case, want = _case("the_bound")
    want_first = D.want_of(D.Case(GroupedReads.from_groups([case.g.records(0)])))
    D.check_deferred_beside_decided(case, want_first)
    D.check(case, want)


@pytest.mark.parametrize("err", [0, 20000])
def test_error_rates(err):
    """0: unanimous columns far above the cap depth; 20 000: many columns and UMI characters through k_call_full."""
    D.check(*_case("pairs", 100, 2, err))


@pytest.mark.parametrize("name", list(D.OPTION_MATRIX))
def test_option_matrix_on_a_long_tail(name):
    D.check(*_case("option_case", name))


def test_read_through_inserts_with_masked_input():
    case, want = _case("read_through")
    assert int(want["stats"][3 + D.REJ_ZERO_LENGTH]) > 0
    D.check(case, want)


def test_lone_strand_is_passed_through():
    case, want = _case("only_a_strand", (1, 1, 0))
    assert want["count"] == 2
    D.check(case, want)


def test_lone_strand_is_rejected_under_1_1_1():
    case, want = _case("only_a_strand", (1, 1, 1))
    assert want["count"] == 0 and int(want["stats"][3 + D.REJ_INSUFFICIENT_READS]) > 0
    D.check(case, want)


def test_single_read_sets():
    D.check(*_case("single_read_sets"))


def test_stray_fragment_records():
    case, want = _case("stray_fragments")
    assert int(want["stats"][3 + D.REJ_FRAGMENT_READ]) > 0
    D.check(case, want)


def test_strand_collision():
    case, want = _case("strand_collision")
    assert int(want["stats"][3 + D.REJ_POTENTIAL_COLLISION]) > 0
    D.check(case, want)


def test_r1_only_molecule():
    D.check(*_case("r1_only"))


@pytest.mark.parametrize("name", ["umi_disagreement", "paired_umi", "no_rx"])
def test_umis(name):
    D.check(*_case(name))


def test_umi_of_unequal_length_is_deferred():
    """Not miscalled: the device entry defers the molecule and decides the one beside it; the oracle refuses such a molecule, and so does the host entry."""
    from fgumi_amd import GroupedReads
    case, _ = _case("umi_of_unequal_length", want=False)
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


@pytest.mark.parametrize("what", ["deletion", "soft_clip", "secondary"])
def test_not_this_paths(what):
    """Deferred as before (duplex_deep 0), never miscalled: the host entry's bytes are the oracle's."""
    D.check(*_case("not_this_path", what))


@pytest.mark.parametrize("what", ["trim", "cap", "methylation"])
def test_options_that_keep_the_path_off(what):
    contigs = D.methylation_contigs() if what == "methylation" else None
    case = D.path_off_case(what)
    D.check(case, D.want_of(case, contigs), contigs)


def test_rejects_keep_the_path_off():
    """--rejects: the device entry serves only batches it defers nothing of and refuses this one, as it did; the host entry decides it without the new kernels."""
    case = D.path_off_case("rejects")
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


def test_switch_at_0_defers_as_before(monkeypatch):
    monkeypatch.setenv("FGX_DUPLEX_DEEP", "0")
    case, want = _case("pairs", 40, 2)
    off = D.Case(case.g, deferred=2)
    assert off.deep == 0
    D.check(off, want)


def test_switch_is_read_per_call(monkeypatch):
    case, want = _case("pairs", 40, 2)
    c = D.Caller()
    try:
        for value, on in (("1", True), ("0", False), (None, True), ("0", False), ("1", True)):
            if value is None:
                monkeypatch.delenv("FGX_DUPLEX_DEEP", raising=False)
            else:
                monkeypatch.setenv("FGX_DUPLEX_DEEP", value)
            got = c.device(case.g)
            if on:
                assert got["duplex_deep"] == 2 and got["deferred"] == 0, (value, got)
                D.assert_equal(got, want, "device entry")
            else:
                assert got["duplex_deep"] == 0 and got["deferred"] == 2, (value, got)
    finally:
        c.close()


def test_unchanged_chain_without_a_deep_molecule(monkeypatch):
    """A batch without a deep molecule: the same kernel launches, the same host synchronisations and the same bytes with the switch on and off."""
    case, want = _case("shallow")
    c = D.Caller()
    try:
        seen = {}
        c.device(case.g)                                           # (a caller's first batch uploads its table images: not part of the comparison)
        for value in ("1", "0"):
            monkeypatch.setenv("FGX_DUPLEX_DEEP", value)
            got = c.device(case.g)
            assert got["deferred"] == 0 and got["duplex_deep"] == 0
            D.assert_equal(got, want, f"device entry, switch {value}")
            seen[value] = c.chain()
        assert seen["1"] == seen["0"] and seen["1"][0] > 0, seen
    finally:
        c.close()


def test_mixed_stream_device_entry():
    D.check(*_case("mixed_stream"))


def check_run_bam(tmp_dir):
    """(child interpreter) fgx_run_bam on the mixed stream, in one chunk and in 64 KiB chunks: the oracle's records in order, no group deferred, no batch
    through the host entry."""
    from fgumi_amd import DuplexConsensusCaller, bgzf
    case = D.mixed_stream()
    g = case.g
    want = D.want_of(case)
    c = DuplexConsensusCaller("", "A", [1, 1, 0], cell_tag="CB", overlapping_consensus=True)
    refs = [("chr%d" % (i + 1), 2147483647) for i in range(24)]
    src, dst = os.path.join(tmp_dir, "grouped.bam"), os.path.join(tmp_dir, "consensus.bam")
    bgzf.write_bam(src, bgzf.grouped_input_header(refs), refs, g.blob)
    for chunk in (0, 1 << 16):
        st = c.run_bam(src, dst, chunk_raw_bytes=chunk, threads=8, strip_strand_suffix=True)
        _, _, stream, off, ln = bgzf.read_bam(dst)
        got = b"".join(bytes(stream[int(a) - 4:int(a) + int(b)]) for a, b in zip(off, ln))
        print(f"chunk {chunk}: chunks {st['chunks']}, deferred groups {st['deferred_groups']}, host entry batches {st['host_entry_batches']}", flush=True)
        D.assert_equal(dict(data=got, count=len(off), stats=np.array(st["stats"][:28], dtype=np.uint64)), want, f"the consensus BAM, chunk_raw_bytes {chunk}")
        assert st["deferred_groups"] == 0 and st["host_entry_batches"] == 0, (st["deferred_groups"], st["host_entry_batches"])
    c.close()


def test_mixed_stream_run_bam(tmp_path):
    run_isolated("test_gpu_duplex_deep", "check_run_bam", str(tmp_path), timeout=600)


def check_under_guard_bands():
    """(child interpreter, FGX_GUARD_BAND set) the long-tail batch through the new kernels, then a look at every guarded buffer."""
    import ctypes as C
    from fgumi_amd import lib
    lib.fgx_debug_check_guard_bands.restype = C.c_int
    lib.fgx_debug_check_guard_bands.argtypes = [C.c_char_p, C.c_int]
    D.check(D.option_case("min_reads_2_1_0"))
    msg = C.create_string_buffer(600)
    bad = lib.fgx_debug_check_guard_bands(msg, 600)
    assert bad == 0, f"deep duplex molecules: {bad} device buffer(s) written outside their bounds: {msg.value.decode()}"


def test_under_guard_bands():
    run_isolated("test_gpu_duplex_deep", "check_under_guard_bands", env={"FGX_GUARD_BAND": "4096"}, timeout=600)
