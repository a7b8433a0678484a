"""GPU parity: CODEC molecules of more than 64 records decided by k_codec_deep_parse + k_codec_deep_cols (fgumi_amd/csrc/codec_deep.inc) — up to 254 records,
under FGX_CODEC_DEEP=1.  Each test compares both entries with the oracle byte for byte, count and all 28 counters included, and asserts the path of the device
batch exactly: how many molecules were deferred, fgx_debug_last_codec_deep, fgx_debug_last_codec_deep_capped, and nothing counted as a simplex big / deep
family or a deep duplex molecule.  The batches are those of tests/codec_deep_cases.py (one to three molecules each, but the mixed stream); each is built once
and never modified.  Without codec_deep.inc every such molecule is deferred and the library has no fgx_debug_last_codec_deep."""
import os

import numpy as np
import pytest

import codec_deep_cases as D
from isolated import run_isolated

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name, *args):
    key = (name,) + args
    if key not in _CASES:
        case = getattr(D, name)(*args)
        _CASES[key] = (case, D.want_of(case))
    return _CASES[key]


@pytest.fixture(autouse=True)
def switch_on(monkeypatch):
    monkeypatch.setenv("FGX_CODEC_DEEP", "1")


def _counted(want, counter):
    return int(want["stats"][3 + counter])


# ---- 1 / 2 ----
def test_32_pairs_stay_with_the_wavefront_kernel_and_33_are_deep():
    case, want = _case("lower_edge")
    assert D.records_per_family(case.g).tolist() == [64, 66] and case.deep == 1
    D.check(case, want)


def test_64_and_65_pairs_take_the_two_builds_of_the_record_kernel():
    D.check(*_case("build_edge"))


# ---- 3 / 4 ----
@pytest.mark.parametrize("n_pairs,ty", [(63, "c"), (64, "C"), (127, "C")])
def test_integer_tag_types(n_pairs, ty):
    """The oracle's own cD is type c at 63 pairs and type C at 64 and at 127 — some position is covered by both strands; the device bytes then equal the oracle's."""
    case, want = _case("pairs", n_pairs)
    cd = D.cd_types(want["data"])
    assert len(cd) == 1 and cd[0] == (ty, 2 * n_pairs), cd
    D.check(case, want)


def test_the_bound():
    """127 pairs are decided, 128 pairs are deferred: the device entry's bytes are the oracle's for the first molecule alone, the host entry's for both."""
    from fgumi_amd import GroupedReads
    case, want = _case("the_bound")
    want_first = D.want_of(D.Case(GroupedReads.from_groups([case.g.records(0)])))
    D.check_deferred_beside_decided(case, want_first)
    D.check(case, want)


# ---- 5 / 6 ----
@pytest.mark.parametrize("err", [0, 20000])
def test_error_rates(err):
    """0: unanimous columns; 20 000: many columns and UMI characters through k_call_full."""
    D.check(*_case("pairs", 100, 2, err))


@pytest.mark.parametrize("name", list(D.OPTION_MATRIX))
def test_option_matrix_on_a_long_tail(name):
    case, want = _case("option_case", name)
    if name in D.OPTION_COUNTER:
        assert _counted(want, D.OPTION_COUNTER[name]) > 0, want["stats"].tolist()
    D.check(case, want)


# ---- 7 ----
@pytest.mark.parametrize("name", ["read_through", "deepest_clip"])
def test_geometry(name):
    D.check(*_case(name))


def test_indel_error_between_strands():
    case, want = _case("abutting_strands")
    assert _counted(want, D.REJ_INDEL_ERROR) > 0
    D.check(case, want)


def test_clip_overlap_failed():
    case, want = _case("clip_overlap_failed")
    assert _counted(want, D.REJ_CLIP_OVERLAP_FAILED) > 0
    D.check(case, want)


# ---- 8 ----
def test_some_templates_are_not_fr_pairs():
    case, want = _case("some_templates_not_fr")
    assert _counted(want, D.REJ_NOT_PRIMARY_FR_PAIR) > 0 and want["count"] == 1
    D.check(case, want)


def test_sets_of_one_read():
    D.check(*_case("one_fr_template"))


def test_iupac_code_in_a_lone_read_is_deferred():
    D.check(*_case("one_fr_template", True))


# ---- 9 ----
@pytest.mark.parametrize("what", D.NOT_THIS_PATH)
def test_not_this_paths(what):
    """Deferred as before (codec_deep 0), never miscalled: the host entry's bytes are the oracle's."""
    D.check(*_case("not_this_path", what))


# ---- 10 ----
@pytest.mark.parametrize("name", ["umi_disagreement", "no_rx", "rx_on_some_records", "cell_barcode_only_on_an_r2"])
def test_umis(name):
    D.check(*_case(name))


def test_umi_of_unequal_length_is_deferred():
    """Not miscalled: the device entry defers the molecule and decides the one beside it."""
    from fgumi_amd import GroupedReads
    case = D.umi_of_unequal_length()
    want_second = D.want_of(D.Case(GroupedReads.from_groups([case.g.records(1)])))
    D.check_deferred_beside_decided(case, want_second)


# ---- 11 ----
@pytest.mark.parametrize("n_pairs,cap,n_molecules,bites", [(40, 20, 2, True), (40, 1, 2, True), (40, 0, 2, False), (40, 40, 2, False), (40, 50, 2, False), (127, 30, 1, True)])
def test_cap(n_pairs, cap, n_molecules, bites):
    """A cap that bites both lists, a cap of 1, a cap of 0 (InsufficientReads, nothing downsampled), a cap at and above the list size (no CAP work), a capped
    molecule at the 127-pair bound."""
    case, want = _case("cap", n_pairs, cap, n_molecules)
    assert (_counted(want, D.REJ_DOWNSAMPLED) > 0) == bites and case.capped == (n_molecules if bites else 0)
    if cap == 0:
        assert _counted(want, D.REJ_INSUFFICIENT_READS) > 0
    D.check(case, want)


# ---- 12 ----
def test_trim_keeps_the_path_off():
    D.check(*_case("path_off_case", "trim"))


def test_rejects_keep_the_path_off():
    """--rejects: the device entry serves only batches it defers nothing of and refuses this one, as it did; the host entry decides it without the new kernels."""
    case, want = _case("path_off_case", "rejects")
    c = D.Caller(**case.opts)
    try:
        with pytest.raises(AssertionError, match="defers"):
            c.device(case.g)
        got = c.host(case.g)
        assert got["codec_deep"] == 0 and got["big"] == 0 and got["deep"] == 0 and got["duplex_deep"] == 0, got
        D.assert_equal(got, want, "host entry")
    finally:
        c.close()


# ---- 13 ----
@pytest.mark.parametrize("value", [None, "0"])
def test_switch_unset_or_0_defers_as_before(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("FGX_CODEC_DEEP")
    else:
        monkeypatch.setenv("FGX_CODEC_DEEP", value)
    case, want = _case("pairs", 40, 2)
    off = D.Case(case.g, deferred=2)
    assert off.deep == 0
    D.check(off, want)


def test_switch_at_1_decides():
    D.check(*_case("pairs", 40, 2))


def test_switch_is_read_per_call(monkeypatch):
    case, want = _case("pairs", 40, 2)
    c = D.Caller()
    try:
        for value, on in (("1", True), ("0", False), (None, False), ("1", True)):
            if value is None:
                monkeypatch.delenv("FGX_CODEC_DEEP", raising=False)
            else:
                monkeypatch.setenv("FGX_CODEC_DEEP", value)
            got = c.device(case.g)
            if on:
                D.assert_path(got, 0, 2, 0)
                D.assert_equal(got, want, "device entry")
            else:
                D.assert_path(got, 2, 0, 0)
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
            monkeypatch.setenv("FGX_CODEC_DEEP", value)
            got = c.device(case.g)
            D.assert_path(got, 0, 0, 0)
            D.assert_equal(got, want, f"device entry, switch {value}")
            seen[value] = c.chain()
        assert seen["1"] == seen["0"] and seen["1"][0] > 0, seen
    finally:
        c.close()


# ---- 14 ----
def test_mixed_stream_device_entry():
    D.check(*_case("mixed_stream"))


def check_run_bam(tmp_dir):
    """(child interpreter, FGX_CODEC_DEEP=1) fgx_run_bam on the mixed stream, in one chunk and in 64 KiB chunks: the oracle's records in order, no group
    deferred, no batch through the host entry."""
    from fgumi_amd import CodecConsensusCaller, CodecConsensusOptions, bgzf
    case = D.mixed_stream()
    g = case.g
    want = D.want_of(case)
    c = CodecConsensusCaller("", "A", CodecConsensusOptions(produce_per_base_tags=True))
    refs = [("chr%d" % (i + 1), 2147483647) for i in range(24)]
    src, dst = os.path.join(tmp_dir, "grouped.bam"), os.path.join(tmp_dir, "consensus.bam")
    bgzf.write_bam(src, bgzf.grouped_input_header(refs), refs, g.blob)
    for chunk in (0, 1 << 16):
        st = c.run_bam(src, dst, chunk_raw_bytes=chunk, threads=8)
        _, _, stream, off, ln = bgzf.read_bam(dst)
        got = b"".join(bytes(stream[int(a) - 4:int(a) + int(b)]) for a, b in zip(off, ln))
        print(f"chunk {chunk}: chunks {st['chunks']}, deferred groups {st['deferred_groups']}, host entry batches {st['host_entry_batches']}", flush=True)
        D.assert_equal(dict(data=got, count=len(off), stats=np.array(st["stats"][:28], dtype=np.uint64)), want, f"the consensus BAM, chunk_raw_bytes {chunk}")
        assert st["deferred_groups"] == 0 and st["host_entry_batches"] == 0, (st["deferred_groups"], st["host_entry_batches"])
    c.close()


def test_mixed_stream_run_bam(tmp_path):
    run_isolated("test_gpu_codec_deep", "check_run_bam", str(tmp_path), env={"FGX_CODEC_DEEP": "1"}, timeout=600)


def check_under_guard_bands():
    """(child interpreter, FGX_GUARD_BAND and FGX_CODEC_DEEP set) the long-tail batch and a capped batch through the new kernels, then a look at every guarded buffer."""
    import ctypes as C
    from fgumi_amd import lib
    lib.fgx_debug_check_guard_bands.restype = C.c_int
    lib.fgx_debug_check_guard_bands.argtypes = [C.c_char_p, C.c_int]
    D.check(D.option_case("per_base_tags_on"))
    D.check(D.cap(40, 20))
    msg = C.create_string_buffer(600)
    bad = lib.fgx_debug_check_guard_bands(msg, 600)
    assert bad == 0, f"deep CODEC molecules: {bad} device buffer(s) written outside their bounds: {msg.value.decode()}"


def test_under_guard_bands():
    run_isolated("test_gpu_codec_deep", "check_under_guard_bands", env={"FGX_GUARD_BAND": "4096", "FGX_CODEC_DEEP": "1"}, timeout=600)
