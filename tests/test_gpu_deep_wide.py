"""GPU parity: FGX_DEEP_WIDE=1 — simplex families the streaming kernels of deep families refuse for size alone (more than 512 records, 1 024 under --max-reads, or
an end that keeps more than 255 reads) decided by the wide kernels of fgumi_amd/csrc/simplex_wide.inc, up to 16 384 records.  Each test compares the
device-resident output with the oracle byte for byte, count and all 28 counters included, and asserts the path: nothing deferred,
fgx_debug_last_wide_families = the families built to need the wide kernels, fgx_debug_last_deep_families = those the existing builds take.  The batches are
those of tests/wide_cases.py; each is built once and never modified."""
import os

import numpy as np
import pytest

import wide_cases as W
from isolated import run_isolated

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name, *args):
    key = (name,) + args
    if key not in _CASES:
        case = getattr(W, name)(*args)
        _CASES[key] = (case, None if name in ("umi_of_unequal_length", "the_bound") else W.want_of(case))
    return _CASES[key]


@pytest.fixture
def wide_on(monkeypatch):
    monkeypatch.setenv("FGX_DEEP_WIDE", "1")


@pytest.mark.parametrize("err", [5000, 0])
def test_255_pairs_stay_with_the_streaming_kernels_and_256_are_wide(wide_on, err):
    """error_rate_ppm 0: unanimous columns far above unanimous_cap_depth()."""
    W.check_on(*_case("byte_edge", err))


def test_513_to_1024_records_without_a_cap(wide_on):
    W.check_on(*_case("up_to_1024_records"))


def test_more_than_1024_records_without_a_cap(wide_on):
    W.check_on(*_case("above_1024_records"))


@pytest.mark.parametrize("cap", [100, 400])
def test_more_than_1024_records_under_a_cap(wide_on, cap):
    """1 100 .. 1 400 records: above DEEP_CAP_MAX.  Cap 100: the ends fit 255 reads after the cut; cap 400: they do not."""
    case, want = _case("capped", cap)
    assert int(want["stats"][3 + W.REJ_DOWNSAMPLED]) > 0
    W.check_on(case, want)


def test_equal_ranks_at_the_cut_keep_file_order(wide_on):
    case, want = _case("capped", 100, 3, (550, 700), True)
    assert int(want["stats"][3 + W.REJ_DOWNSAMPLED]) > 0
    W.check_on(case, want)


def test_min_reads_3_on_read_through_inserts(wide_on):
    W.check_on(*_case("read_through"))


def test_masked_input(wide_on):
    W.check_on(*_case("masked"))


def test_umi_characters_with_more_than_255_observations(wide_on):
    W.check_on(*_case("umi_disagreement"))


def test_umi_of_unequal_length_is_deferred(wide_on):
    """Not miscalled: the device entry defers the family (and decides the one beside it); the oracle refuses such a family, and so does the host entry."""
    case, _ = _case("umi_of_unequal_length")
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


def test_orphan_end(wide_on):
    case, want = _case("orphan_end")
    assert want["count"] == 0 and int(want["stats"][3 + W.REJ_ORPHAN_CONSENSUS]) == 300 and int(want["stats"][3 + W.REJ_INSUFFICIENT_READS]) == 0
    W.check_on(case, want)


def test_the_bound(wide_on):
    """A family of exactly WIDE_MAX records beside one of WIDE_MAX + 2: the device entry finishes the first (the oracle's bytes for it) and defers the second;
    the host entry returns the oracle's bytes for both."""
    from fgumi_amd import GroupedReads
    case, _ = _case("the_bound")
    n = W.records_per_family(case.g)
    assert n.tolist() == [W.WIDE_MAX, W.WIDE_MAX + 2]
    want = W.want_of(case)
    first = GroupedReads.from_groups([case.g.records(0)])
    want_first = W.want_of(W.Case(first, 1, 0))
    c = W.Caller()
    try:
        got = c.device(case.g)
        assert got["deferred"] == 1 and got["wide"] == 1 and got["deep"] == 0, {k: got[k] for k in ("big", "deep", "wide", "deferred")}
        assert got["data"] == want_first["data"] and got["count"] == want_first["count"]
        W.assert_equal(c.host(case.g), want, "host entry")
    finally:
        c.close()


def test_mixed_stream_device_entry(wide_on):
    W.check_on(*_case("mixed_stream"))


def check_run_bam(tmp_dir):
    """(child interpreter, FGX_DEEP_WIDE=1) fgx_run_bam on the mixed stream, in one chunk and in many: the oracle's records in order, no group deferred, no batch
    through the host entry."""
    from fgumi_amd import VanillaUmiConsensusCaller, VanillaUmiConsensusOptions, bgzf
    import fgx_opts
    import orc
    case = W.mixed_stream()
    g = case.g
    want = orc.process(fgx_opts.defaults(min_reads=1), g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=100000)
    c = VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(min_reads=1, min_consensus_base_quality=2, cell_tag="CB"), overlapping_consensus=True)
    refs = [("chr%d" % (i + 1), 2147483647) for i in range(24)]
    src, dst = os.path.join(tmp_dir, "grouped.bam"), os.path.join(tmp_dir, "consensus.bam")
    bgzf.write_bam(src, bgzf.grouped_input_header(refs), refs, g.blob)
    for chunk in (0, 1 << 16):
        st = c.run_bam(src, dst, chunk_raw_bytes=chunk, threads=8)
        _, _, stream, off, ln = bgzf.read_bam(dst)
        got = b"".join(bytes(stream[int(a) - 4:int(a) + int(b)]) for a, b in zip(off, ln))
        print(f"chunk {chunk}: chunks {st['chunks']}, deferred groups {st['deferred_groups']}, host entry batches {st['host_entry_batches']}", flush=True)
        assert got == want["data"], "the consensus BAM's records differ from the oracle's"
        assert st["stats"][:28] == [int(v) for v in want["stats"]]
        assert st["deferred_groups"] == 0 and st["host_entry_batches"] == 0, (st["deferred_groups"], st["host_entry_batches"])
    c.close()


def test_mixed_stream_run_bam(tmp_path):
    run_isolated("test_gpu_deep_wide", "check_run_bam", str(tmp_path), env={"FGX_DEEP_WIDE": "1"}, timeout=600)


@pytest.mark.parametrize("value", [None, "0", ""])
def test_switch_off(monkeypatch, value):
    """Unset, "0" and "": the library as it was — every such family deferred by the device entry, the oracle's bytes from the host entry."""
    if value is None:
        monkeypatch.delenv("FGX_DEEP_WIDE", raising=False)
    else:
        monkeypatch.setenv("FGX_DEEP_WIDE", value)
    W.check_off(*_case("up_to_1024_records"))


def test_switch_is_read_per_call(monkeypatch):
    case, want = _case("up_to_1024_records")
    c = W.Caller()
    try:
        for value, on in (("1", True), ("0", False), ("yes", True), ("", False)):
            monkeypatch.setenv("FGX_DEEP_WIDE", value)
            got = c.device(case.g)
            if on:
                assert got["wide"] == case.wide and got["deferred"] == 0, (value, got)
                W.assert_equal(got, want, "device entry")
            else:
                assert got["wide"] == 0 and got["deferred"] == case.g.n_grp, (value, got)
    finally:
        c.close()


def check_under_guard_bands():
    """(child interpreter, FGX_GUARD_BAND and FGX_DEEP_WIDE set) the wide kernels' batch, then a look at every guarded buffer."""
    import ctypes as C
    from fgumi_amd import lib
    lib.fgx_debug_check_guard_bands.restype = C.c_int
    lib.fgx_debug_check_guard_bands.argtypes = [C.c_char_p, C.c_int]
    lib.fgx_debug_guarded_buffers.restype = C.c_int
    W.check_on(W.up_to_1024_records())
    msg = C.create_string_buffer(600)
    bad = lib.fgx_debug_check_guard_bands(msg, 600)
    assert bad == 0, f"wide families: {bad} device buffer(s) written outside their bounds: {msg.value.decode()}"
    assert lib.fgx_debug_guarded_buffers() >= 20, lib.fgx_debug_guarded_buffers()


def test_wide_kernels_under_guard_bands():
    run_isolated("test_gpu_deep_wide", "check_under_guard_bands", env={"FGX_GUARD_BAND": "4096", "FGX_DEEP_WIDE": "1"}, timeout=600)
