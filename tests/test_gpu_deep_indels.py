"""GPU parity of FGX_DEEP_INDELS=1: duplex molecules of 65 .. 512 records with indel reads.  k_canon_duplex_deep (fgumi_amd/csrc/canon_deep.inc, a workgroup per
molecule) against the scalar form at 512 records — status always; in scope delta, lengths, every byte of every kept record and its prefix —, both entries against the
oracle with the switch on (bytes, count, all 28 counters; nothing deferred where the case is in scope; fgx_debug_last_deep_indels), and one mixed stream through
fgx_run_bam.  The molecules are those of tests/deep_indel_cases.py, a few hundred records each.  Without the feature the library has none of the three exports and
the device entry defers every such molecule."""
import os

import numpy as np
import pytest

import deep_indel_cases as D
from isolated import run_isolated

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name, option_set=-1):
    key = (name, option_set)
    if key not in _CASES:
        case = D.CASES[name]()
        if option_set >= 0:
            case = D.with_option_set(case, option_set)
            case.in_scope = D.canonical(D.options_of(case), case.recs)["status"] == 0       # (the option set decides; the comparison is the test)
        _CASES[key] = case
    return _CASES[key]


@pytest.fixture
def switch_on(monkeypatch):
    monkeypatch.setenv("FGX_DEEP_INDELS", "1")


@pytest.mark.parametrize("name", list(D.CASES))
def test_kernel_against_the_scalar_form(name):
    D.check_kernel_against_scalar(_case(name))


@pytest.mark.parametrize("name", ["130_records", "prefixes", "nibbles_insert_141", "first_record_dropped_same_cb"])
@pytest.mark.parametrize("option_set", [0, 1, 2])
def test_kernel_against_the_scalar_form_under_the_option_sets(name, option_set):
    D.check_kernel_against_scalar(_case(name, option_set))


@pytest.mark.parametrize("name", list(D.CASES))
def test_end_to_end(switch_on, name):
    D.check_end_to_end(_case(name))


@pytest.mark.parametrize("name", ["130_records", "nibbles_insert_150", "drops_to_64"])
@pytest.mark.parametrize("option_set", [0, 1, 2])
def test_end_to_end_under_the_option_sets(switch_on, name, option_set):
    D.check_end_to_end(_case(name, option_set))


def test_switch_unset_defers_as_before(monkeypatch):
    """Unset and "0": the molecule is deferred by the device entry (the host entry's bytes are the oracle's); "1": decided."""
    case = _case("130_records")
    o = D.options_of(case)
    g = D.grouped(case.recs)
    want = D.want_of(o, g)
    c = D.Caller(o)
    try:
        for value, on in ((None, False), ("1", True), ("0", False)):
            if value is None:
                monkeypatch.delenv("FGX_DEEP_INDELS", raising=False)
            else:
                monkeypatch.setenv("FGX_DEEP_INDELS", value)
            got = c.device(g)
            if on:
                assert got["deferred"] == 0 and got["deep_indels"] == 1 and got["canon"] == 1, (value, got["deferred"], got["deep_indels"])
                D.assert_equal(got, want, "device entry")
            else:
                assert got["deferred"] == 1 and got["deep_indels"] == 0 and got["canon"] == 0, (value, got["deferred"], got["deep_indels"])
                D.assert_equal(c.host(g), want, "host entry")
    finally:
        c.close()


def mixed_stream():
    """2 000 shallow molecules around three deep indel ones (66, 130 and 510 records; MI values of their own).  The filter leaves the first one 64 records, which
    the second pass's k_family_wave<1> decides; the other two are the deep kernels'."""
    from fgumi_amd import GroupedReads, simulate_grouped_reads
    small = simulate_grouped_reads(2000, duplex=1, family_size=1, family_size_max=5, error_rate_ppm=5000)
    deep = [D.molecule(31, 17, 16, major=D.DEL, minority={4: D.INS}, g=91, mi=900001), D.molecule(32, 33, 32, major=D.INS, g=92, mi=900002, err=D.DEEP_ERR),
            D.molecule(33, 128, 127, major=D.CLIP_DEL, minority={9: D.DEL, 200: D.DEL}, g=93, mi=900003, err=D.DEEP_ERR)]
    groups = [small.records(i) for i in range(1000)] + deep + [small.records(i) for i in range(1000, 2000)]
    return GroupedReads.from_groups([[bytes(r) for r in recs] for recs in groups])


def check_run_bam(tmp_dir):
    """(child interpreter, FGX_DEEP_INDELS=1) fgx_run_bam on the mixed stream: the oracle's records in order, no group deferred, no batch through the host entry."""
    import fgx_opts
    from fgumi_amd import DuplexConsensusCaller, bgzf
    g = mixed_stream()
    want = D.want_of(fgx_opts.defaults(kind=1), g)
    c = DuplexConsensusCaller("", "A", [1, 1, 0], cell_tag="CB", overlapping_consensus=True)
    refs = [("chr%d" % (i + 1), 2147483647) for i in range(24)]
    src, dst = os.path.join(tmp_dir, "grouped.bam"), os.path.join(tmp_dir, "consensus.bam")
    bgzf.write_bam(src, bgzf.grouped_input_header(refs), refs, g.blob)
    st = c.run_bam(src, dst, chunk_raw_bytes=0, threads=8, strip_strand_suffix=True)
    _, _, stream, off, ln = bgzf.read_bam(dst)
    got = b"".join(bytes(stream[int(a) - 4:int(a) + int(b)]) for a, b in zip(off, ln))
    print(f"chunks {st['chunks']}, deferred groups {st['deferred_groups']}, host entry batches {st['host_entry_batches']}, deep indel molecules {c.last_deep_indel_molecules()}", flush=True)
    D.assert_equal(dict(data=got, count=len(off), stats=np.array(st["stats"][:28], dtype=np.uint64)), want, "the consensus BAM")
    assert st["deferred_groups"] == 0 and st["host_entry_batches"] == 0, (st["deferred_groups"], st["host_entry_batches"])
    assert c.last_deep_indel_molecules() == 2
    c.close()


def test_mixed_stream_run_bam(tmp_path):
    run_isolated("test_gpu_deep_indels", "check_run_bam", str(tmp_path), env={"FGX_DEEP_INDELS": "1"}, timeout=600)
