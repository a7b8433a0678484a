"""GPU: indel reads in the methylation-aware mode (EM-Seq / TAPs) of the duplex and the simplex caller, decided by the device pipeline through the canonical
second pass (FGX_METH_CANON=1) — canon_device.hip emitting every canonical record's reference runs, k_family_wave<1, 1> (duplex) and k_deep_parse<.., .., 1> /
k_deep_cols<1> (simplex) looking the reference base up through the anchor's runs — through every entry: fgx_process_batch_device (the pass runs where the records lie), fgx_process_batch (device pass + second pass +
what is left through the general path), run_bam.  The oracle is the arbiter: bytes, record count, the 28 counters.

The batches and the crafted molecules are those of tests/test_wavemu_methylation_indels.py (tests/methindel_cases.py) at a larger size.  The library
reads the switch per call.  Without this change it ignores the switch: nothing is canonicalised, and every switch-on test fails."""
import numpy as np
import pytest

import methclip_cases as mc
import methindel_cases as mi
from fgumi_amd import DuplexConsensusCaller, GroupedReads, MethylationMode, VanillaUmiConsensusCaller, VanillaUmiConsensusOptions

pytestmark = pytest.mark.gpu

SIMPLEX_N, DUPLEX_N = 1500, 1200


@pytest.fixture
def switch_on(monkeypatch):
    monkeypatch.setenv("FGX_METH_CANON", "1")


@pytest.fixture
def switch_unset(monkeypatch):
    monkeypatch.delenv("FGX_METH_CANON", raising=False)


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("mode", [1, 2], ids=["em_seq", "taps"])
def test_duplex_indel_molecules(switch_on, mode, entry):
    mi.check_duplex_batch(mode, (1, 1, 0), DUPLEX_N, 60 + mode, entry, True)


@pytest.mark.parametrize("entry", ["device", "host"])
def test_duplex_indel_molecules_under_min_reads_3_2_1(switch_on, entry):
    mi.check_duplex_batch(1, (3, 2, 1), DUPLEX_N, 63, entry, True, shared=True)


def test_duplex_indel_molecules_canonicalised_on_the_host_cores(switch_on, monkeypatch):
    monkeypatch.setenv("FGX_CANON_DEVICE", "0")
    mi.check_duplex_batch(1, (1, 1, 0), DUPLEX_N, 61, "host", True)


@pytest.mark.parametrize("entry", ["device", "host"])
def test_crafted_duplex_molecules(switch_on, entry):
    mi.check_crafted(entry, True)


@pytest.mark.parametrize("entry", ["device", "host"])
def test_switch_unset_keeps_indel_molecules_deferred(switch_unset, entry):
    """... and the host entry gives the oracle's bytes through the general path, as before."""
    mi.check_duplex_batch(1, (1, 1, 0), DUPLEX_N, 61, entry, True, switch=False)


def test_switch_set_to_zero_is_off(monkeypatch):
    monkeypatch.setenv("FGX_METH_CANON", "0")
    mi.check_duplex_batch(1, (1, 1, 0), 300, 61, "device", True, switch=False)


# ---- simplex --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("mode,kw", [(1, {}), (2, {}), (1, dict(max_reads=3))], ids=["em_seq", "taps", "em_seq_max_reads_3"])
def test_simplex_indel_families(switch_on, mode, kw, entry):
    mi.check_simplex_batch(mode, SIMPLEX_N, 70 + mode + (2 if kw else 0), entry, True, kw=kw)


def test_simplex_indel_families_canonicalised_on_the_host_cores(switch_on, monkeypatch):
    monkeypatch.setenv("FGX_CANON_DEVICE", "0")
    mi.check_simplex_batch(1, SIMPLEX_N, 71, "host", True)


@pytest.mark.parametrize("entry", ["device", "host"])
def test_crafted_simplex_families(switch_on, entry):
    mi.check_crafted_simplex(entry, True)


@pytest.mark.parametrize("entry", ["device", "host"])
def test_switch_unset_keeps_indel_families_deferred(switch_unset, entry):
    mi.check_simplex_batch(1, SIMPLEX_N, 71, entry, True, switch=False)


def test_deep_families_with_an_indel_in_a_third_of_the_reads(switch_on):
    """Families of 100 .. 120 records (at most 128: in the form's scope); the canonical families keep more than 64 records, so the second pass runs the
    <256, DEEP_MAX, 1> build of the record kernel, with runs."""
    contigs, groups = mi.deep_indel_families(97)
    assert all(100 <= len(g) <= 120 for g in groups)
    n_reads = sum(len(g) for g in groups)
    assert n_reads / 4 < sum(mc.has_indel(r) for g in groups for r in g) < n_reads / 2
    # what pins the build: the record kernel's wavefront-sized build hands every family of more than 64 records on to <256, DEEP_MAX, 1> (`n > MAXR`), and the second
    # pass is given the CANONICAL families — so each of them must keep more than 64 records (and at most 128 came in)
    kept = mi.canonical_sizes(mc.options(0, 1), groups)
    assert all(k is not None and 64 < k <= 128 for k in kept), kept
    got, want, oos = mi.check_groups(mc.options(0, 1), contigs, groups, "device", True, min_mm=4, max_oos_share=0.0)      # (12 families, one record each)
    assert got["canon"] == len(groups)


# ---- file -> file ---------------------------------------------------------------------------------------------------------------------------
def _run_bam(c, contigs, groups, o, tmp_path, **kw):
    from fgumi_amd import bgzf
    indel = [i for i, grp in enumerate(groups) if any(mc.has_indel(r) for r in grp)]
    assert len(indel) > 80 and not mi.out_of_scope(o, groups, indel)          # the file's groups are all in the form's scope
    g = GroupedReads.from_groups(groups)
    want = mc.oracle(o, contigs, g)
    assert b"MM" in want["data"]
    names = [f"chr{i + 1}" for i in range(len(contigs))]
    refs = [(n, len(s)) for n, s in zip(names, contigs)]
    c.set_reference({n: bytes(s) for n, s in zip(names, contigs)}, names)
    src, dst = str(tmp_path / "grouped.bam"), str(tmp_path / "consensus.bam")
    bgzf.write_bam(src, bgzf.grouped_input_header(refs), refs, g.blob)
    try:
        for chunk in (0, 1 << 16):
            st = c.run_bam(src, dst, chunk_raw_bytes=chunk, threads=8, **kw)
            text, orefs, stream, off, ln = bgzf.read_bam(dst)
            got = b"".join(bytes(stream[int(o_) - 4:int(o_) + int(l)]) for o_, l in zip(off, ln))
            mc.assert_same_records(got, want["data"])
            assert st["consensus_records"] == want["count"]
            assert st["stats"][:len(want["stats"])] == [int(v) for v in want["stats"]]
            assert st["host_entry_batches"] == 0 and st["deferred_groups"] == 0, (st["host_entry_batches"], st["deferred_groups"])
    finally:
        c.close()


def test_run_bam_duplex_keeps_indel_molecules_on_the_device(switch_on, tmp_path):
    contigs, groups = mi.duplex_batch(800, 66)
    c = DuplexConsensusCaller("", "A", [1, 1, 0], cell_tag="CB", overlapping_consensus=True, produce_per_base_tags=True, methylation_mode=MethylationMode.EmSeq)
    _run_bam(c, contigs, groups, mc.options(1, 1), tmp_path, strip_strand_suffix=True)


def test_run_bam_simplex_keeps_indel_families_on_the_device(switch_on, tmp_path):
    contigs, groups = mi.simplex_batch(800, 76, in_header=True)
    c = VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(min_reads=1, min_consensus_base_quality=2, cell_tag="CB", methylation_mode=MethylationMode.EmSeq),
                                  overlapping_consensus=True)
    _run_bam(c, contigs, groups, mc.options(0, 1), tmp_path)
