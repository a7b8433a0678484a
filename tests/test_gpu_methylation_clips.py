"""GPU: soft- / hard-clipped reads in the methylation-aware mode (EM-Seq / TAPs) decided by the device-resident pipeline — the clip-taking build of
the streaming record kernel in its three size classes (k_deep_parse<64, 64, 1>, <256, DEEP_MAX, 1>, <256, DEEP_CAP_MAX, 1>) for the simplex caller,
k_family_wave<1, 1> for the duplex caller — through every entry: fgx_process_batch_device, fgx_process_batch (device pass + deferred subset),
run_bam.  The oracle is the arbiter: bytes, record count, the 28 counters.

The `M` / `S` batches and the crafted families are those of tests/test_wavemu_methylation_clips.py (tests/methclip_cases.py) at a larger size; before
this change every group with a clipped record was deferred, so `deferred == 0` and the fgx_debug_last_meth_clipped count fail on that code."""
import ctypes as C

import numpy as np
import pytest

import bamutil
import methclip_cases as mc
import methsim
from fgumi_amd import DuplexConsensusCaller, GroupedReads, MethylationMode, VanillaUmiConsensusCaller, VanillaUmiConsensusOptions, lib
from isolated import run_isolated

pytestmark = pytest.mark.gpu

SIMPLEX_N, DUPLEX_N = 1500, 1200


# ---- 1. the M / S batches, both entries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("mode,kw", [(1, {}), (2, {}), (1, dict(max_reads=3))], ids=["em_seq", "taps", "em_seq_max_reads_3"])
def test_simplex_clipped_families(mode, kw, entry):
    mc.check_ms_batch(0, mode, 1, SIMPLEX_N, 80 + mode + (2 if kw else 0), entry, True, kw)


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("mode,min_reads", [(1, (1, 1, 0)), (2, (1, 1, 0)), (1, (3, 2, 1))], ids=["em_seq_1_1_0", "taps_1_1_0", "em_seq_3_2_1"])
def test_duplex_clipped_molecules(mode, min_reads, entry):
    mc.check_ms_batch(1, mode, min_reads, DUPLEX_N, 84 + mode, entry, True)


@pytest.mark.parametrize("entry", ["device", "host"])
@pytest.mark.parametrize("kind", [0, 1], ids=["simplex", "duplex"])
def test_crafted_families(kind, entry):
    mc.check_crafted(kind, entry, True)


@pytest.mark.parametrize("kind", [0, 1], ids=["simplex", "duplex"])
def test_plain_groups_count_no_clipped_family(kind):
    mc.check_plain_counts_nothing(kind, "device", True)


# ---- 2. the larger size classes of the record kernel ---------------------------------------------------------------------------------------
def test_deep_families_with_a_third_of_the_reads_clipped():
    """Families of 70 .. 150 records: the <64, 64, 1> build hands them to <256, DEEP_MAX, 1>."""
    rng = methsim.seeded(93)
    contigs = methsim.genome(rng)
    groups = mc.simplex_ms_groups(rng, contigs, 24, depth=(70, 75), read_len=(60, 120), per_read_clip=1 / 3, layouts=("frag", "frag_rev"), long_names=True) + \
        mc.simplex_ms_groups(rng, contigs, 24, depth=(35, 75), read_len=(60, 120), per_read_clip=1 / 3, layouts=("pair", "pair_overlap"), long_names=True)
    assert all(70 <= len(g) <= 150 for g in groups)
    n_reads = sum(len(g) for g in groups)
    assert n_reads / 4 < sum(mc.multi_op(r) for g in groups for r in g) < n_reads / 2
    mc.check_all_on_device(mc.options(0, 1), contigs, groups, mc.n_clipped_groups(groups), "device", True, min_mm=20)


def test_a_family_of_600_records_under_max_reads():
    """600 records, --max-reads 50: beyond DEEP_MAX, so <256, DEEP_CAP_MAX, 1> takes it (with a few small families around it)."""
    rng = methsim.seeded(94)
    contigs = methsim.genome(rng)
    groups = mc.simplex_ms_groups(rng, contigs, 3, depth=(2, 6)) + \
        mc.simplex_ms_groups(rng, contigs, 1, depth=(600, 600), read_len=(60, 120), per_read_clip=1 / 3, layouts=("frag",), long_names=True)
    assert len(groups[3]) == 600 and 150 < sum(mc.multi_op(r) for r in groups[3]) < 250
    mc.check_all_on_device(mc.options(0, 1, max_reads=50), contigs, groups, mc.n_clipped_groups(groups), "device", True, min_mm=2)


# ---- 3. the unfiltered methsim batches: indel reads stay deferred, clip-only groups do not -------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1], ids=["simplex", "duplex"])
def test_unfiltered_batches_defer_indel_groups_only(kind):
    from fgumi_amd import GroupedReads
    rng = methsim.seeded(70 + kind)
    contigs = methsim.genome(rng)
    groups = methsim.duplex_groups(rng, contigs, 1200) if kind == 1 else methsim.simplex_groups(rng, contigs, 1500)
    g = GroupedReads.from_groups(groups)
    indel = {i for i, grp in enumerate(groups) if any(mc.has_indel(r) for r in grp)}
    clip_only = {i for i, grp in enumerate(groups) if i not in indel and any(mc.multi_op(r) for r in grp)}
    assert len(indel) > 50 and len(clip_only) > 50, (len(indel), len(clip_only))
    o = mc.options(kind, 1)
    want = mc.oracle(o, contigs, g)
    got = mc.product(o, contigs, g, "device", True)
    deferred = set(got["deferred"])
    print(len(groups), "groups:", len(indel), "with an indel record,", len(clip_only), "clip-only,", len(deferred), "deferred,", got["meth_clipped"], "clipped and decided on the device")
    assert not (deferred & clip_only), sorted(deferred & clip_only)[:10]
    assert 0 < len(deferred) <= len(indel), (len(deferred), len(indel))
    assert deferred <= indel
    assert got["meth_clipped"] >= len(clip_only)
    # device pass + deferred subset through the host entry: the oracle's bytes
    host = mc.product(o, contigs, g, "host", True)
    assert host["count"] == want["count"]
    mc.assert_same_records(host["data"], want["data"])
    assert np.array_equal(host["stats"], want["stats"])
    assert 0 < host["n_deferred"] <= len(indel)


# ---- 4. file -> file ------------------------------------------------------------------------------------------------------------------------
def _run_bam(c, contigs, groups, o, tmp_path, **kw):
    from fgumi_amd import bgzf
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
        counts = c.last_methylation_device_counts()
        assert counts["on_device"] > 0 and counts["clipped"] > 0, counts       # (the last chunk's batch: half its groups are clipped)
    finally:
        c.close()


def test_run_bam_simplex_keeps_clipped_families_on_the_device(tmp_path):
    rng = methsim.seeded(95)
    contigs = methsim.genome(rng)
    groups = [g for g in mc.simplex_ms_groups(rng, contigs, 800) if bamutil.parse(g[0])["ref_id"] < len(contigs)]   # (a BAM file names header contigs only)
    assert mc.n_clipped_groups(groups) > len(groups) // 3
    c = VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(min_reads=1, min_consensus_base_quality=2, cell_tag="CB", methylation_mode=MethylationMode.EmSeq),
                                  overlapping_consensus=True)
    _run_bam(c, contigs, groups, mc.options(0, 1), tmp_path)


def test_run_bam_duplex_keeps_clipped_molecules_on_the_device(tmp_path):
    contigs, groups, _ = mc.ms_batch(1, 800, 96)
    c = DuplexConsensusCaller("", "A", [1, 1, 0], cell_tag="CB", overlapping_consensus=True, produce_per_base_tags=True, methylation_mode=MethylationMode.EmSeq)
    _run_bam(c, contigs, groups, mc.options(1, 1), tmp_path, strip_strand_suffix=True)


# ---- 5. guard bands -------------------------------------------------------------------------------------------------------------------------
def check_under_guard_bands():
    """(child interpreter, FGX_GUARD_BAND set) The M / S batches, then a look at every guarded buffer."""
    lib.fgx_debug_check_guard_bands.restype = C.c_int
    lib.fgx_debug_check_guard_bands.argtypes = [C.c_char_p, C.c_int]
    lib.fgx_debug_guarded_buffers.restype = C.c_int
    for kind, n, seed in ((0, SIMPLEX_N, 81), (1, DUPLEX_N, 85)):
        mc.check_ms_batch(kind, 1, None, n, seed, "device", True)
        msg = C.create_string_buffer(600)
        bad = lib.fgx_debug_check_guard_bands(msg, 600)
        assert bad == 0, f"kind {kind}: {bad} device buffer(s) written outside their bounds: {msg.value.decode()}"
    assert lib.fgx_debug_guarded_buffers() >= 10, lib.fgx_debug_guarded_buffers()


def test_clip_taking_kernels_under_guard_bands():
    run_isolated("test_gpu_methylation_clips", "check_under_guard_bands", env={"FGX_GUARD_BAND": "4096"}, timeout=900)
