"""GPU: the duplex caller's methylation-aware mode (EM-Seq / TAPs) under --max-reads-per-strand in the device-resident pipeline — k_family_wave<1, 1, 1>,
k_emit_duplex_fast<1, 1> / k_emit_duplex<1, 1>, the tag kernels of duplex_meth.inc — through `DuplexConsensusCaller.process_batch_device`, `run_bam` and the
host entry: nothing deferred, bytes, record count and the 28 counters equal the oracle's (tests/orc.py with `orc.set_reference`).  The batches and the
crafted molecules are those of tests/test_wavemu_duplex_meth_cap.py; every case runs in a child interpreter under its own time limit."""
import ctypes as C

import numpy as np
import pytest

from isolated import run_isolated

pytestmark = pytest.mark.gpu

N_GROUPS = 1200


def sim_batch(mode, n_groups=N_GROUPS):
    import test_wavemu_duplex_meth_cap as emu
    return emu.sim_batch(70 + mode, n_groups)


def device_entry(g, contigs, mode, cap, min_reads=(1, 1, 0), guard=False):
    """The batch through process_batch_device of a caller in the mode with the cap, against the oracle; returns the oracle's parsed records."""
    import bamutil
    import test_gpu_duplex_methylation_device as dev
    from fgumi_amd import lib, split_records
    want = dev.oracle(dev.options(mode, min_reads, duplex_max_reads_per_strand=cap), contigs, g)
    c = dev.caller(mode, min_reads, contigs, max_reads_per_strand=cap)
    try:
        out = c.process_batch_device(g.to_device())
        assert out.n_deferred == 0, f"{out.n_deferred} of {g.n_grp} molecules deferred"
        assert out.count == want["count"]
        dev.assert_same_records(out.to_host(), want["data"])
        assert np.array_equal(np.array(c.last_stats_array, dtype=np.uint64), want["stats"]), (c.last_stats_array, want["stats"].tolist())
        assert lib.fgx_debug_last_meth_device(c._h) == g.n_grp
        if guard:
            lib.fgx_debug_check_guard_bands.restype = C.c_int
            lib.fgx_debug_check_guard_bands.argtypes = [C.c_char_p, C.c_int]
            lib.fgx_debug_guarded_buffers.restype = C.c_int
            msg = C.create_string_buffer(600)
            bad = lib.fgx_debug_check_guard_bands(msg, 600)
            assert bad == 0, f"{bad} device buffer(s) written outside their bounds: {msg.value.decode()}"
            assert lib.fgx_debug_guarded_buffers() >= 10, lib.fgx_debug_guarded_buffers()
    finally:
        c.close()
    return [bamutil.parse(r) for r in split_records(want["data"])]


# ---- 1. the simulated batch, device-resident entry --------------------------------------------------------------------------------------------------------
def check_sim(mode, cap, guard=False):
    import test_wavemu_duplex_meth_cap as emu
    contigs, g = sim_batch(mode)
    assert g.n_grp > 700 and 2 * emu.cap_bites(g, cap) >= g.n_grp, (emu.cap_bites(g, cap), g.n_grp)
    tags = [r["tags"] for r in device_entry(g, contigs, mode, cap, guard=guard)]
    assert sum("au" in t and "bu" in t for t in tags) > 300 and sum("MM" in t for t in tags) > 300, len(tags)


@pytest.mark.parametrize("mode", [1, 2], ids=["em_seq", "taps"])
@pytest.mark.parametrize("cap", [1, 3])
def test_capped_molecules_through_the_device_resident_entry(mode, cap):
    run_isolated("test_gpu_duplex_meth_cap", "check_sim", mode, cap, timeout=600)


def test_capped_batch_under_guard_bands():
    run_isolated("test_gpu_duplex_meth_cap", "check_sim", 1, 3, True, env={"FGX_GUARD_BAND": "4096"}, timeout=600)


# ---- 2. the crafted molecules ---------------------------------------------------------------------------------------------------------------------------
def check_crafted():
    """The crafted molecules of the emulator file as two batches — a cap of 2, and a cap of 4 for the five-read pin and the cap that does not bite —, the
    oracle's records of each molecule held against the emulator file's expectations."""
    import test_wavemu_duplex_meth_cap as emu
    from fgumi_amd import GroupedReads
    ref, EM = emu.crafted_genome(), emu.EM
    cap2 = [emu.crafted_a("1"), emu.crafted_b(mi="2"), emu.crafted_b(agree=True, mi="3"), emu.crafted_c("4"), emu.crafted_d(True, "5"), emu.crafted_d(False, "6"),
            emu.crafted_g(5, "7"), emu.crafted_h("8")]
    w = device_entry(GroupedReads.from_groups([emu.records_of(m) for m in cap2]), ref, 1, 2)
    assert len(w) == 2 * len(cap2)
    of = lambda i: w[2 * i:2 * i + 2]
    emu.expect_dropped_read_carries_the_conversion(of(0), emu.oracle_only(cap2[0], ref, duplex_max_reads_per_strand=2)[0])
    emu.expect_dropped_read_counts_in_the_recount(of(1), of(2))
    emu.expect_longest_read_dropped(of(3), emu.oracle_only(cap2[3], ref, **EM)[0])
    emu.expect_anchor_over_all_reads(of(4), of(5))
    emu.expect_no_annotation_outside_the_genome(of(6), emu.oracle_only(emu.crafted_g(0), ref, duplex_max_reads_per_strand=2, **EM)[0])
    emu.expect_reverse_set(of(7), emu.oracle_only(cap2[7], ref, duplex_max_reads_per_strand=2)[0])
    g_file, g_rank, g_five = emu.crafted_e("9")
    cap4 = [g_five, emu.crafted_f("10")]
    w = device_entry(GroupedReads.from_groups([emu.records_of(m) for m in cap4]), ref, 1, 4)
    emu.expect_rank_order_is_the_summation_order(w[0:2], emu.oracle_only(g_file, ref, **EM)[0], emu.oracle_only(g_rank, ref, **EM)[0])
    off, _ = emu.oracle_only(cap4[1], ref, **EM)
    assert w[2:4] == off and "MM" in off[0]["tags"]                   # a cap above the largest set: the cap-off run of the mode


def test_crafted_molecules():
    run_isolated("test_gpu_duplex_meth_cap", "check_crafted", timeout=600)


def check_per_field_writer():
    """k_emit_duplex<1, 1>: the crafted molecules whose dropped read alone carries the conversion, under a 70-character read-name prefix, through the host entry."""
    import bamutil
    import test_gpu_duplex_methylation_device as dev
    import test_wavemu_duplex_meth_cap as emu
    from fgumi_amd import GroupedReads, split_records
    from test_wavemu_record_writers import writer_counts
    g = GroupedReads.from_groups([emu.records_of(emu.crafted_a("1")), emu.records_of(emu.crafted_h("2"))])
    got, want = dev.same_through_the_host_entry(dev.options(1, (1, 1, 0), duplex_max_reads_per_strand=2, read_name_prefix=b"k" * 70), emu.crafted_genome(), g)
    assert got["meth_device"] == g.n_grp and got["deferred"] == 0, got
    assert writer_counts(want["data"]) == (0, want["count"]) and want["count"] == 4
    assert all(bamutil.parse(r)["tags"]["cE"][1] == 0.0 for r in split_records(want["data"]))          # (the recount reads the normalised all-reads counts)


def test_long_read_name_prefix_takes_the_per_field_writer():
    run_isolated("test_gpu_duplex_meth_cap", "check_per_field_writer", timeout=600)


# ---- 3. file -> file --------------------------------------------------------------------------------------------------------------------------------------
def check_run_bam(tmp_dir, cap=2, n_groups=600):
    import os
    import test_gpu_duplex_methylation_device as dev
    from fgumi_amd import bgzf
    contigs, g = sim_batch(1, n_groups)
    want = dev.oracle(dev.options(1, (1, 1, 0), duplex_max_reads_per_strand=cap), contigs, g)
    assert b"MM" in want["data"] and b"bu" in want["data"]
    names = [f"chr{i + 1}" for i in range(len(contigs))]
    refs = [(n, len(s)) for n, s in zip(names, contigs)]
    src, dst = os.path.join(tmp_dir, "grouped.bam"), os.path.join(tmp_dir, "consensus.bam")
    bgzf.write_bam(src, bgzf.grouped_input_header(refs), refs, g.blob)
    c = dev.caller(1, (1, 1, 0), contigs, max_reads_per_strand=cap)
    try:
        for chunk in (0, 1 << 16):
            st = c.run_bam(src, dst, chunk_raw_bytes=chunk, threads=8, strip_strand_suffix=True)
            _, _, stream, off, ln = bgzf.read_bam(dst)
            got = b"".join(bytes(stream[int(o_) - 4:int(o_) + int(l)]) for o_, l in zip(off, ln))
            print(f"chunk {chunk}: chunks {st['chunks']}, deferred groups {st['deferred_groups']}, host entry batches {st['host_entry_batches']}", flush=True)
            assert chunk == 0 or st["chunks"] > 1, st["chunks"]
            dev.assert_same_records(got, want["data"])
            assert st["consensus_records"] == want["count"]
            assert st["stats"][:len(want["stats"])] == [int(v) for v in want["stats"]]
            assert st["host_entry_batches"] == 0 and st["deferred_groups"] == 0, (st["host_entry_batches"], st["deferred_groups"])
    finally:
        c.close()


def test_run_bam_on_a_capped_file_in_the_mode(tmp_path):
    run_isolated("test_gpu_duplex_meth_cap", "check_run_bam", str(tmp_path), timeout=600)


# ---- 4. host entry ----------------------------------------------------------------------------------------------------------------------------------------
def check_host_entry(mode, cap):
    import test_gpu_duplex_methylation_device as dev
    contigs, g = sim_batch(mode)
    got, _ = dev.same_through_the_host_entry(dev.options(mode, (1, 1, 0), duplex_max_reads_per_strand=cap), contigs, g)
    assert got["meth_device"] == g.n_grp and got["deferred"] == 0, got


def test_one_op_batch_through_the_host_entry():
    run_isolated("test_gpu_duplex_meth_cap", "check_host_entry", 1, 2, timeout=600)
