"""--max-reads-per-strand decided by the device-resident pipeline on the GPU: the batches of tests/test_wavemu_strand_cap.py at 20 000 molecules through
DuplexConsensusCaller / CodecConsensusCaller.process_batch_device (nothing deferred, bytes and counters against the oracle), once more between guard bands
(the all-reads observation counts are a new device buffer), a duplex `--rejects` batch under a cap, fgx_run_bam on capped files (no batch through the host
entry) and the cap-off run of the same batch.  Every case runs in a child interpreter under its own time limit."""
import ctypes as C

import numpy as np
import pytest

import fgx_opts
import orc
from isolated import run_isolated

pytestmark = pytest.mark.gpu

N = 20000
DUPLEX_SIM = dict(family_size=12, duplex=1)
CODEC_SIM = dict(family_size=4, read_length=300, insert_mean=350, insert_sd=60, codec=1)
REJ_DOWNSAMPLED = 19          # FGX_REJ_DOWNSAMPLED (include/fgumi_amd.h)


def _caller_and_options(kind, cap, min_reads=(1, 1, 0), track_rejects=False):
    from fgumi_amd import CodecConsensusCaller, CodecConsensusOptions, DuplexConsensusCaller
    if kind == 1:
        c = DuplexConsensusCaller("", "A", list(min_reads), cell_tag="CB", overlapping_consensus=True, max_reads_per_strand=cap, track_rejects=track_rejects)
        o = fgx_opts.defaults(kind=1, duplex_max_reads_per_strand=-1 if cap is None else cap, duplex_min_reads=tuple(min_reads), track_rejects=int(track_rejects))
    else:
        c = CodecConsensusCaller("", "A", CodecConsensusOptions(max_reads_per_strand=cap, produce_per_base_tags=True, cell_tag="CB"))
        o = fgx_opts.defaults(kind=2, codec_max_reads_per_strand=-1 if cap is None else cap, overlapping_consensus=0)
    return c, o


def _look(what):
    from fgumi_amd import lib
    lib.fgx_debug_check_guard_bands.restype = C.c_int
    lib.fgx_debug_check_guard_bands.argtypes = [C.c_char_p, C.c_int]
    msg = C.create_string_buffer(600)
    bad = lib.fgx_debug_check_guard_bands(msg, 600)
    assert bad == 0, f"{what}: {bad} device buffer(s) written outside their bounds: {msg.value.decode()}"


def check_device_batch(kind, cap, min_reads=(1, 1, 0), n=N, guard=False):
    """`n` simulate-shaped molecules generated in HBM, the records left in HBM: nothing deferred, bytes, count and the 28 counters equal the oracle's."""
    from fgumi_amd import simulate_grouped_reads
    sim = DUPLEX_SIM if kind == 1 else CODEC_SIM
    c, o = _caller_and_options(kind, cap, min_reads)
    dg = c.simulate_on_device(n, **sim)
    out = c.process_batch_device(dg)
    data = out.to_host()
    stats = list(c.last_stats_array)
    if guard:
        _look(f"kind {kind} cap {cap}")
    g = simulate_grouped_reads(n, **sim)
    want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=100 if kind == 1 else 1000)
    print(f"kind {kind} cap {cap} min_reads {min_reads}: deferred {out.n_deferred} of {n}, records {out.count} / {want['count']}, downsampled {int(want['stats'][3 + REJ_DOWNSAMPLED])}", flush=True)
    assert out.n_deferred == 0, f"{out.n_deferred} of {n} molecules deferred"
    if data != want["data"]:
        import bamutil
        from fgumi_amd import split_records
        got_recs, want_recs = split_records(data), split_records(want["data"])
        bad = [i for i, (x, y) in enumerate(zip(got_recs, want_recs)) if x != y]
        raise AssertionError(f"{len(bad)} of {len(want_recs)} records differ (got {len(got_recs)}); first, record {bad[0] if bad else -1}:\n got {bamutil.parse(got_recs[bad[0]]) if bad else None}\nwant {bamutil.parse(want_recs[bad[0]]) if bad else None}")
    assert out.count == want["count"]
    assert stats[:28] == [int(v) for v in want["stats"]], (stats[:28], want["stats"].tolist())
    if kind == 2 and cap is not None:
        assert int(want["stats"][3 + REJ_DOWNSAMPLED]) > 0
    c.close()


def check_under_guard_bands():
    """(FGX_GUARD_BAND set) the capped batches once more, every guarded buffer verified after each."""
    from fgumi_amd import lib
    lib.fgx_debug_guarded_buffers.restype = C.c_int
    check_device_batch(1, 3, n=4000, guard=True)
    check_device_batch(1, 1, n=4000, guard=True)
    check_device_batch(2, 2, n=4000, guard=True)
    assert lib.fgx_debug_guarded_buffers() >= 20, lib.fgx_debug_guarded_buffers()


def check_duplex_rejects_under_a_cap():
    """`--rejects` with a duplex cap: the reject set does not depend on the cap, so the side kernels serve the batch — nothing deferred, records, rejects and
    counters equal the oracle's, and the cap bites molecules of the batch."""
    import test_gpu_zz_rejects_device as tgr
    from test_wavemu_strand_cap import set_sizes
    from fgumi_amd._lib import Options, Output, hip_memcpy_d2h, lib
    import torch
    g = tgr.strand_batch("duplex", 23)
    assert sum(1 for c in set_sizes(g) if max(c.values()) > 2) > 50
    o = tgr.strand_options("duplex", dict(duplex_min_reads=(3, 2, 1)))
    o.duplex_max_reads_per_strand = 2
    want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=100000)
    assert want["n_rejects"] > 0 and want["count"] > 0
    po = Options.from_buffer_copy(bytes(o))
    po.device = 0
    h = lib.fgx_create(C.byref(po))
    assert h, lib.fgx_global_error().decode()
    try:
        dg = g.to_device(0)
        torch.cuda.synchronize()
        fetch = lambda p, n: hip_memcpy_d2h(p, int(n)) if n else b""
        out, nd, dp = Output(), C.c_uint32(), C.c_void_p()
        rc = lib.fgx_process_batch_device(h, dg.blob.data_ptr(), dg.blob_len, dg.rec_off.data_ptr(), dg.rec_len.data_ptr(), dg.n_rec, dg.grp_first.data_ptr(), dg.n_grp,
                                          C.byref(out), C.byref(nd), C.byref(dp))
        assert rc == 0, lib.fgx_last_error(h).decode()
        assert nd.value == 0, f"{nd.value} molecules deferred by the device entry"
        assert int(out.n_rejects) == want["n_rejects"] and fetch(out.rejects, out.rejects_len) == want["rejects"]
        assert fetch(out.data, out.data_len) == want["data"] and int(out.count) == want["count"]
        assert np.array_equal(np.array(list(out.stats), dtype=np.uint64), want["stats"])
    finally:
        lib.fgx_destroy(h)


def check_run_bam(kind, cap, tmp_dir, n=3000):
    """fgx_run_bam on a capped file, in one chunk and in many: the consensus BAM's records and the counters equal the oracle's, no group deferred and no batch
    through the host entry."""
    import os
    from fgumi_amd import bgzf, simulate_grouped_reads
    g = simulate_grouped_reads(n, **(DUPLEX_SIM if kind == 1 else CODEC_SIM))
    c, o = _caller_and_options(kind, cap)
    want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=100000)
    refs = [("chr%d" % (i + 1), 2147483647) for i in range(24)]
    src, dst = os.path.join(tmp_dir, "grouped.bam"), os.path.join(tmp_dir, "consensus.bam")
    bgzf.write_bam(src, bgzf.grouped_input_header(refs), refs, g.blob)
    for chunk in (0, 1 << 20):
        st = c.run_bam(src, dst, chunk_raw_bytes=chunk, threads=8, strip_strand_suffix=(kind == 1))
        _, _, stream, off, ln = bgzf.read_bam(dst)
        got = b"".join(bytes(stream[int(a) - 4:int(a) + int(b)]) for a, b in zip(off, ln))
        print(f"kind {kind} cap {cap} chunk {chunk}: chunks {st['chunks']}, deferred groups {st['deferred_groups']}, host entry batches {st['host_entry_batches']}", flush=True)
        assert got == want["data"], "the consensus BAM's records differ from the oracle's"
        assert st["stats"][:28] == [int(v) for v in want["stats"]]
        assert st["deferred_groups"] == 0 and st["host_entry_batches"] == 0, (st["deferred_groups"], st["host_entry_batches"])
    c.close()


def check_per_field_writer_cap_build():
    """k_emit_duplex<0, 1> — the per-field writer's CAP build — with a record whose recount reads the all-reads counts: the crafted molecule of
    tests/test_wavemu_strand_cap.py whose dropped read is the only one that disagrees, under a 70-character prefix, decided on the device."""
    import bamutil
    from fgumi_amd import split_records
    from test_gpu_duplex_methylation_device import same_through_the_host_entry
    from test_wavemu_record_writers import cap_changes_the_recount, capped_molecule, writer_counts
    g = capped_molecule()
    kw = dict(kind=1, read_name_prefix=b"k" * 70)
    got, want = same_through_the_host_entry(fgx_opts.defaults(duplex_max_reads_per_strand=2, **kw), None, g)
    assert got["deferred"] == 0, got
    assert writer_counts(want["data"]) == (0, want["count"])
    off = orc.process(fgx_opts.defaults(**kw), g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=100)
    cap_changes_the_recount(*([bamutil.parse(r) for r in split_records(w["data"])] for w in (want, off)))


@pytest.mark.parametrize("cap,min_reads", [(1, (1, 1, 0)), (3, (1, 1, 0)), (4, (3, 2, 1))], ids=["cap1", "cap3", "cap4_min_3_2_1"])
def test_duplex_cap_on_the_device(cap, min_reads):
    run_isolated("test_gpu_strand_cap", "check_device_batch", 1, cap, min_reads, timeout=600)


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_codec_cap_on_the_device(cap):
    run_isolated("test_gpu_strand_cap", "check_device_batch", 2, cap, timeout=600)


@pytest.mark.parametrize("kind", [1, 2], ids=["duplex", "codec"])
def test_cap_off_run_of_the_same_batch(kind):
    """The cap-off builds: the same batch without a cap equals the oracle's cap-off output."""
    run_isolated("test_gpu_strand_cap", "check_device_batch", kind, None, timeout=600)


def test_capped_batches_under_guard_bands():
    run_isolated("test_gpu_strand_cap", "check_under_guard_bands", env={"FGX_GUARD_BAND": "4096"}, timeout=600)


def test_duplex_rejects_under_a_cap_stay_on_the_device():
    run_isolated("test_gpu_strand_cap", "check_duplex_rejects_under_a_cap", timeout=600)


@pytest.mark.parametrize("kind,cap", [(1, 3), (2, 2)], ids=["duplex", "codec"])
def test_run_bam_on_a_capped_file(kind, cap, tmp_path):
    run_isolated("test_gpu_strand_cap", "check_run_bam", kind, cap, str(tmp_path), timeout=600)


def test_long_read_name_prefix_takes_the_per_field_writer_cap_build():
    run_isolated("test_gpu_strand_cap", "check_per_field_writer_cap_build", timeout=600)
