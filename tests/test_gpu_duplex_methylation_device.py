"""GPU: the duplex caller's methylation-aware mode (EM-Seq / TAPs) decided by the device-resident pipeline — k_family_wave<1, 1> (anchor, reference
lookup, counts and normalisation per read set), the record writers' conversion-artifact rule, am/au/at, bm/bu/bt, MM/ML/cu/ct behind RX
(duplex_meth.inc) — through every entry: `DuplexConsensusCaller.process_batch_device`, `fgx_process_batch` (device pass + deferred subset on the general
path), `run_bam`.  The oracle (tests/orc.py with `orc.set_reference`) is the arbiter everywhere: bytes, record count, the 28 counters.

What the device takes in this mode: molecules whose records are each one aligned block (one CIGAR op); soft-clipped and indel reads, a per-strand cap
that bites and everything else the duplex kernel defers go to the general path, which knows the mode."""
import ctypes as C
import os

import numpy as np
import pytest

import bamutil
import fgx_opts
import methsim
import orc
from fgumi_amd import DuplexConsensusCaller, GroupedReads, MethylationMode, lib, simulate_grouped_reads, split_records
from fgumi_amd._lib import Options, Output
from isolated import run_isolated

pytestmark = pytest.mark.gpu

lib.fgx_debug_last_meth_device.restype = C.c_uint32
lib.fgx_debug_last_meth_device.argtypes = [C.c_void_p]
lib.fgx_debug_last_deferral.restype = None
lib.fgx_debug_last_deferral.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]


def n_ops(rec):
    return bamutil.parse(rec)["n_cigar"]


def batch(mode, plain, n_groups=1200):
    """tests/methsim.py's duplex batch of the mode's seed (the one tests/test_gpu_methylation.py uses); `plain`: only the groups whose records all
    have one CIGAR op."""
    rng = methsim.seeded(70 + mode)
    contigs = methsim.genome(rng)
    groups = methsim.duplex_groups(rng, contigs, n_groups)
    if plain:
        groups = [g for g in groups if all(n_ops(r) == 1 for r in g)]
    return contigs, groups


def options(mode, min_reads, **kw):
    o = fgx_opts.defaults(kind=1, methylation_mode=mode, **kw)
    o.duplex_min_reads[0], o.duplex_min_reads[1], o.duplex_min_reads[2] = min_reads
    return o


def oracle(o, contigs, g, batch_groups=100, threads=1):
    orc.set_reference(contigs)
    try:
        return orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=batch_groups, threads=threads)
    finally:
        orc.set_reference(None)


def caller(mode, min_reads, contigs, **kw):
    c = DuplexConsensusCaller("", "A", list(min_reads), cell_tag="CB", overlapping_consensus=bool(kw.pop("overlapping_consensus", 1)),
                              produce_per_base_tags=bool(kw.pop("produce_per_base_tags", 1)), methylation_mode=mode, **kw)
    names = [f"chr{i + 1}" for i in range(len(contigs))]
    c.set_reference({n: bytes(s) for n, s in zip(names, contigs)}, names)
    return c


def assert_same_records(got, want):
    if got != want:
        for i, (a, b) in enumerate(zip(split_records(got), split_records(want))):
            if a != b:
                raise AssertionError(f"record {i} differs:\n got {bamutil.parse(a)}\nwant {bamutil.parse(b)}")
        raise AssertionError(f"record count / length differs: {len(got)} bytes against {len(want)}")


def tag_counts(data, first=None):
    recs = [bamutil.parse(r)["tags"] for r in split_records(data)[:first]]
    return dict(records=len(recs), both=sum("au" in t and "bu" in t for t in recs), mm=sum("MM" in t for t in recs), ba_only=sum("bu" in t and "au" not in t for t in recs))


# ---- 1. plain molecules, device-resident entry ---------------------------------------------------------------------------------------------------------
def check_plain_device_entry(mode, min_reads, kw, guard=False):
    contigs, groups = batch(mode, plain=True)
    g = GroupedReads.from_groups(groups)
    want = oracle(options(mode, min_reads, **kw), contigs, g)
    n = tag_counts(want["data"])
    print("oracle:", len(groups), "groups", n)
    if tuple(min_reads) == (1, 1, 0):      # the oracle's records are not an empty comparison: two-strand, MM-carrying and BA-only (bm / bu / bt alone) records
        assert n["both"] > 1000 and n["mm"] > 800 and n["ba_only"] > 200, n
    else:
        assert n["both"] > 1000 and n["mm"] > 500, n
    c = caller(mode, min_reads, contigs, **kw)
    try:
        out = c.process_batch_device(g.to_device())
        assert out.n_deferred == 0, out.n_deferred
        assert out.count == want["count"]
        assert_same_records(out.to_host(), want["data"])
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


@pytest.mark.parametrize("mode,min_reads,kw", [
    (1, (1, 1, 0), {}), (2, (1, 1, 0), {}), (1, (3, 2, 1), {}), (2, (3, 2, 1), {}), (1, (1, 1, 0), dict(produce_per_base_tags=0, overlapping_consensus=0)),
], ids=["em_seq_1_1_0", "taps_1_1_0", "em_seq_3_2_1", "taps_3_2_1", "em_seq_no_per_base_tags_no_overlap"])
def test_plain_molecules_through_the_device_resident_entry(mode, min_reads, kw):
    check_plain_device_entry(mode, min_reads, kw)


# ---- 2. mixed batch, host entry --------------------------------------------------------------------------------------------------------------------------
def host_entry(o, contigs, g):
    po = Options.from_buffer_copy(bytes(o))
    h = lib.fgx_create(C.byref(po))
    assert h, lib.fgx_global_error().decode()
    try:
        if contigs:
            bufs = [C.create_string_buffer(bytes(s), max(1, len(s))) for s in contigs]
            ptrs = (C.c_void_p * len(bufs))(*[C.cast(b, C.c_void_p).value for b in bufs])
            lens = (C.c_uint64 * len(bufs))(*[len(s) for s in contigs])
            assert lib.fgx_set_reference(h, len(bufs), ptrs, lens) == 0, lib.fgx_last_error(h).decode()
        out = Output()
        rc = lib.fgx_process_batch(h, g.blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, g.grp_first.ctypes.data, g.n_grp, C.byref(out))
        assert rc == 0, lib.fgx_last_error(h).decode()
        d2 = (C.c_uint64 * 2)()
        lib.fgx_debug_last_deferral(h, d2)
        return dict(data=C.string_at(out.data, out.data_len) if out.data_len else b"", count=int(out.count), stats=np.array(list(out.stats), dtype=np.uint64),
                    meth_device=int(lib.fgx_debug_last_meth_device(h)), deferred=int(d2[0]), canon=int(d2[1]))
    finally:
        lib.fgx_destroy(h)


def same_through_the_host_entry(o, contigs, g):
    want = oracle(o, contigs, g)
    got = host_entry(o, contigs, g)
    assert got["count"] == want["count"]
    assert_same_records(got["data"], want["data"])
    assert np.array_equal(got["stats"], want["stats"]), (got["stats"].tolist(), want["stats"].tolist())
    return got, want


@pytest.mark.parametrize("mode", [1, 2], ids=["em_seq", "taps"])
def test_mixed_batch_through_the_host_entry(mode):
    """The unfiltered 1 200 groups (deletions and soft clips in a third of them): device pass + the deferred subset on the general path.  No plain
    molecule may be deferred: at most the groups that hold a record with more than one CIGAR op are."""
    contigs, groups = batch(mode, plain=False)
    g = GroupedReads.from_groups(groups)
    n_complex = sum(any(n_ops(r) > 1 for r in grp) for grp in groups)
    assert 300 < n_complex < 400, n_complex
    got, _ = same_through_the_host_entry(options(mode, (1, 1, 0)), contigs, g)
    print("mixed batch:", got["meth_device"], "groups on the device pipeline,", got["deferred"], "deferred,", n_complex, "groups with a record of several CIGAR ops")
    assert got["meth_device"] == g.n_grp, got
    assert 0 < got["deferred"] <= n_complex, (got["deferred"], n_complex)
    assert got["canon"] == 0, got                       # the canonical-form second pass takes no molecule in this mode


def test_mixed_batch_with_a_per_strand_cap_that_bites():
    """duplex_max_reads_per_strand = 2: the annotation runs over all reads of a set, the consensus over the capped ones — the molecules the cap bites are
    deferred by design (name-rank downsampling on the host)."""
    contigs, groups = batch(1, plain=False)
    g = GroupedReads.from_groups(groups)
    got, _ = same_through_the_host_entry(options(1, (1, 1, 0), duplex_max_reads_per_strand=2), contigs, g)
    assert got["meth_device"] == g.n_grp, got


# ---- 3. the reference's own cases ----------------------------------------------------------------------------------------------------------------------
def test_the_references_duplex_cases_through_the_device_pipeline():
    import test_oracle_methylation_pins as pins
    cases = [(kw, contigs, groups) for kw, contigs, groups in pins.replay_cases() if kw.get("kind") == 1]
    assert len(cases) >= 2
    n_device = n_tagged = 0
    for kw, contigs, groups in cases:
        kw = dict(kw)
        mr = kw.pop("duplex_min_reads", None)
        o = fgx_opts.defaults(**kw)
        if mr:
            o.duplex_min_reads[0], o.duplex_min_reads[1], o.duplex_min_reads[2] = mr
        g = GroupedReads.from_groups(groups)
        got, want = same_through_the_host_entry(o, contigs, g)
        on_device = bool(o.methylation_mode) and bool(contigs) and not o.trim and not o.track_rejects
        assert got["meth_device"] == (g.n_grp if on_device else 0), (kw, got)
        n_device += on_device
        n_tagged += sum("bu" in bamutil.parse(r)["tags"] or "au" in bamutil.parse(r)["tags"] for r in split_records(want["data"]))
    assert n_device >= 1 and n_tagged >= 2, (n_device, n_tagged)


# ---- 4. opt-out ------------------------------------------------------------------------------------------------------------------------------------------
def test_opt_out_sends_the_batch_through_the_general_path(monkeypatch):
    contigs, groups = batch(1, plain=True, n_groups=400)
    g = GroupedReads.from_groups(groups)
    o = options(1, (1, 1, 0))
    on, _ = same_through_the_host_entry(o, contigs, g)
    assert on["meth_device"] == g.n_grp and on["deferred"] == 0, on
    monkeypatch.setenv("FGX_METH_DEVICE", "0")
    off, _ = same_through_the_host_entry(o, contigs, g)
    assert off["meth_device"] == 0 and off["data"] == on["data"], (off["meth_device"], off["deferred"])


def test_long_read_name_prefix_takes_the_per_field_writer():
    """k_emit_duplex<1> — the per-field writer's methylation build — with records it accepts: the smallest batch here under a 70-character prefix, every
    group decided on the device."""
    from test_wavemu_record_writers import writer_counts
    contigs, groups = batch(1, plain=True, n_groups=400)
    g = GroupedReads.from_groups(groups)
    got, want = same_through_the_host_entry(options(1, (1, 1, 0), read_name_prefix=b"m" * 70), contigs, g)
    assert got["meth_device"] == g.n_grp and got["deferred"] == 0, got
    assert writer_counts(want["data"]) == (0, want["count"]) and tag_counts(want["data"])["mm"] > 100


# ---- 5. file -> file -------------------------------------------------------------------------------------------------------------------------------------
def test_run_bam_keeps_the_batches_on_the_device(tmp_path):
    from fgumi_amd import bgzf
    contigs, groups = batch(1, plain=True)
    g = GroupedReads.from_groups(groups)
    want = oracle(options(1, (1, 1, 0)), contigs, g)
    assert b"MM" in want["data"] and b"bu" in want["data"]
    names = [f"chr{i + 1}" for i in range(len(contigs))]
    refs = [(n, len(s)) for n, s in zip(names, contigs)]
    src, dst = str(tmp_path / "grouped.bam"), str(tmp_path / "consensus.bam")
    bgzf.write_bam(src, bgzf.grouped_input_header(refs), refs, g.blob)
    c = caller(1, (1, 1, 0), contigs)
    try:
        for chunk in (0, 1 << 16):
            st = c.run_bam(src, dst, chunk_raw_bytes=chunk, threads=8, strip_strand_suffix=True)
            text, orefs, stream, off, ln = bgzf.read_bam(dst)
            got = b"".join(bytes(stream[int(o_) - 4:int(o_) + int(l)]) for o_, l in zip(off, ln))
            assert_same_records(got, want["data"])
            assert st["consensus_records"] == want["count"]
            assert st["stats"][:len(want["stats"])] == [int(v) for v in want["stats"]]
            assert st["host_entry_batches"] == 0 and st["deferred_groups"] == 0, (st["host_entry_batches"], st["deferred_groups"])
    finally:
        c.close()


# ---- 6. at size ------------------------------------------------------------------------------------------------------------------------------------------
def _threads():
    n = os.cpu_count() or 1
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, -(-int(q) // int(p))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 64))


@pytest.mark.timeout(1500)
def test_50000_molecules_against_the_oracle_shard_by_shard():
    """50 000 simulated duplex molecules of 6 + 6 pairs (BASELINE configs[2] shape) over a random genome under the simulator's coordinates (molecule m at
    1000 + 1000 m of contig 0): the reads are unrelated to that genome, so about one read base in sixteen is rewritten — the normalisation and the
    conversion-artifact rule are both live in every record."""
    n, shard, sim = 50000, 10000, dict(family_size=12, duplex=1)
    rng = np.random.default_rng(7)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=1000 + n * 1000 + 2000, dtype=np.uint8)].tobytes()
    o = options(1, (1, 1, 0))
    c = DuplexConsensusCaller("", "A", [1, 1, 0], cell_tag="CB", overlapping_consensus=True, methylation_mode=MethylationMode.EmSeq)
    c.set_reference({"chr1": genome}, ["chr1"])
    try:
        dg = c.simulate_on_device(n, **sim)
        out = c.process_batch_device(dg)
        assert out.n_deferred == 0 and out.count == 2 * n, (out.n_deferred, out.count)
        assert lib.fgx_debug_last_meth_device(c._h) == n
        st = np.array(c.last_stats_array, dtype=np.uint64)
        full = out.to_host()
        del dg, out
        off = 0
        stats = np.zeros(28, dtype=np.uint64)
        T = _threads()
        orc.set_reference([genome])
        try:
            for k in range(n // shard):
                gk = simulate_grouped_reads(shard, first_family=k * shard, **sim)
                want = orc.process(o, gk.blob, gk.rec_off, gk.rec_len, gk.grp_first, batch_groups=100, threads=T)
                part = want["data"]
                if k == 0:
                    t = tag_counts(part, first=1000)             # (not an empty comparison: two-strand records with MM)
                    assert t["both"] > 900 and t["mm"] > 900, t
                assert_same_records(full[off:off + len(part)], part)
                off += len(part)
                stats += want["stats"]
        finally:
            orc.set_reference(None)
        assert off == len(full), (off, len(full))
        assert np.array_equal(stats, st), (stats.tolist(), st.tolist())
    finally:
        c.close()


# ---- 7. guard bands --------------------------------------------------------------------------------------------------------------------------------------
def test_new_kernels_under_guard_bands():
    """The plain batch once more in a child interpreter with every device buffer between sentinel bands (FGX_GUARD_BAND), then a look at every band."""
    run_isolated("test_gpu_duplex_methylation_device", "check_plain_device_entry", 1, (1, 1, 0), {}, True, env={"FGX_GUARD_BAND": "4096"}, timeout=900)
