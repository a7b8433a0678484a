"""The duplex caller's methylation-aware mode (EM-Seq / TAPs) in the device-resident pipeline, in the wave-level emulator (tests/wavemu: the
real launch chain and kernel sources, 64 lanes in lock-step on the CPU): k_family_wave<1, 1> (anchor, reference lookup, unconverted /
converted counts and the normalisation in the column loops), the record writers' conversion-artifact rule (k_emit_duplex_fast<1>) and the
tag kernels behind RX (k_duplex_meth_sizes / k_duplex_meth_tail: am/au/at, bm/bu/bt, MM/ML/cu/ct), against the oracle.

The molecules are the single-`M` ones of tests/methsim.py's duplex batch — A-only, B-only and two-strand molecules, conversions on the A
strand's C's and the B strand's G's, overlapping mates, soft-masked and N stretches in the genome.  With the mode off the duplex kernels decide
every one of them without a deferral, so a deferral here is the new code's."""
import ctypes as C

import numpy as np
import pytest

import bamutil
import fgx_opts
import methsim
import orc
from isolated import run_isolated
from test_wavemu import env


def plain_groups(groups):
    """The groups whose records all have one CIGAR op."""
    return [g for g in groups if all(bamutil.parse(r)["n_cigar"] == 1 for r in g)]


def check_device_entry(mode, min_reads, seed=71, n_groups=400, **kw):
    from fgumi_amd import GroupedReads
    from fgumi_amd._lib import Options, Output, lib
    rng = methsim.seeded(seed)
    contigs = methsim.genome(rng)
    groups = plain_groups(methsim.duplex_groups(rng, contigs, n_groups))
    assert len(groups) > n_groups // 2
    g = GroupedReads.from_groups(groups)
    o = fgx_opts.defaults(kind=1, methylation_mode=mode, **kw)
    o.duplex_min_reads[0], o.duplex_min_reads[1], o.duplex_min_reads[2] = min_reads
    orc.set_reference(contigs)
    try:
        want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=100)
    finally:
        orc.set_reference(None)
    recs = [bamutil.parse(r) for r in bamutil_split(want["data"])]
    assert sum("au" in r["tags"] and "bu" in r["tags"] for r in recs) > 100 and sum("MM" in r["tags"] for r in recs) > 100      # (not an empty comparison)
    lib.fgx_debug_last_meth_device.restype = C.c_uint32
    lib.fgx_debug_last_meth_device.argtypes = [C.c_void_p]
    po = Options.from_buffer_copy(bytes(o))
    h = lib.fgx_create(C.byref(po))
    assert h, lib.fgx_global_error().decode()
    try:
        bufs = [C.create_string_buffer(bytes(s), max(1, len(s))) for s in contigs]
        ptrs = (C.c_void_p * len(bufs))(*[C.cast(b, C.c_void_p).value for b in bufs])
        lens = (C.c_uint64 * len(bufs))(*[len(s) for s in contigs])
        assert lib.fgx_set_reference(h, len(bufs), ptrs, lens) == 0, lib.fgx_last_error(h).decode()
        blob = np.concatenate([g.blob, np.zeros(64, dtype=np.uint8)])
        out, nd, dp = Output(), C.c_uint32(), C.c_void_p()
        rc = lib.fgx_process_batch_device(h, blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, g.grp_first.ctypes.data, g.n_grp,
                                          C.byref(out), C.byref(nd), C.byref(dp))
        assert rc == 0, lib.fgx_last_error(h).decode()
        assert nd.value == 0, nd.value
        got = C.string_at(out.data, out.data_len) if out.data_len else b""
        assert int(out.count) == want["count"]
        if got != want["data"]:
            for i, (a, b) in enumerate(zip(bamutil_split(got), bamutil_split(want["data"]))):
                if a != b:
                    raise AssertionError(f"record {i} differs:\n got {bamutil.parse(a)}\nwant {bamutil.parse(b)}")
            raise AssertionError("record count / length differs")
        assert np.array_equal(np.array(list(out.stats), dtype=np.uint64), want["stats"]), (list(out.stats), want["stats"].tolist())
        assert int(lib.fgx_debug_last_meth_device(h)) == g.n_grp
    finally:
        lib.fgx_destroy(h)


def bamutil_split(data):
    from fgumi_amd import split_records
    return split_records(data)


@pytest.mark.parametrize("mode", [1, 2], ids=["em_seq", "taps"])
@pytest.mark.parametrize("min_reads", [(1, 1, 0), (3, 2, 1)], ids=["min_1_1_0", "min_3_2_1"])
def test_single_m_duplex_molecules_in_the_emulated_kernels(mode, min_reads):
    run_isolated("test_wavemu_duplex_methylation", "check_device_entry", mode, min_reads, env=env(), timeout=1500)


def test_without_per_base_tags_and_overlap_correction():
    run_isolated("test_wavemu_duplex_methylation", "check_device_entry", 1, (1, 1, 0), 72, 300, env=env(), timeout=1500)
    run_isolated("test_wavemu_duplex_methylation", "check_device_entry_kw", 1, (1, 1, 0), dict(produce_per_base_tags=0, overlapping_consensus=0), env=env(), timeout=1500)


def check_device_entry_kw(mode, min_reads, kw):
    check_device_entry(mode, min_reads, **kw)
