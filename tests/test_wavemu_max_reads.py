"""--max-reads decided by the streaming kernels of deep simplex families (k_deep_parse's cut in its builds <64, 64>, <128, 128>, <256, 512> and <256, 1024>,
k_deep_cols over the survivors' rows), executed on the CPU in 64-lane lock-step (tests/wavemu — a cross-lane operation or a barrier under divergent control
flow faults there): one batch through fgx_process_batch_device of the emulation library against the oracle — nothing deferred, every family above 64 records
finished by the streaming kernels, bytes, count and all 28 counters equal.

The simplex cap (downsample_filtered_source_reads, vanilla_caller.rs:902-932) keeps, per end, the `max_reads` lowest fgbio name ranks, ties in file order; the
survivors stay in FILE order and what is dropped counts as Downsampled."""
import ctypes as C

import numpy as np
import pytest

import fgx_opts
import orc
from isolated import run_isolated
from max_reads_cases import REJ_DOWNSAMPLED, families_the_cap_bites, families_with_a_tie_cut_in_the_middle, methylation_batch, with_tied_names
from test_wavemu import env


def device_entry(g, contigs=None, want_bites=True, **opts):
    """fgx_process_batch_device on host arrays against the oracle.  Returns (families the streaming kernels finished, the oracle's result)."""
    from fgumi_amd._lib import Options, Output, lib
    o = fgx_opts.defaults(**opts)
    if contigs is not None:
        orc.set_reference(contigs)
    try:
        want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=50)
    finally:
        orc.set_reference(None)
    assert (int(want["stats"][3 + REJ_DOWNSAMPLED]) > 0) == want_bites          # the comparison is not empty: the oracle dropped reads
    for f in ("fgx_debug_last_deep_families", "fgx_debug_last_big_families", "fgx_debug_last_meth_device"):
        getattr(lib, f).restype = C.c_uint32
        getattr(lib, f).argtypes = [C.c_void_p]
    po = Options.from_buffer_copy(bytes(o))
    h = lib.fgx_create(C.byref(po))
    assert h, lib.fgx_global_error().decode()
    try:
        if contigs is not None:
            bufs = [C.create_string_buffer(bytes(s), max(1, len(s))) for s in contigs]
            ptrs = (C.c_void_p * len(bufs))(*[C.cast(b, C.c_void_p).value for b in bufs])
            lens = (C.c_uint64 * len(bufs))(*[len(s) for s in contigs])
            assert lib.fgx_set_reference(h, len(bufs), ptrs, lens) == 0, lib.fgx_last_error(h).decode()
        blob = np.concatenate([g.blob, np.zeros(64, dtype=np.uint8)])
        out, nd, dp = Output(), C.c_uint32(), C.c_void_p()
        rc = lib.fgx_process_batch_device(h, blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, g.grp_first.ctypes.data, g.n_grp,
                                          C.byref(out), C.byref(nd), C.byref(dp))
        assert rc == 0, lib.fgx_last_error(h).decode()
        path = dict(big=int(lib.fgx_debug_last_big_families(h)), deep=int(lib.fgx_debug_last_deep_families(h)), meth=int(lib.fgx_debug_last_meth_device(h)))
        assert nd.value == 0, f"{nd.value} of {g.n_grp} families deferred ({path})"
        got = C.string_at(out.data, out.data_len) if out.data_len else b""
        if got != want["data"]:
            import bamutil
            from fgumi_amd import split_records
            for i, (a, b) in enumerate(zip(split_records(got), split_records(want["data"]))):
                assert a == b, f"record {i} differs:\n got {bamutil.parse(a)}\nwant {bamutil.parse(b)}"
        assert int(out.count) == want["count"] and got == want["data"]
        stats = np.array(np.ctypeslib.as_array(out.stats, shape=(len(want["stats"]),)), dtype=np.uint64)
        assert np.array_equal(stats, want["stats"]), (stats.tolist(), want["stats"].tolist())
    finally:
        lib.fgx_destroy(h)
    return path, want


def check_simulated(n_families, sim, cap, min_reads=1, bites_at_least=0.25):
    from fgumi_amd import simulate_grouped_reads
    g = simulate_grouped_reads(n_families, **sim)
    n = np.diff(np.asarray(g.grp_first, dtype=np.int64))
    assert n.min() > 64 and families_the_cap_bites(g, cap) >= bites_at_least * n_families
    path, _ = device_entry(g, min_reads=min_reads, max_reads=cap)
    assert path["big"] == path["deep"] == n_families, path          # every family finished by the streaming kernels: none went on to k_family


def check_ties():
    from fgumi_amd import simulate_grouped_reads
    g = with_tied_names(simulate_grouped_reads(30, family_size=40, family_size_max=60))
    assert families_with_a_tie_cut_in_the_middle(g, 2) >= 1
    path, _ = device_entry(g, min_reads=1, max_reads=2)
    assert path["big"] == path["deep"] == 30, path


def check_methylation(mode):
    contigs, g = methylation_batch(43, 150)
    assert g.n_grp > 75 and families_the_cap_bites(g, 3) >= 25
    path, _ = device_entry(g, contigs, min_reads=1, max_reads=3, methylation_mode=mode)
    assert path["meth"] == g.n_grp, path


def check_cap_that_does_not_bite():
    """A cap above every end and no cap at all: the same bytes (the oracle's), the same path."""
    from fgumi_amd import simulate_grouped_reads
    g = simulate_grouped_reads(20, family_size=35, family_size_max=70)
    p0, w0 = device_entry(g, want_bites=False, min_reads=1)
    p1, w1 = device_entry(g, want_bites=False, min_reads=1, max_reads=10000)
    assert p0 == p1 and p0["deep"] == 20 and w0["data"] == w1["data"]


@pytest.mark.parametrize("cap", [4, 20])
def test_two_and_four_wavefront_builds(cap):
    """70 - 140 records per family: the <128, 128> build and the <256, 512> build."""
    run_isolated("test_wavemu_max_reads", "check_simulated", 40, dict(family_size=35, family_size_max=70), cap, env=env(), timeout=1500)


def test_min_reads_above_one_takes_the_consensus_length_from_the_survivors():
    from max_reads_cases import READ_THROUGH
    run_isolated("test_wavemu_max_reads", "check_simulated", 25, dict(family_size=35, family_size_max=60, **READ_THROUGH), 5, 3, env=env(), timeout=1500)


def test_families_of_more_than_512_records():
    """520 - 700 records: the <256, 1024> build, launched over what the <256, 512> build handed on."""
    run_isolated("test_wavemu_max_reads", "check_simulated", 3, dict(family_size=260, family_size_max=350), 30, env=env(), timeout=1500)


def test_equal_ranks_at_the_cut():
    run_isolated("test_wavemu_max_reads", "check_ties", env=env(), timeout=1500)


@pytest.mark.parametrize("mode", [1, 2], ids=["em_seq", "taps"])
def test_methylation_mode_through_the_wavefront_sized_build(mode):
    run_isolated("test_wavemu_max_reads", "check_methylation", mode, env=env(), timeout=1500)


def test_cap_that_does_not_bite():
    run_isolated("test_wavemu_max_reads", "check_cap_that_does_not_bite", env=env(), timeout=1500)
