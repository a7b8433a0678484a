"""`fgumi simplex` on the output of `fgumi group --allow-unmapped`, decided by the device kernels — executed on the CPU in 64-lane lock-step (tests/wavemu: the
real launch chain and kernel sources of fastpath.hip under a shim; a cross-lane operation or a barrier under divergent control flow faults there).

For the simplex caller an unmapped record is a read without a CIGAR: no clip against the mate, no part in the overlap step (whatever ref_id / pos say), and an
end that holds mapped and unmapped source reads loses the unmapped ones (drop_unmapped_if_any_mapped, vanilla_caller.rs:1206-1232).  Every batch goes through
fgx_process_batch_device and is compared with the oracle byte for byte — count, all 28 counters (the four overlap counters among them) — with NOTHING deferred;
each case first asserts on the oracle's own result that it decides what it is named for."""
import ctypes as C

import numpy as np
import pytest

import fgx_opts
import orc
import unmapped_cases as uc
from isolated import run_isolated
from test_wavemu import env


def device_entry(g, contigs=None, allow_deferral=False, **opts):
    """fgx_process_batch_device of the emulation library on host arrays against the oracle.  Returns (path counters, the oracle's result)."""
    from fgumi_amd._lib import Options, Output, lib
    o = fgx_opts.defaults(**opts)
    if contigs is not None:
        orc.set_reference(contigs)
    try:
        want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=50)
    finally:
        orc.set_reference(None)
    for f in ("fgx_debug_last_deep_families", "fgx_debug_last_big_families"):
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
        rec_off, rec_len, grp_first = (np.ascontiguousarray(a) for a in (g.rec_off, g.rec_len, g.grp_first))
        out, nd, dp = Output(), C.c_uint32(), C.c_void_p()
        rc = lib.fgx_process_batch_device(h, blob.ctypes.data, g.blob.size, rec_off.ctypes.data, rec_len.ctypes.data, g.n_rec, grp_first.ctypes.data, g.n_grp,
                                          C.byref(out), C.byref(nd), C.byref(dp))
        assert rc == 0, lib.fgx_last_error(h).decode()
        path = dict(big=int(lib.fgx_debug_last_big_families(h)), deep=int(lib.fgx_debug_last_deep_families(h)), deferred=int(nd.value))
        if allow_deferral:
            if nd.value:                                    # the deferred families through the host entry of the same library: the whole batch, as a caller would
                out = Output()
                rc = lib.fgx_process_batch(h, blob.ctypes.data, g.blob.size, rec_off.ctypes.data, rec_len.ctypes.data, g.n_rec, grp_first.ctypes.data, g.n_grp, C.byref(out))
                assert rc == 0, lib.fgx_last_error(h).decode()
        else:
            assert nd.value == 0, f"{nd.value} of {g.n_grp} families deferred ({path})"
        got = C.string_at(out.data, out.data_len) if out.data_len else b""
        if got != want["data"]:
            import bamutil
            from fgumi_amd import split_records
            a, b = split_records(got), split_records(want["data"])
            for i, (x, y) in enumerate(zip(a, b)):
                assert x == y, f"record {i} differs:\n got {bamutil.parse(x)}\nwant {bamutil.parse(y)}"
            assert len(a) == len(b), (len(a), len(b))
        assert int(out.count) == want["count"] and got == want["data"]
        stats = np.array(np.ctypeslib.as_array(out.stats, shape=(len(want["stats"]),)), dtype=np.uint64)
        assert np.array_equal(stats, want["stats"]), (stats.tolist(), want["stats"].tolist())
    finally:
        lib.fgx_destroy(h)
    return path, want


def oracle_overlap(g, **opts):
    return [int(v) for v in orc.process(fgx_opts.defaults(**opts), g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=50)["stats"][uc.OVERLAP]]


def check_wholly_unmapped(n_families, sim, placed, opts=None, want_deep=False, fragments=False, keep_reverse=True, downsampled=False):
    """Every record unmapped.  Pairs: the mapped twin shows overlapping bases, the unmapped batch none — whatever the positions say."""
    from fgumi_amd import simulate_grouped_reads
    opts = dict(min_reads=1, **(opts or {}))
    g = simulate_grouped_reads(n_families, **sim)
    if fragments:
        g = uc.as_fragments(g)
        assert (uc.flags_of(g) & 0x10).any() and not (uc.flags_of(g) & 0x10).all()          # REVERSE is honoured where it is set: both strands occur
    else:
        assert min(oracle_overlap(g, **opts)[:2]) > 0
    u = uc.unmap(g, uc.everything(g), placed=placed, keep_reverse=keep_reverse)
    assert (uc.flags_of(u) & 0x4).all() and int(u.blob.size) == int(g.blob.size) - 4 * g.n_rec
    path, want = device_entry(u, **opts)
    assert want["count"] > 0 and int(want["stats"][3 + uc.REJ_UNMAPPED]) == 0 and not any(int(v) for v in want["stats"][uc.OVERLAP])
    assert (int(want["stats"][3 + uc.REJ_DOWNSAMPLED]) > 0) == downsampled
    if want_deep:
        assert path["big"] == path["deep"] == n_families, path          # every family finished by the streaming kernels


def check_r1_mapped_r2_unmapped(n_families, sim, placed):
    from fgumi_amd import simulate_grouped_reads
    g = simulate_grouped_reads(n_families, **sim)
    assert min(oracle_overlap(g, min_reads=1)[:2]) > 0
    u = uc.unmap(g, uc.all_r2(g), placed=placed)
    _, want = device_entry(u, min_reads=1)
    assert want["count"] == 2 * n_families and int(want["stats"][3 + uc.REJ_UNMAPPED]) == 0 and not any(int(v) for v in want["stats"][uc.OVERLAP])


def check_mixed(case):
    if case == "every_third_pair":
        g, u = uc.mixed_every_third_pair(20, 5)
        _, want = device_entry(u, min_reads=1)
        assert int(want["stats"][3 + uc.REJ_UNMAPPED]) == 80 and want["count"] == 40
        ov, ov_twin = [int(v) for v in want["stats"][uc.OVERLAP]], oracle_overlap(g, min_reads=1)
        assert 0 < ov[0] < ov_twin[0]                                # the mapped pairs are still corrected, the unmapped ones are not
    elif case == "one_mapped_two_unmapped_min_reads_2":
        g, u = uc.mixed_one_mapped_two_unmapped(20)
        _, want = device_entry(u, min_reads=2)
        st = want["stats"]
        assert int(st[3 + uc.REJ_UNMAPPED]) == 40 and int(st[3 + uc.REJ_INSUFFICIENT]) == 20 and int(st[3 + uc.REJ_ORPHAN]) == 60 and want["count"] == 0
    elif case == "only_mapped_read_trims_away":
        g, u = uc.mixed_only_mapped_read_trims_away(20)
        _, want = device_entry(u, min_reads=1)
        st = want["stats"]
        assert int(st[3 + uc.REJ_UNMAPPED]) == 0 and int(st[3 + uc.REJ_ZERO_LENGTH]) == 20 and want["count"] == 40
    elif case == "max_reads_2":
        g, u = uc.mixed_every_third_pair(20, 6)
        _, want = device_entry(u, min_reads=1, max_reads=2)
        st = want["stats"]
        assert int(st[3 + uc.REJ_UNMAPPED]) == 80 and int(st[3 + uc.REJ_DOWNSAMPLED]) == 80 and want["count"] == 40
    else:
        raise ValueError(case)


def check_methylation(mode):
    """The methylation-aware mode needs a reference position per read: families with unmapped records may stay deferred there, and stay correct."""
    from max_reads_cases import methylation_batch
    contigs, g = methylation_batch(47, 60)
    which = uc.family_of(g) % 2 == 0
    u = uc.unmap(g, which, mate=uc.mates(g))
    assert which.any() and not which.all()
    device_entry(u, contigs, allow_deferral=True, min_reads=1, methylation_mode=mode)


@pytest.mark.parametrize("placed", [False, True], ids=["pos_minus_one", "placed_at_the_mate"])
def test_wholly_unmapped_depth8_pairs_stay_in_the_split_pipeline(placed):
    """k_split_parse's shared span comes from pos / ref_id equality: -1 / -1, or each mate at the other's position, would show a full overlap."""
    run_isolated("test_wavemu_unmapped", "check_wholly_unmapped", 500, dict(family_size=8), placed, env=env(), timeout=1500)


def test_wholly_unmapped_depth3_families():
    run_isolated("test_wavemu_unmapped", "check_wholly_unmapped", 300, dict(family_size=3), True, env=env(), timeout=900)


def test_wholly_unmapped_depth1_and_depth2_families_through_the_seg_head():
    run_isolated("test_wavemu_unmapped", "check_wholly_unmapped", 200, dict(family_size=1, family_size_max=2), False, env=env(), timeout=900)


def test_unmapped_fragments_keep_their_strand():
    run_isolated("test_wavemu_unmapped", "check_wholly_unmapped", 200, dict(family_size=4), False, None, False, True, env=env(), timeout=900)


def test_unmapped_reads_with_reverse_cleared():
    run_isolated("test_wavemu_unmapped", "check_wholly_unmapped", 150, dict(family_size=5), False, None, False, False, False, env=env(), timeout=900)


@pytest.mark.parametrize("placed", [False, True], ids=["pos_minus_one", "placed_at_the_mate"])
def test_r1_mapped_r2_unmapped_is_uniform_by_flag(placed):
    run_isolated("test_wavemu_unmapped", "check_r1_mapped_r2_unmapped", 300, dict(family_size=6), placed, env=env(), timeout=900)


def test_wholly_unmapped_deep_families_through_the_streaming_kernels():
    """40 families of 80 .. 200 records: k_deep_parse / k_deep_cols finish every one."""
    run_isolated("test_wavemu_unmapped", "check_wholly_unmapped", 40, dict(family_size=40, family_size_max=100), True, None, True, env=env(), timeout=1500)


@pytest.mark.parametrize("case", ["every_third_pair", "one_mapped_two_unmapped_min_reads_2", "only_mapped_read_trims_away", "max_reads_2"])
def test_mixed_ends_are_decided_by_the_wavefront_kernel(case):
    run_isolated("test_wavemu_unmapped", "check_mixed", case, env=env(), timeout=900)


def test_wholly_unmapped_families_under_a_biting_max_reads():
    e = env()
    run_isolated("test_wavemu_unmapped", "check_wholly_unmapped", 150, dict(family_size=8), False, dict(max_reads=3), False, False, True, True, env=e, timeout=900)
    run_isolated("test_wavemu_unmapped", "check_wholly_unmapped", 25, dict(family_size=40, family_size_max=70), True, dict(max_reads=10), True, False, True, True, env=e, timeout=1500)


@pytest.mark.parametrize("mode", [1, 2], ids=["em_seq", "taps"])
def test_methylation_mode_with_unmapped_families_stays_correct(mode):
    run_isolated("test_wavemu_unmapped", "check_methylation", mode, env=env(), timeout=1500)
