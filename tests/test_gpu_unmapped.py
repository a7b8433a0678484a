"""GPU parity: `fgumi simplex` on the output of `fgumi group --allow-unmapped`, decided by the device kernels.

For the simplex caller an unmapped record is a read without a CIGAR (create_source_read, vanilla_caller.rs:1080-1190): no clip against its mate, no part in the
overlap step whatever ref_id / pos say (overlapping.rs:236-240), and an end that holds mapped and unmapped source reads loses the unmapped ones
(drop_unmapped_if_any_mapped, :1206-1232, counted as Unmapped).  Ends that are uniform by flag stay in the kernels a mapped family of their shape runs in (split
pipeline, seg head, wave2 chain, streaming kernels); an end with both goes to k_family_wave<0>.  Every batch is compared with the oracle byte for byte — count and
all 28 counters, the four overlap counters among them — with nothing deferred, and each case first asserts on the oracle's own result that it decides what it is
named for.  The mapped twin of every batch still gives the oracle's bytes."""
import ctypes as C

import numpy as np
import pytest

import fgx_opts
import orc
import unmapped_cases as uc
from isolated import run_isolated

pytestmark = pytest.mark.gpu

_BATCHES = {}


def _sim(key, n_families, **sim):
    """(mapped batch, the oracle's result for it at --min-reads 1): computed once, never modified."""
    if key not in _BATCHES:
        from fgumi_amd import simulate_grouped_reads
        g = simulate_grouped_reads(n_families, **sim)
        _BATCHES[key] = (g, orc.process(fgx_opts.defaults(min_reads=1), g.blob, g.rec_off, g.rec_len, g.grp_first))
    return _BATCHES[key]


def _caller(min_reads=1, max_reads=None):
    from fgumi_amd import VanillaUmiConsensusCaller, VanillaUmiConsensusOptions
    return VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(min_reads=min_reads, max_reads=max_reads, min_consensus_base_quality=2, cell_tag="CB"),
                                     overlapping_consensus=True)


def _debug(c):
    from fgumi_amd import lib
    for f in ("fgx_debug_last_big_families", "fgx_debug_last_deep_families"):
        getattr(lib, f).restype = C.c_uint32
        getattr(lib, f).argtypes = [C.c_void_p]
    lib.fgx_debug_last_split_builds.restype = None
    lib.fgx_debug_last_split_builds.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.fgx_debug_last_chain.restype = None
    lib.fgx_debug_last_chain.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    b, ch = (C.c_uint64 * 4)(), (C.c_uint32 * 2)()
    lib.fgx_debug_last_split_builds(c._h, b)
    lib.fgx_debug_last_chain(c._h, ch)
    return dict(big=int(lib.fgx_debug_last_big_families(c._h)), deep=int(lib.fgx_debug_last_deep_families(c._h)), packed=int(b[0]), classic=int(b[1]), build=int(b[2]),
                launches=int(ch[0]), syncs=int(ch[1]))


def _run(g, want=None, min_reads=1, max_reads=None):
    """The batch through the device-resident entry against the oracle: nothing deferred, bytes, count, counters.  Returns (path, the oracle's result)."""
    if want is None:
        want = orc.process(fgx_opts.defaults(min_reads=min_reads, max_reads=-1 if max_reads is None else max_reads), g.blob, g.rec_off, g.rec_len, g.grp_first)
    c = _caller(min_reads, max_reads)
    try:
        out = c.process_batch_device(g.to_device())
        got = out.to_host()
        path = _debug(c)
        stats = np.array(c.last_stats_array, dtype=np.uint64)
        assert out.n_deferred == 0, f"{out.n_deferred} of {g.n_grp} families deferred ({path})"
        assert out.count == want["count"] and got == want["data"], f"output differs from the oracle ({len(got)} vs {len(want['data'])} bytes; path {path})"
        assert np.array_equal(stats, want["stats"]), (stats.tolist(), want["stats"].tolist())
    finally:
        c.close()
    return path, want


def _wholly(key, n_families, placed, sim, **opts):
    g, want_twin = _sim(key, n_families, **sim)
    assert min(int(v) for v in want_twin["stats"][uc.OVERLAP][:2]) > 0
    if not opts:
        _run(g, want_twin)                                                               # existing behaviour: the mapped twin
    u = uc.unmap(g, uc.everything(g), placed=placed)
    path, want = _run(u, **opts)
    assert want["count"] > 0 and int(want["stats"][3 + uc.REJ_UNMAPPED]) == 0 and not any(int(v) for v in want["stats"][uc.OVERLAP])
    return path, want


@pytest.mark.parametrize("placed", [False, True], ids=["pos_minus_one", "placed_at_the_mate"])
def test_wholly_unmapped_depth8_families(placed):
    """k_split_parse derives a pair's shared span from pos / ref_id equality: -1 / -1, or each mate at the other's position, would show a full overlap."""
    _wholly("d8", 2000, placed, dict(family_size=8))


def test_wholly_unmapped_depth3_families():
    _wholly("d3", 2000, True, dict(family_size=3))


def test_wholly_unmapped_depth1_and_depth2_families():
    _wholly("d12", 2000, False, dict(family_size=1, family_size_max=2))


def test_wholly_unmapped_deep_families_stay_with_the_streaming_kernels():
    path, _ = _wholly("deep", 100, True, dict(family_size=40, family_size_max=100))
    assert path["big"] == path["deep"] == 100, path


@pytest.mark.parametrize("cap,key,n,sim", [(3, "d8", 2000, dict(family_size=8)), (10, "deep", 100, dict(family_size=40, family_size_max=100))], ids=["shallow", "deep"])
def test_wholly_unmapped_families_under_a_biting_max_reads(cap, key, n, sim):
    path, want = _wholly(key, n, False, sim, max_reads=cap)
    assert int(want["stats"][3 + uc.REJ_DOWNSAMPLED]) > 0
    if key == "deep":
        assert path["big"] == path["deep"] == n, path


@pytest.mark.parametrize("placed", [False, True], ids=["pos_minus_one", "placed_at_the_mate"])
def test_r1_mapped_r2_unmapped_is_uniform_by_flag(placed):
    g, _ = _sim("d8", 2000, family_size=8)
    _, want = _run(uc.unmap(g, uc.all_r2(g), placed=placed))
    assert want["count"] == 2 * g.n_grp and int(want["stats"][3 + uc.REJ_UNMAPPED]) == 0 and not any(int(v) for v in want["stats"][uc.OVERLAP])


def test_unmapped_fragments_keep_their_strand():
    g, _ = _sim("d3", 2000, family_size=3)
    f = uc.as_fragments(g)
    rev = (uc.flags_of(f) & 0x10) != 0
    assert rev.any() and not rev.all()
    _run(f)
    _, want = _run(uc.unmap(f, uc.everything(f), mate=np.full(f.n_rec, -1, dtype=np.int64)))
    assert want["count"] == f.n_grp


@pytest.mark.parametrize("case", ["every_third_pair", "one_mapped_two_unmapped_min_reads_2", "only_mapped_read_trims_away", "max_reads_2"])
def test_mixed_ends_are_decided_by_the_wavefront_kernel(case):
    n = 500
    if case == "every_third_pair":
        g, u = uc.mixed_every_third_pair(n, 5)
        w_twin = _run(g)[1]
        _, want = _run(u)
        assert int(want["stats"][3 + uc.REJ_UNMAPPED]) == 4 * n and want["count"] == 2 * n
        assert 0 < int(want["stats"][24]) < int(w_twin["stats"][24])             # the mapped pairs are still corrected, the unmapped ones are not
    elif case == "one_mapped_two_unmapped_min_reads_2":
        g, u = uc.mixed_one_mapped_two_unmapped(n)
        _run(g, min_reads=2)
        st = _run(u, min_reads=2)[1]["stats"]
        assert int(st[3 + uc.REJ_UNMAPPED]) == 2 * n and int(st[3 + uc.REJ_INSUFFICIENT]) == n and int(st[3 + uc.REJ_ORPHAN]) == 3 * n
    elif case == "only_mapped_read_trims_away":
        g, u = uc.mixed_only_mapped_read_trims_away(n)
        _run(g)
        _, want = _run(u)
        st = want["stats"]
        assert int(st[3 + uc.REJ_UNMAPPED]) == 0 and int(st[3 + uc.REJ_ZERO_LENGTH]) == n and want["count"] == 2 * n
    else:
        g, u = uc.mixed_every_third_pair(n, 6)
        _run(g, max_reads=2)
        st = _run(u, max_reads=2)[1]["stats"]
        assert int(st[3 + uc.REJ_UNMAPPED]) == 4 * n and int(st[3 + uc.REJ_DOWNSAMPLED]) == 4 * n


# ---- the path taken (child interpreters: the library's switches are read once per process) ------------------------------------------------------------

def check_split_pipeline_keeps_unmapped_families(n_families):
    """A wholly unmapped depth-8 batch is finished by the split pipeline — the packed build, as for its mapped twin — with the twin's launches and host syncs."""
    import torch  # noqa: F401
    from fgumi_amd import simulate_grouped_reads
    g = simulate_grouped_reads(n_families, family_size=8)
    p_twin, _ = _run(g)
    u = uc.unmap(g, uc.everything(g), placed=True)
    p, want = _run(u)
    print("mapped", p_twin, "\nunmapped", p, flush=True)
    assert not any(int(v) for v in want["stats"][uc.OVERLAP])
    assert p["packed"] + p["classic"] == n_families and p["big"] == 0, p
    assert p_twin["build"] == 1 and p["build"] == 1 and p["packed"] >= 0.9 * n_families, (p_twin, p)
    assert (p["launches"], p["syncs"]) == (p_twin["launches"], p_twin["syncs"]), (p_twin, p)


def test_wholly_unmapped_depth8_batch_is_finished_by_the_split_pipeline():
    run_isolated("test_gpu_unmapped", "check_split_pipeline_keeps_unmapped_families", 20000)


def check_rejects_device_entry():
    """--rejects on a batch with mixed ends through the device entry: the oracle's reject set, nothing deferred."""
    import torch
    from fgumi_amd import GroupedReads
    from fgumi_amd._lib import Options, Output, hip_memcpy_d2h, lib
    parts = [uc.mixed_every_third_pair(200, 5)[1], uc.mixed_one_mapped_two_unmapped(200)[1], uc.mixed_only_mapped_read_trims_away(200)[1]]
    g = GroupedReads.from_groups([p.records(i) for p in parts for i in range(p.n_grp)])
    o = fgx_opts.defaults(kind=0, track_rejects=1, min_reads=2)
    want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=50)
    assert want["n_rejects"] > 0 and int(want["stats"][3 + uc.REJ_UNMAPPED]) > 0
    po = Options.from_buffer_copy(bytes(o))
    po.device = 0
    h = lib.fgx_create(C.byref(po))
    assert h, lib.fgx_global_error().decode()
    try:
        dg = g.to_device(0)
        torch.cuda.synchronize()
        out, nd, dp = Output(), C.c_uint32(), C.c_void_p()
        rc = lib.fgx_process_batch_device(h, dg.blob.data_ptr(), dg.blob_len, dg.rec_off.data_ptr(), dg.rec_len.data_ptr(), dg.n_rec, dg.grp_first.data_ptr(), dg.n_grp,
                                          C.byref(out), C.byref(nd), C.byref(dp))
        assert rc == 0, lib.fgx_last_error(h).decode()
        assert nd.value == 0, f"{nd.value} groups deferred by the device entry"
        assert int(out.n_rejects) == want["n_rejects"]
        assert hip_memcpy_d2h(out.rejects, int(out.rejects_len)) == want["rejects"]
        assert hip_memcpy_d2h(out.data, int(out.data_len)) == want["data"] and int(out.count) == want["count"]
        assert np.array_equal(np.array(list(out.stats), dtype=np.uint64), want["stats"])
    finally:
        lib.fgx_destroy(h)


def test_rejects_of_a_batch_with_mixed_ends_come_from_the_device_entry():
    run_isolated("test_gpu_unmapped", "check_rejects_device_entry")


def check_run_bam(tmp_dir):
    """fgx_run_bam on a BGZF file of wholly unmapped families: with allow_unmapped the oracle's records and counters, no group deferred, no batch through the host
    entry; without it the grouping stage drops every record."""
    import os
    from fgumi_amd import bgzf, simulate_grouped_reads
    g = simulate_grouped_reads(5000, family_size=4)
    u = uc.unmap(g, uc.everything(g))
    want = orc.process(fgx_opts.defaults(min_reads=1), u.blob, u.rec_off, u.rec_len, u.grp_first, batch_groups=100000)
    assert want["count"] == 2 * u.n_grp
    c = _caller()
    refs = [("chr%d" % (i + 1), 2147483647) for i in range(24)]
    src, dst = os.path.join(tmp_dir, "grouped.bam"), os.path.join(tmp_dir, "consensus.bam")
    bgzf.write_bam(src, bgzf.grouped_input_header(refs), refs, u.blob)
    st = c.run_bam(src, dst, threads=8, allow_unmapped=True)
    _, _, stream, off, ln = bgzf.read_bam(dst)
    got = b"".join(bytes(stream[int(a) - 4:int(a) + int(b)]) for a, b in zip(off, ln))
    print(f"chunks {st['chunks']}, deferred groups {st['deferred_groups']}, host entry batches {st['host_entry_batches']}", flush=True)
    assert got == want["data"], "the consensus BAM's records differ from the oracle's"
    assert st["stats"][:28] == [int(v) for v in want["stats"]]
    assert st["deferred_groups"] == 0 and st["host_entry_batches"] == 0, (st["deferred_groups"], st["host_entry_batches"])
    c.run_bam(src, dst, threads=8, allow_unmapped=False)
    _, _, _, off, _ = bgzf.read_bam(dst)
    assert len(off) == 0
    c.close()


def test_run_bam_with_allow_unmapped(tmp_path):
    run_isolated("test_gpu_unmapped", "check_run_bam", str(tmp_path), timeout=600)


def check_under_guard_bands():
    """(child interpreter, FGX_GUARD_BAND set) One wholly unmapped and one mixed batch, each followed by a look at every guarded buffer."""
    from fgumi_amd import lib, simulate_grouped_reads
    lib.fgx_debug_check_guard_bands.restype = C.c_int
    lib.fgx_debug_check_guard_bands.argtypes = [C.c_char_p, C.c_int]
    lib.fgx_debug_guarded_buffers.restype = C.c_int

    def look(what):
        msg = C.create_string_buffer(600)
        bad = lib.fgx_debug_check_guard_bands(msg, 600)
        assert bad == 0, f"{what}: {bad} device buffer(s) written outside their bounds: {msg.value.decode()}"
    g = simulate_grouped_reads(1500, family_size=2, family_size_max=50)
    _run(uc.unmap(g, uc.everything(g), placed=True))
    look("wholly unmapped")
    _run(uc.mixed_every_third_pair(1000, 7, error_rate_ppm=20000)[1])
    look("mixed ends")
    assert lib.fgx_debug_guarded_buffers() >= 20, lib.fgx_debug_guarded_buffers()


def test_unmapped_batches_under_guard_bands():
    run_isolated("test_gpu_unmapped", "check_under_guard_bands", env={"FGX_GUARD_BAND": "4096"}, timeout=600)
