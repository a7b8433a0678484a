"""GPU parity: --max-reads on deep simplex families.  k_deep_parse (simplex_deep.inc) cuts an end above the cap to its `max_reads` lowest fgbio name ranks
(ties in file order, the survivors in file order, the dropped reads counted as Downsampled) in every build — <64, 64> (methylation-aware mode), <128, 128>,
<256, 512> and, for families of 513 .. 1 024 records that fit an end's 255 reads only after the cut, <256, 1024> — and k_deep_cols streams the survivors' rows.
Each test compares the device-resident output with the oracle byte for byte, all 28 counters included, and asserts the path taken: no family deferred, every
family above 64 records finished by the streaming kernels."""
import ctypes as C

import numpy as np
import pytest

import fgx_opts
import orc
from fgumi_amd import MethylationMode, VanillaUmiConsensusCaller, VanillaUmiConsensusOptions, lib, simulate_grouped_reads
from isolated import run_isolated
from max_reads_cases import READ_THROUGH, REJ_DOWNSAMPLED, end_sizes, families_the_cap_bites, families_with_a_tie_cut_in_the_middle, methylation_batch, with_tied_names

pytestmark = pytest.mark.gpu

for _f in ("fgx_debug_last_big_families", "fgx_debug_last_deep_families", "fgx_debug_last_meth_device"):
    getattr(lib, _f).restype = C.c_uint32
    getattr(lib, _f).argtypes = [C.c_void_p]

_BATCHES = {}


def _deep_batch():
    """300 families of 80 .. 300 records (computed once, never modified)."""
    if "deep" not in _BATCHES:
        _BATCHES["deep"] = simulate_grouped_reads(300, family_size=40, family_size_max=150, error_rate_ppm=10000)
    return _BATCHES["deep"]


def _caller(min_reads, max_reads, **kw):
    return VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(min_reads=min_reads, max_reads=max_reads, min_consensus_base_quality=2, cell_tag="CB", **kw),
                                     overlapping_consensus=True)


def _run(g, min_reads=1, max_reads=None, bites=True):
    """tests/test_gpu_deep_families.py::_run with a cap."""
    want = orc.process(fgx_opts.defaults(min_reads=min_reads, max_reads=-1 if max_reads is None else max_reads), g.blob, g.rec_off, g.rec_len, g.grp_first)
    assert (int(want["stats"][3 + REJ_DOWNSAMPLED]) > 0) == bites
    c = _caller(min_reads, max_reads)
    out = c.process_batch_device(g.to_device())
    got = out.to_host()
    path = dict(big=lib.fgx_debug_last_big_families(c._h), deep=lib.fgx_debug_last_deep_families(c._h), deferred=int(out.n_deferred))
    stats = np.array(c.last_stats_array, dtype=np.uint64)
    c.close()
    assert got == want["data"], f"output differs from the oracle ({len(got)} vs {len(want['data'])} bytes; path {path})"
    assert np.array_equal(stats, want["stats"]), (stats.tolist(), want["stats"].tolist())
    return path, want


@pytest.mark.parametrize("cap,share", [(10, 0.9), (50, 0.25)])
def test_cap_on_the_two_and_four_wavefront_builds(cap, share):
    g = _deep_batch()
    n = np.diff(np.asarray(g.grp_first, dtype=np.int64))
    if "deep_ends" not in _BATCHES:
        _BATCHES["deep_ends"] = end_sizes(g).max(axis=1)
    assert n.min() > 64 and (n > 128).sum() > 50 and (_BATCHES["deep_ends"] > cap).sum() >= share * len(n)
    path, _ = _run(g, max_reads=cap)
    assert path["deferred"] == 0 and path["big"] == path["deep"] == len(n), path


def test_consensus_length_comes_from_the_survivors():
    """--min-reads 3 under --max-reads 5 on read-through inserts: the final lengths differ inside an end, and the min_reads-th longest SURVIVOR sets the length."""
    g = simulate_grouped_reads(300, family_size=40, family_size_max=100, **READ_THROUGH)
    n = np.diff(np.asarray(g.grp_first, dtype=np.int64))
    assert n.min() > 64 and families_the_cap_bites(g, 5) == len(n)
    path, _ = _run(g, min_reads=3, max_reads=5)
    assert path["deferred"] == 0 and path["big"] == path["deep"] == len(n), path


def test_families_of_up_to_1024_records_fit_after_the_cut():
    """540 .. 1 000 records, ends of 270 .. 500 reads: under a cap of 100 the <256, 512> build (up to 512 records; the limit of 255 reads per end applies after the
    cut) and the <256, 1024> build finish all of them; without a cap no such family is the streaming kernels' and the host entry finishes the batch."""
    g = simulate_grouped_reads(12, family_size=270, family_size_max=500, error_rate_ppm=5000)
    n = np.diff(np.asarray(g.grp_first, dtype=np.int64))
    assert n.min() >= 540 and n.max() <= 1024 and (n > 512).sum() >= 1
    path, _ = _run(g, max_reads=100)
    assert path["deferred"] == 0 and path["big"] == path["deep"] == 12, path
    want = orc.process(fgx_opts.defaults(min_reads=1), g.blob, g.rec_off, g.rec_len, g.grp_first)
    c = _caller(1, None)
    out = c.process_batch(g)
    assert out.data == want["data"] and np.array_equal(np.array(c.last_stats_array, dtype=np.uint64), want["stats"])
    assert lib.fgx_debug_last_big_families(c._h) == 12 and lib.fgx_debug_last_deep_families(c._h) == 0
    c.close()


@pytest.mark.parametrize("cap", [1, 2, 4])
def test_equal_ranks_at_the_cut_keep_file_order(cap):
    if "ties" not in _BATCHES:
        _BATCHES["ties"] = with_tied_names(simulate_grouped_reads(200, family_size=40, family_size_max=60, error_rate_ppm=10000))
    g = _BATCHES["ties"]
    assert families_with_a_tie_cut_in_the_middle(g, cap) >= 1
    path, _ = _run(g, max_reads=cap)
    assert path["deferred"] == 0 and path["big"] == path["deep"] == 200, path


@pytest.mark.parametrize("mode", [1, 2], ids=["em_seq", "taps"])
def test_methylation_mode(mode):
    """Every family on the streaming kernels (the <64, 64> build): a cap that bites defers nothing."""
    import bamutil
    from fgumi_amd import split_records
    contigs, g = methylation_batch(40 + mode, 1500)
    assert families_the_cap_bites(g, 3) >= 50
    o = fgx_opts.defaults(min_reads=1, max_reads=3, methylation_mode=mode)
    orc.set_reference(contigs)
    try:
        want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first)
    finally:
        orc.set_reference(None)
    assert int(want["stats"][3 + REJ_DOWNSAMPLED]) > 0
    assert sum("cu" in bamutil.parse(r)["tags"] for r in split_records(want["data"])) >= 100
    c = _caller(1, 3, methylation_mode=MethylationMode.EmSeq if mode == 1 else MethylationMode.Taps)
    names = ["chr%d" % (i + 1) for i in range(len(contigs))]
    c.set_reference(dict(zip(names, contigs)), names)
    out = c.process_batch_device(g.to_device())
    assert out.n_deferred == 0, f"{out.n_deferred} of {g.n_grp} groups deferred"
    assert out.to_host() == want["data"]
    assert np.array_equal(np.array(c.last_stats_array, dtype=np.uint64), want["stats"])
    assert lib.fgx_debug_last_meth_device(c._h) == g.n_grp
    c.close()


def test_cap_that_does_not_bite():
    g = _deep_batch()
    p0, w0 = _run(g, bites=False)
    p1, w1 = _run(g, max_reads=10000, bites=False)
    assert p0 == p1 and p1["deferred"] == 0 and p1["deep"] == p1["big"] == g.n_grp and w0["data"] == w1["data"]


def check_run_bam(tmp_dir):
    """fgx_run_bam on the capped deep batch, in one chunk and in many: the oracle's records and counters, no group deferred, no batch through the host entry."""
    import os
    from fgumi_amd import bgzf
    g = _deep_batch()
    want = orc.process(fgx_opts.defaults(min_reads=1, max_reads=50), g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=100000)
    assert int(want["stats"][3 + REJ_DOWNSAMPLED]) > 0
    c = _caller(1, 50)
    refs = [("chr%d" % (i + 1), 2147483647) for i in range(24)]
    src, dst = os.path.join(tmp_dir, "grouped.bam"), os.path.join(tmp_dir, "consensus.bam")
    bgzf.write_bam(src, bgzf.grouped_input_header(refs), refs, g.blob)
    for chunk in (0, 1 << 20):
        st = c.run_bam(src, dst, chunk_raw_bytes=chunk, threads=8)
        _, _, stream, off, ln = bgzf.read_bam(dst)
        got = b"".join(bytes(stream[int(a) - 4:int(a) + int(b)]) for a, b in zip(off, ln))
        print(f"chunk {chunk}: chunks {st['chunks']}, deferred groups {st['deferred_groups']}, host entry batches {st['host_entry_batches']}", flush=True)
        assert got == want["data"], "the consensus BAM's records differ from the oracle's"
        assert st["stats"][:28] == [int(v) for v in want["stats"]]
        assert st["deferred_groups"] == 0 and st["host_entry_batches"] == 0, (st["deferred_groups"], st["host_entry_batches"])
    c.close()


def test_run_bam_on_a_capped_file(tmp_path):
    run_isolated("test_gpu_max_reads_deep", "check_run_bam", str(tmp_path), timeout=600)
