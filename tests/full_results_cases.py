"""The cases of k_call_full's result array (TEST INFRASTRUCTURE, shared by tests/test_wavemu_full_results.py and tests/test_gpu_full_results.py).

For a pair family that the packed build of k_split_cols finished and that emit_pair writes, k_call_full leaves its answers densely in a result
array and emit_pair patches them into the columns it holds (fgumi_amd/csrc/fastpath.h, FullResult); every other answer is scattered into the scratch
planes as before.  Each case is one batch through the device entry, compared byte for byte and on the 28 counters with the oracle, and then
`fgx_debug_last_full_results` — column answers through the array, column answers scattered, families the writer applies, families refused because
their items are not in one piece — against what the case is built to do."""
import ctypes as C

import numpy as np

import fgx_opts
import orc

DEFAULT_ON = True                # the library's default of FGX_FULL_RESULTS (fastpath.h: FGX_FULL_RESULTS_DEFAULT)
LENGTHS = (8, 9, 147, 149, 151, 255, 256)   # odd Lc (the code group starts elsewhere than the others), the pulled-back last group in every alignment


def make_case(name):
    """-> (GroupedReads factory arguments or a GroupedReads, oracle option overrides, what the counters must show)."""
    sim, opts, want = dict(family_size=8), dict(min_reads=1), "most"
    if name.startswith("b_length_"):
        sim = dict(family_size=8, read_length=int(name.rsplit("_", 1)[1]))
        want = "some" if sim["read_length"] >= 16 else "bytes"      # (families of 8- and 9-base reads are not the packed build's: everything is scattered)
    elif name == "c_noisy_2pct":                  # 2 % errors, ~40 items per family: items in column 0, in column Lc - 1, in the zone two lanes hold
        sim = dict(family_size=8, error_rate_ppm=20000)
        want = "some"
    elif name == "c_noisy_5pct":                  # 5 % errors, ~90 items per family: most families hold more than the 64 results a wavefront loads
        sim = dict(family_size=8, error_rate_ppm=50000)
        want = "over"
    elif name == "d_length_257":                  # emit_pair refuses a record of more than 256 columns
        sim = dict(family_size=8, read_length=257, insert_mean=500)
        want = "none"
    elif name == "d_fragments":
        want = "none"
    elif name == "e_long_tail":                   # ends of 17 - 31 rows: two items per column, with continuation items
        sim = dict(family_size=2, family_size_max=50)
        want = "some"
    elif name == "f_min_reads_3":                 # shallow families: N / quality 0 below --min-reads
        sim = dict(family_size=3, family_size_max=12)      # (from 3 pairs up: smaller families are k_simplex_seg's, whose exit the emulator cannot follow)
        opts = dict(min_reads=3)
        want = "some"
    elif name == "f_min_quality_40":              # the masked answers: N / quality 2
        opts = dict(min_reads=1, min_consensus_base_quality=40)
    elif name in ("g_switched_off", "g_unset"):   # FGX_FULL_RESULTS=0 / not set in the child's environment
        want = "none" if name == "g_switched_off" or not DEFAULT_ON else "most"
    elif name == "h_cut_ranges":                  # FGX_POOL_DIV / FGX_POOL_SLACK in the child's environment: lists of a few slots, ranges that cross their ends
        want = "cut"
    return sim, opts, want


def build_batch(name, n_families):
    from fgumi_amd import simulate_grouped_reads
    sim, opts, want = make_case(name)
    g = simulate_grouped_reads(n_families, **sim)
    if name == "d_fragments":                     # every family keeps its R1 reads, unpaired: single-end families
        from cols_slices_cases import _end, _groups, _pack
        groups = _groups(g)
        for i, recs in enumerate(groups):
            frags = _end(recs, False)
            for r in frags:
                r.flag &= 0x10
                r.mate_ref, r.mate_pos, r.tlen = -1, -1, 0
                r.tags = [t for t in r.tags if t[0] != b"MC"]
            groups[i] = frags
        g = _pack(groups)
    return g, opts, want


def counters(lib, h):
    lib.fgx_debug_last_full_results.restype = None
    lib.fgx_debug_last_full_results.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.fgx_debug_last_split_builds.restype = None
    lib.fgx_debug_last_split_builds.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.fgx_debug_last_full_results_over.restype = C.c_uint64
    lib.fgx_debug_last_full_results_over.argtypes = [C.c_void_p]
    r, b = (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
    lib.fgx_debug_last_full_results(h, r)
    lib.fgx_debug_last_split_builds(h, b)
    return [int(x) for x in r] + [int(lib.fgx_debug_last_full_results_over(h))], [int(x) for x in b]


def no_call_positions(data):
    """Positions of the consensus records (a BAM record stream) that show N with quality 0: what a column below --min-reads leaves."""
    n, p = 0, 0
    while p < len(data):
        size = int.from_bytes(data[p:p + 4], "little")
        l_name, n_cig = data[p + 12], int.from_bytes(data[p + 16:p + 18], "little")
        l_seq = int.from_bytes(data[p + 20:p + 24], "little")
        seq = p + 36 + l_name + 4 * n_cig
        qual = seq + (l_seq + 1) // 2
        for i in range(l_seq):
            code = (data[seq + (i >> 1)] >> 4) if i % 2 == 0 else (data[seq + (i >> 1)] & 15)
            n += 1 if code == 15 and data[qual + i] == 0 else 0
        p += 4 + size
    return n


def check_path(name, n_families, want, res, builds, data=b""):
    """The path the answers took ("bytes": whatever the families' shapes give; the bytes were compared before).  `data`: the records, equal to the oracle's."""
    arr, scat, applied, cut, over = res
    print(f"{name}: families {n_families}, packed build {builds[0]}, writer applies {applied} ({applied / n_families:.3f}), not in one piece {cut}, more than 64 items {over}, "
          f"answers through the array {arr}, scattered {scat}")
    assert applied + cut + over <= builds[0] <= n_families, (res, builds)      # only families of the packed build
    if want != "cut":
        assert cut == 0, res                       # (lists of the default size end far behind a small batch's items)
    if want == "most":
        assert over == 0, res                      # (3.3 items per depth-8 family at 0.1 % errors)
    if name == "f_min_reads_3":
        # families of 3 pairs under --min-reads 3: a column of the read-through zone that lost an observation to the overlap correction is below the
        # floor, and where its remaining observations disagree it is an item — its answer is N / quality 0.  The records (equal to the oracle's) must show such positions.
        masked = no_call_positions(data)
        print(f"{name}: positions N / quality 0 in the records: {masked}")
        assert masked > 0
    if want == "none":
        assert arr == 0 and applied == 0 and cut == 0 and over == 0, res
        return
    if applied == n_families:                      # every family's answers go through the array: nothing may be scattered
        assert scat == 0, res
    if want == "most":
        # the issue's bound.  Every pair family of the packed build is applied (its items are in one piece unless the list ends inside them), and the
        # packed build takes at least nine depth-8 families in ten (the existing tolerance of the packed tests)
        assert applied >= 0.9 * n_families, res
        assert applied == builds[0] and cut == 0, (res, builds)
        assert arr > 0, res
    elif want == "some":
        assert applied > 0 and arr > 0, res
    elif want == "cut":                            # ranges that a list's end cuts: refused for that reason alone
        assert cut > 0 and over == 0 and applied > 0 and arr > 0 and scat > 0, res
    elif want == "over":                           # families of more than 64 items: refused for that reason alone
        assert over > 0 and cut == 0 and applied > 0 and arr > 0 and scat > 0, res


def check_emulated(name, n_families):
    """Through fgx_process_batch_device of the emulation library (FGX_LIB): host arrays stand in for the tensors in HBM."""
    from fgumi_amd._lib import Options, Output, lib
    g, opts, want = build_batch(name, n_families)
    o = fgx_opts.defaults(**opts)
    ref = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=50)
    po = Options.from_buffer_copy(bytes(o))
    h = lib.fgx_create(C.byref(po))
    assert h, lib.fgx_global_error().decode()
    try:
        blob = np.concatenate([g.blob, np.zeros(64, dtype=np.uint8)])
        out, nd, dp = Output(), C.c_uint32(), C.c_void_p()
        rc = lib.fgx_process_batch_device(h, blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, g.grp_first.ctypes.data, g.n_grp,
                                          C.byref(out), C.byref(nd), C.byref(dp))
        assert rc == 0, lib.fgx_last_error(h).decode()
        assert nd.value == 0, nd.value
        got = C.string_at(out.data, out.data_len) if out.data_len else b""
        assert int(out.count) == ref["count"] and got == ref["data"]
        assert np.array_equal(np.array(np.ctypeslib.as_array(out.stats, shape=(28,)), dtype=np.uint64), ref["stats"])
        check_path(name, n_families, want, *counters(lib, h), got)
    finally:
        lib.fgx_destroy(h)


def check_gpu(name, n_families):
    """Through the device entry on the GPU (tensors in HBM)."""
    import torch  # noqa: F401
    from fgumi_amd import VanillaUmiConsensusCaller, VanillaUmiConsensusOptions, lib
    g, opts, want = build_batch(name, n_families)
    o = fgx_opts.defaults(**opts)
    ref = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first)
    c = VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(min_reads=opts.get("min_reads", 1), min_consensus_base_quality=opts.get("min_consensus_base_quality", 2),
                                                                      cell_tag="CB"), overlapping_consensus=True)
    try:
        out = c.process_batch_device(g.to_device())
        assert out.n_deferred == 0
        got = out.to_host()
        assert out.count == ref["count"] and got == ref["data"]
        assert np.array_equal(np.array(c.last_stats_array, dtype=np.uint64), ref["stats"])
        check_path(name, n_families, want, *counters(lib, c._h), got)
    finally:
        c.close()


def check_whole_rule():
    """full_range_whole (fastpath.h), the decision "the family's items lie in one piece", as the host-callable export: a reservation of `items` slots at
    `base` of a list of `cap` slots is whole iff it ends inside the list."""
    from fgumi_amd._lib import lib
    lib.fgx_debug_full_range_whole.restype = C.c_int
    lib.fgx_debug_full_range_whole.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    for base, items, cap, whole in [(0, 1, 1, 1), (0, 2, 1, 0), (5, 3, 8, 1), (5, 4, 8, 0), (8, 1, 8, 0), (9, 1, 8, 0), (0, 0, 8, 1), (7, 1, 8, 1),
                                    (0xFFFFFFF0, 0x20, 0xFFFFFFFF, 0), (0x7FFFFFFE, 1, 0x7FFFFFFF, 1), (0xFFFFFFFF, 0xFFFFFFFF, 16, 0)]:
        assert lib.fgx_debug_full_range_whole(base, items, cap) == whole, (base, items, cap, whole)
