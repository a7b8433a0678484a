"""The cases of the packed column pass's two row loops (TEST INFRASTRUCTURE, shared by tests/test_wavemu_packed_rows.py and
tests/test_gpu_packed_rows.py): k_split_cols<.., 1> tests every family once — is each raw quality, at the positions below its read's own
length, at or above --min-input-base-quality? — and a CLEAN family's rows are counted without a quality read (simplex_split.inc phase 1b,
packed_core.h).  Each case is one batch through the device entry, compared byte for byte and counter for counter with the oracle, and then
the row loops its families took (fgx_debug_last_packed_rows) against what the batch's own quality bytes say."""
import ctypes as C

import numpy as np

import fgx_opts
import orc

FLOOR = 10                       # --min-input-base-quality of the reference CLI
POSITIONS = (0, 7, 8, 15, 16, -1)   # where case d lowers a byte: the edges of the first groups of eight, and l_seq - 1


def _records(g, fam):
    """(record index, flag, l_seq, offset of QUAL in the blob, tlen) of the family's records."""
    out = []
    for r in range(int(g.grp_first[fam]), int(g.grp_first[fam + 1])):
        b = int(g.rec_off[r])
        h = g.blob[b:b + 32]
        l_name, n_cig = int(h[8]), int(h[12]) | (int(h[13]) << 8)
        flag = int(h[14]) | (int(h[15]) << 8)
        l_seq = int.from_bytes(bytes(h[16:20]), "little")
        tlen = int.from_bytes(bytes(h[28:32]), "little", signed=True)
        out.append((r, flag, l_seq, b + 32 + l_name + 4 * n_cig + (l_seq + 1) // 2, tlen))
    return out


def raw_dirty_families(g, floor):
    """The families that hold a quality byte below the floor at a position below l_seq: what the clean test has to find."""
    dirty = set()
    for fam in range(g.n_grp):
        for _, _, l_seq, qo, _ in _records(g, fam):
            if (g.blob[qo:qo + l_seq] < floor).any():
                dirty.add(fam)
                break
    return dirty


def lower_bytes(g, value, step=7):
    """Case d / e: in every `step`-th family ONE quality byte becomes `value` — position POSITIONS[i], in the first or the last record of the
    R1 or the R2 end, all 24 combinations in turn.  Returns {family: overlapping mates?}."""
    chosen = {}
    combo = 0
    for fam in range(0, g.n_grp, step):
        recs = _records(g, fam)
        ends = [[x for x in recs if x[1] & 0x40], [x for x in recs if x[1] & 0x80]]
        end = ends[(combo // 2) % 2]
        if not end:
            continue
        rec = end[0] if combo % 2 == 0 else end[-1]
        pos = POSITIONS[(combo // 4) % len(POSITIONS)]
        _, _, l_seq, qo, tlen = rec
        g.blob[qo + (l_seq - 1 if pos < 0 else pos)] = value
        chosen[fam] = abs(tlen) < 2 * l_seq
        combo += 1
    assert combo >= 24 and any(chosen.values()) and not all(chosen.values()), (combo, sum(chosen.values()))   # every combination; with and without overlapping mates
    return chosen


def make_case(name, n_families):
    """-> (GroupedReads, oracle options, expected general families or None (= whatever the raw bytes say), floor)."""
    from fgumi_amd import simulate_grouped_reads
    floor, sim, expect = FLOOR, dict(family_size=8), None
    if name == "b_length_147":        # three qualities in the last 16-byte chunk, tag text (a NUL included) behind them
        sim = dict(family_size=8, read_length=147)
    elif name == "c_floor_30":        # the raw qualities of cycles 0 - 4 lie below: every family is general
        floor = 30
    elif name in ("e_floor_11_byte_11", "e_floor_11_byte_10"):
        floor = 11
    elif name == "f_long_tail":
        sim = dict(family_size=2, family_size_max=50)
    g = simulate_grouped_reads(n_families, **sim)
    if name == "d_one_byte_below":
        expect = set(lower_bytes(g, FLOOR - 1))
    elif name == "e_floor_11_byte_11":
        lower_bytes(g, 11)
        expect = set()
    elif name == "e_floor_11_byte_10":
        expect = set(lower_bytes(g, 10))
    dirty = raw_dirty_families(g, floor)
    if name in ("a_depth8", "b_length_147"):
        assert not dirty                              # (simgen.h quality_at: no raw quality below 16)
    elif name == "c_floor_30":
        assert len(dirty) == n_families
    elif expect is not None:
        assert dirty == expect
    return g, fgx_opts.defaults(min_reads=1, min_input_base_quality=floor), dirty, floor


def _counters(lib, h):
    lib.fgx_debug_last_split_builds.restype = None
    lib.fgx_debug_last_split_builds.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.fgx_debug_last_packed_rows.restype = None
    lib.fgx_debug_last_packed_rows.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    b, r = (C.c_uint64 * 4)(), (C.c_uint64 * 2)()
    lib.fgx_debug_last_split_builds(h, b)
    lib.fgx_debug_last_packed_rows(h, r)
    return [int(x) for x in b], [int(x) for x in r]


def check_rows(name, n_families, dirty, builds, rows):
    """The row loops against the batch's own bytes.  A family outside the packed build (at most 10 % of a depth-8 batch: the existing tolerance)
    reports neither; the counters then bound each other, and where every family took the packed build they are exact."""
    packed, (clean, general) = builds[0], rows
    print(f"{name}: families {n_families}, packed build {packed}, clean {clean}, general {general}, raw-dirty {len(dirty)}")
    assert clean + general == packed, (builds, rows)
    if name == "f_long_tail":
        assert packed > 0 and builds[1] > 0, builds
    else:
        assert packed >= 0.9 * n_families, builds
    outside = n_families - packed
    assert len(dirty) - outside <= general <= len(dirty), (builds, rows, len(dirty))
    assert n_families - len(dirty) - outside <= clean <= n_families - len(dirty), (builds, rows, len(dirty))
    if name in ("a_depth8", "b_length_147", "e_floor_11_byte_11"):
        assert general == 0 and clean == packed
    if name == "c_floor_30":
        assert clean == 0 and general == packed


def check_emulated(name, n_families):
    """Through fgx_process_batch_device of the emulation library (FGX_LIB): host arrays stand in for the tensors in HBM."""
    from fgumi_amd._lib import Options, Output, lib
    g, o, dirty, _ = make_case(name, n_families)
    want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=50)
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
        assert int(out.count) == want["count"] and got == want["data"]
        assert np.array_equal(np.array(np.ctypeslib.as_array(out.stats, shape=(28,)), dtype=np.uint64), want["stats"])
        check_rows(name, n_families, dirty, *_counters(lib, h))
    finally:
        lib.fgx_destroy(h)


def check_gpu(name, n_families):
    """Through the device entry on the GPU (tensors in HBM)."""
    import torch  # noqa: F401
    from fgumi_amd import VanillaUmiConsensusCaller, VanillaUmiConsensusOptions, lib
    g, o, dirty, floor = make_case(name, n_families)
    want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first)
    c = VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(min_reads=1, min_consensus_base_quality=2, cell_tag="CB", min_input_base_quality=floor),
                                  overlapping_consensus=True)
    try:
        out = c.process_batch_device(g.to_device())
        assert out.n_deferred == 0
        assert out.count == want["count"] and out.to_host() == want["data"]
        assert np.array_equal(np.array(c.last_stats_array, dtype=np.uint64), want["stats"])
        check_rows(name, n_families, dirty, *_counters(lib, c._h))
    finally:
        c.close()
