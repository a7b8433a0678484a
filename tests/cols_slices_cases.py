"""The cases of the packed column kernel's scalar state and of its first LDS slice (TEST INFRASTRUCTURE, shared by
tests/test_wavemu_cols_slices.py and tests/test_gpu_cols_slices.py).

k_split_cols<.., 1> keeps a family's uniforms in scalar registers from its descriptor to its result, runs the packed pass once for a family whose
ends have equally many rows and twice — a second copy of the pass — for one whose ends differ, and finds the descriptors of the columns it does
not answer itself (8 bytes each) and their k_call_full items (48 bytes each) in the room behind the family's tile in the wavefront's LDS slice;
a family without that room takes the next launch (larger slices).  Each case is one small batch through the device entry, compared byte for byte
and on the 28 counters with the oracle, and then `fgx_debug_last_split_builds` against what the case is built to do: which build finished the
families, and how many the first launch handed on.

Two kinds of input:
  * `simulate` data as the benchmark has it (inserts N(300, 50), 0.1 % errors): the packed build alone is launched and finishes at least nine
    families in ten (the tolerance of the existing packed tests: the rest is k_simplex_wave2's shape), the classic builds none.  No retries:
    a family needs 56 bytes per column that shows a second base (2400 bases x 0.001 = 2.4 such columns expected, 31 fit the 1776 bytes behind a 16-record tile) and 8 per
    column of the overlap zone that one mate lost to a disagreement; a family of 32 error columns is not in a batch of a few hundred.
  * QUIET families — mates that do not overlap, no errors: every column unanimous, nothing flagged — with bases and qualities edited at chosen
    columns, so that the number of descriptors and items of a family is known exactly.  Every family is then the packed build's, and the
    retries are exactly the families built not to fit."""
import ctypes as C

import numpy as np

import fgx_opts
import orc
from layouts import Rec

FLOOR = 10                       # --min-input-base-quality of the reference CLI
QUIET = dict(insert_mean=420, insert_sd=5, error_rate_ppm=0)      # inserts of 400 - 440 bases: the mates of a 2 x 150 pair are 100 bases apart


def slice_constants(mean_records):
    """(slice, room, item bytes, descriptor bytes) of the first packed launch, from the library's own constants."""
    from fgumi_amd._lib import lib
    lib.fgx_debug_split_first_slice.restype = None
    lib.fgx_debug_split_first_slice.argtypes = [C.c_double, C.c_int, C.POINTER(C.c_uint32)]
    o = (C.c_uint32 * 4)()
    lib.fgx_debug_split_first_slice(float(mean_records), 1, o)
    return tuple(int(x) for x in o)


def _groups(g):
    return [[Rec(r) for r in g.records(i)] for i in range(g.n_grp)]


def _pack(groups):
    from fgumi_amd import GroupedReads
    return GroupedReads.from_groups([[r.encode() for r in recs] for recs in groups])


def _end(recs, r2):
    return [r for r in recs if bool(r.flag & 0x80) == r2] if any(r.flag & 1 for r in recs) else ([] if r2 else list(recs))


def _set_base(r, pos, code):
    s = bytearray(r.seq)
    s[pos >> 1] = (s[pos >> 1] & 0x0F) | (code << 4) if pos % 2 == 0 else (s[pos >> 1] & 0xF0) | code
    r.seq = bytes(s)


def _base(r, pos):
    return (r.seq[pos >> 1] >> 4) if pos % 2 == 0 else (r.seq[pos >> 1] & 15)


def second_base(end, pos):
    """Half of the end's rows show another base at `pos`: a column the packed pass hands to k_call_full (one descriptor + one item per 16 rows)."""
    for r in end[len(end) // 2:]:
        _set_base(r, pos, {1: 2, 2: 4, 4: 8, 8: 1}.get(_base(r, pos), 1))


def one_observation(end, pos):
    """Every row but the first falls below the quality floor at `pos`: a column of ONE observation — a descriptor, answered from the table, no item."""
    for i, r in enumerate(end):
        q = bytearray(r.qual)
        q[pos] = 30 if i == 0 else FLOOR - 5
        r.qual = bytes(q)


def noisy_family(recs, n_items, n_desc_only):
    """`n_items` columns with a second base and `n_desc_only` columns of one observation, spread over both ends from position 8 on, every 3rd base."""
    ends = [_end(recs, False), _end(recs, True)]
    cols = [(e, p) for p in range(8, 140, 3) for e in (0, 1)]
    assert n_items + n_desc_only <= len(cols), (n_items, n_desc_only)
    for k in range(n_items):
        second_base(ends[cols[k][0]], cols[k][1])
    for k in range(n_items, n_items + n_desc_only):
        one_observation(ends[cols[k][0]], cols[k][1])


def make_case(name):
    """-> (GroupedReads, dict(packed=exact count or None, min_packed=..., classic=0, retries=..., build=1))."""
    from fgumi_amd import simulate_grouped_reads
    if name == "a_flagship_64":                  # the benchmark's shape at its smallest: 16 workgroups of four families
        g = simulate_grouped_reads(64, family_size=8)
        return g, dict(min_packed=58, retries=0)
    if name == "b_unequal_ends":
        # quiet families of 8 pairs; every 4th from 1 on becomes a fragment-only family (its R1 reads, unpaired), the one after it loses the R2 reads of
        # two pairs (8 + 6 rows: the two-run path, both runs with columns for k_call_full), so that the four wavefronts of a workgroup hold a pair
        # family in one run, a fragment family, a family in two runs and another pair family
        groups = _groups(simulate_grouped_reads(48, family_size=8, **QUIET))
        for i in range(1, 48, 4):
            frags = _end(groups[i], False)
            for r in frags:
                r.flag &= 0x10
                r.mate_ref, r.mate_pos, r.tlen = -1, -1, 0
                r.tags = [t for t in r.tags if t[0] != b"MC"]
            groups[i] = frags
            recs = groups[i + 1]
            gone = {r.name for r in _end(recs, True)[:2]}
            groups[i + 1] = recs = [r for r in recs if not (r.flag & 0x80 and r.name in gone)]
            assert len(_end(recs, False)) == 8 and len(_end(recs, True)) == 6
            for p in (11, 77):
                second_base(_end(recs, False), p)
                second_base(_end(recs, True), p + 1)
        return _pack(groups), dict(packed=48, retries=0)
    if name == "c_lengths_147_151":              # the last group of eight pulled back (147) or one position into a 19th group (151); R2 ends are reverse
        a, b = simulate_grouped_reads(40, family_size=8, read_length=147), simulate_grouped_reads(40, family_size=8, read_length=151, seed=43)
        groups = [x for pair in zip(_groups(a), _groups(b)) for x in pair]
        return _pack(groups), dict(min_packed=72, retries=0)
    if name == "d_length_100":                   # rows of 112 + 56 bytes: the generic-stride packed build
        return simulate_grouped_reads(64, family_size=8, read_length=100), dict(min_packed=58, retries=0)
    if name == "e_slice_room":
        groups = _groups(simulate_grouped_reads(24, family_size=8, **QUIET))
        _, room, item, desc = slice_constants(16)
        a = room // (item + desc)
        b = (room - a * (item + desc)) // desc
        assert a >= 4 and a * (item + desc) + b * desc == room, (room, item, desc)     # descriptors + items fill the room to the byte
        noisy_family(groups[5], a, b)            # fits exactly: stays in the first launch
        noisy_family(groups[10], a + 1, b)       # one item more: the second launch
        noisy_family(groups[15], 2 * a, b)       # about twice the room: the second launch (its slice is twice the first)
        return _pack(groups), dict(packed=24, retries=2)
    if name == "f_two_items_per_column":         # ends of 20 rows: a column's observations travel as two consecutive items, the family's items in ONE list
        groups = _groups(simulate_grouped_reads(2, family_size=20, **QUIET))
        for recs in groups:
            for p in (9, 64, 133):
                second_base(_end(recs, False), p)
            second_base(_end(recs, True), 40)
        return _pack(groups), dict(packed=2, retries=0)
    raise KeyError(name)


def check_oracle_accepts(name):
    """(CPU, the oracle alone) the crafted families are called, not refused: a consensus record per end of every family, so that a refusal cannot hide
    a miss of the kernels."""
    g, _ = make_case(name)
    want = orc.process(fgx_opts.defaults(min_reads=1), g.blob, g.rec_off, g.rec_len, g.grp_first)
    ends = sum(1 + any(r.flag & 0x80 for r in recs) for recs in _groups(g))
    assert want["count"] == ends, (want["count"], ends)
    assert int(want["stats"][0]) > 0


def check_builds(name, n_families, expect, builds):
    packed, classic, build, retries = builds
    print(f"{name}: families {n_families}, packed build {packed}, classic builds {classic}, first-stage build {build}, first-stage retries {retries}")
    assert build == 1 and classic == 0, builds
    if "packed" in expect:
        assert packed == expect["packed"] == n_families, (builds, expect)
    else:
        assert expect["min_packed"] <= packed <= n_families and expect["min_packed"] >= 0.9 * n_families, (builds, expect)
    assert retries == expect["retries"], (builds, expect)


def _builds(lib, h):
    lib.fgx_debug_last_split_builds.restype = None
    lib.fgx_debug_last_split_builds.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    b = (C.c_uint64 * 4)()
    lib.fgx_debug_last_split_builds(h, b)
    return [int(x) for x in b]


def check_emulated(name):
    """Through fgx_process_batch_device of the emulation library (FGX_LIB): host arrays stand in for the tensors in HBM."""
    from fgumi_amd._lib import Options, Output, lib
    g, expect = make_case(name)
    o = fgx_opts.defaults(min_reads=1)
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
        check_builds(name, g.n_grp, expect, _builds(lib, h))
    finally:
        lib.fgx_destroy(h)


def check_gpu(name):
    """Through the device entry on the GPU (tensors in HBM)."""
    import torch  # noqa: F401
    from fgumi_amd import VanillaUmiConsensusCaller, VanillaUmiConsensusOptions, lib
    g, expect = make_case(name)
    want = orc.process(fgx_opts.defaults(min_reads=1), g.blob, g.rec_off, g.rec_len, g.grp_first)
    c = VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(min_reads=1, min_consensus_base_quality=2, cell_tag="CB", min_input_base_quality=FLOOR),
                                  overlapping_consensus=True)
    try:
        out = c.process_batch_device(g.to_device())
        assert out.n_deferred == 0
        assert out.count == want["count"] and out.to_host() == want["data"]
        assert np.array_equal(np.array(c.last_stats_array, dtype=np.uint64), want["stats"])
        check_builds(name, g.n_grp, expect, _builds(lib, c._h))
    finally:
        c.close()
