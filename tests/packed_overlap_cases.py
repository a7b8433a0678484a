"""The cases of the packed column kernel's overlap step on packed words (TEST INFRASTRUCTURE, shared by tests/test_wavemu_packed_overlap.py and
tests/test_gpu_packed_overlap.py): k_split_cols<.., 1> corrects the overlapping bases of a family's mates eight positions per lane
(simplex_split.inc phase 2a, packed_core.h ov_step); a family with a shared quality of 128 or more, and every family when
FGX_S2_PACKED_OVERLAP=0, keeps the byte-wise steps.  Each case is one batch of depth-8 families through the device entry, compared byte for
byte and counter for counter with the oracle, and then the step its families took (fgx_debug_last_packed_overlap) against the batch's own
positions and lengths."""
import ctypes as C

import numpy as np

import fgx_opts
import orc

FLOOR = 10

# name -> (simulate_grouped_reads arguments, floor, edit of the blob)
GEOMETRY = {}
for _L in (150, 147, 151):
    for _ins, _what in ((299, "1"), (293, "7"), (237, "63"), (152, "148"), (120, "full"), (400, "none")):
        GEOMETRY[f"len{_L}_insert{_ins}_overlap_{_what}"] = (dict(family_size=8, read_length=_L, insert_mean=_ins, insert_sd=3), FLOOR, None)
CONTENT = {
    "code_15_in_shared_positions": (dict(family_size=8), FLOOR, "n"),
    "floor_30_drops_on_agreements": (dict(family_size=8), 30, None),
    # (floor 0 was asked for; under floor 7 no depth-8 family is the packed build's — eight agreeing observations are no certain cap there —
    # and the step would not run: the lowest floor that reaches it stands in.  Floor 0 itself: tests/test_packed_overlap_core.py.)
    "floor_7_the_lowest_of_the_packed_build": (dict(family_size=8), 7, None),
    "quality_128_and_200_in_shared_positions": (dict(family_size=8), FLOOR, "high"),
}
CASES = dict(GEOMETRY, **CONTENT)


def _records(g, fam):
    """(flag, pos, l_seq, offset of SEQ in the blob) of the family's records."""
    out = []
    for r in range(int(g.grp_first[fam]), int(g.grp_first[fam + 1])):
        b = int(g.rec_off[r])
        h = g.blob[b:b + 32]
        l_name, n_cig = int(h[8]), int(h[12]) | (int(h[13]) << 8)
        flag = int(h[14]) | (int(h[15]) << 8)
        pos = int.from_bytes(bytes(h[4:8]), "little", signed=True)
        l_seq = int.from_bytes(bytes(h[16:20]), "little")
        out.append((flag, pos, l_seq, b + 32 + l_name + 4 * n_cig))
    return out


def shared(g, fam):
    """The shared bases of the family's pairs from its own records (one geometry per family: simgen.h): (records of the earlier mates, records of
    the later mates, first shared base of an earlier mate, number of shared bases) — the later mates share their bases from 0."""
    recs = _records(g, fam)
    r1, r2 = [x for x in recs if x[0] & 0x40], [x for x in recs if x[0] & 0x80]
    assert r1 and len(r1) == len(r2)
    (_, p1, l1, _), (_, p2, l2, _) = r1[0], r2[0]
    lo, hi = max(p1, p2), min(p1 + l1, p2 + l2)
    early, late = (r1, r2) if p1 <= p2 else (r2, r1)
    return early, late, lo - min(p1, p2), max(0, hi - lo)


def overlapping_families(g):
    return {fam for fam in range(g.n_grp) if shared(g, fam)[3] > 0}


def _set_code(g, seq_off, p, code):
    sh = 0 if p & 1 else 4
    g.blob[seq_off + p // 2] = (int(g.blob[seq_off + p // 2]) & ~(15 << sh) & 0xFF) | (code << sh)


def write_n(g, step=5):
    """Code 15 at the first, the last and a middle shared base of one mate of every `step`-th overlapping family, the earlier and the later
    mate and the family's first and last pair in turn; in every fourth chosen family at the SAME shared base of both mates as well."""
    combo = 0
    for fam in sorted(overlapping_families(g))[::step]:
        early, late, off, cn = shared(g, fam)
        pair = 0 if combo % 2 == 0 else len(early) - 1
        for w in {0, cn - 1, cn // 2}:
            if (combo // 2) % 2 == 0:
                _set_code(g, early[pair][3], off + w, 15)
            else:
                _set_code(g, late[pair][3], w, 15)
        if combo % 4 == 3:
            _set_code(g, early[pair][3], off + cn // 3, 15)
            _set_code(g, late[pair][3], cn // 3, 15)
        combo += 1
    assert combo >= 8, combo


def write_high(g, step=7):
    """A quality byte of 128 or of 200 at a shared base — the first, the last, a middle one — of one mate of every `step`-th family.  Returns the
    chosen families with overlapping mates: the guard's."""
    chosen = set()
    combo = 0
    for fam in range(0, g.n_grp, step):
        early, late, off, cn = shared(g, fam)
        if cn == 0:
            continue
        pair = 0 if combo % 2 == 0 else len(early) - 1
        w = (0, cn - 1, cn // 2)[(combo // 4) % 3]
        rec, p = (early[pair], off + w) if (combo // 2) % 2 == 0 else (late[pair], w)
        g.blob[rec[3] + (rec[2] + 1) // 2 + p] = 128 if combo % 2 == 0 else 200
        chosen.add(fam)
        combo += 1
    assert combo >= 12, combo
    return chosen


def make_case(name, n_families):
    """-> (GroupedReads, oracle options, floor, families with overlapping mates, the guard's families)."""
    from fgumi_amd import simulate_grouped_reads
    sim, floor, edit = CASES[name]
    g = simulate_grouped_reads(n_families, **sim)
    guard = set()
    if edit == "n":
        write_n(g)
    elif edit == "high":
        guard = write_high(g)
    ov = overlapping_families(g)
    if name.endswith("overlap_none"):
        assert not ov
    elif name.endswith("overlap_1") and "len147" in name:
        pass                                             # (2 x 147 < 299: few families overlap, by a base or two)
    else:
        assert len(ov) >= 0.4 * n_families, len(ov)
    return g, fgx_opts.defaults(min_reads=1, min_input_base_quality=floor), floor, ov, guard


def _counters(lib, h):
    lib.fgx_debug_last_split_builds.restype = None
    lib.fgx_debug_last_split_builds.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.fgx_debug_last_packed_overlap.restype = None
    lib.fgx_debug_last_packed_overlap.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    b, r = (C.c_uint64 * 4)(), (C.c_uint64 * 3)()
    lib.fgx_debug_last_split_builds(h, b)
    lib.fgx_debug_last_packed_overlap(h, r)
    return [int(x) for x in b], [int(x) for x in r]


def check_steps(name, n_families, ov, guard, builds, steps, switched_off=False):
    """The steps the families took against the batch's own geometry.  A family outside the packed build (at most 10 % of a depth-8 batch: the
    tolerance of packed_rows_cases.check_rows) reports nothing; the counters are then bounded from both sides, and exact where every family took
    the packed build."""
    n_packed_build, (packed, bytewise, guarded) = builds[0], steps
    print(f"{name}: families {n_families}, packed build {n_packed_build}, overlapping {len(ov)}, packed step {packed}, byte-wise {bytewise}, guard {guarded}, chosen {len(guard)}")
    assert n_packed_build >= 0.9 * n_families, builds
    outside = n_families - n_packed_build
    assert len(ov) - outside <= packed + bytewise <= len(ov), (builds, steps, len(ov))
    assert guarded <= bytewise
    if switched_off:
        assert packed == 0 and guarded == 0, steps
        return
    assert len(guard) - outside <= guarded <= len(guard), (builds, steps, len(guard))
    assert bytewise == guarded, steps                      # every other family with overlapping mates: the packed step
    if not guard:
        assert guarded == 0 and bytewise == 0 and len(ov) - outside <= packed <= len(ov), (builds, steps, len(ov))


def check_emulated(name, n_families, switched_off=False):
    """Through fgx_process_batch_device of the emulation library (FGX_LIB): host arrays stand in for the tensors in HBM."""
    from fgumi_amd._lib import Options, Output, lib
    g, o, _, ov, guard = make_case(name, n_families)
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
        check_steps(name, n_families, ov, guard, *_counters(lib, h), switched_off=bool(switched_off))
    finally:
        lib.fgx_destroy(h)


def check_gpu(name, n_families, switched_off=False):
    """Through the device entry on the GPU (tensors in HBM)."""
    import torch  # noqa: F401
    from fgumi_amd import VanillaUmiConsensusCaller, VanillaUmiConsensusOptions, lib
    g, o, floor, ov, guard = make_case(name, n_families)
    want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first)
    c = VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(min_reads=1, min_consensus_base_quality=2, cell_tag="CB", min_input_base_quality=floor),
                                  overlapping_consensus=True)
    try:
        out = c.process_batch_device(g.to_device())
        assert out.n_deferred == 0
        assert out.count == want["count"] and out.to_host() == want["data"]
        assert np.array_equal(np.array(c.last_stats_array, dtype=np.uint64), want["stats"])
        check_steps(name, n_families, ov, guard, *_counters(lib, c._h), switched_off=bool(switched_off))
    finally:
        c.close()
