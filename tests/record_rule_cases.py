"""Edge records at the call sites of the record rules (fgumi_amd/csrc/record_core.h) — TEST INFRASTRUCTURE shared by tests/test_wavemu_record_rules.py
(host arrays, the wave emulator) and tests/test_gpu_record_rules.py (tensors in HBM).

One small batch per (head of the launch chain, edge): plain simulated families, and the last family (the last four under k_simplex_seg<4>) carrying one edge record each.  Each batch goes through
both entries of the library against the oracle (bytes and the 28 counters; where the oracle raises, the product refuses — layout_runs' rules), and the
ROUTE the batch took is compared with ROUTES below: was the edge family decided on the device or deferred, how many kernels the chain launched (a family handed from one kernel to the next adds launches), how many families left the first kernel for
the next one (`routed`), how many went to the workgroup kernel (`big`), the streaming kernels (`deep`) and the wide kernels (`wide`), which column builds
ran.  The table was recorded from the commit BEFORE the parsers were rewritten over record_core.h, under the wave emulator; the test fails on any change.
RULES gives, per edge, the source rule that explains its routes.

Family sizes are counted in PAIRS by simulate_grouped_reads, so the heads' smallest families are 6 / 16 / 66 / 514 records where the issue says 3 / 8 / 65 / 513.
Heads (pairs per family -> records): seg4 3 -> 6, packed 8 -> 16, pair 2 .. 50, wave2 4 -> 8 (FGX_SPLIT=0), deep 33 -> 66 (the smallest even family above
64 records), indel 4 -> 8 with an insertion read in the edge family (the workgroup kernel k_family), wide 257 -> 514 records of 20 bases (FGX_DEEP_WIDE=1:
an end of more than 255 reads)."""
import ctypes as C
import json
import os

import numpy as np

import fgx_opts
import layout_runs as LR
import layouts
from layouts import Rec

HEADS = {
    # head: (families, simulate_grouped_reads arguments, environment, edge families).  The edge record sits in the LAST `edge families` families.  k_simplex_seg<4> (the
    # seg4 and wave2 heads) holds four consecutive families in a wavefront, and the emulator wants all 64 lanes at every cross-lane operation: a family that leaves the
    # kernel beside three that stay ends the emulation (not the hardware), and so does a wavefront that is not full — there the last FOUR families carry the edge
    # and leave together.  For the split kernel and k_simplex_seg<2> one family is enough, alone behind a multiple of four.
    "seg4": (12, dict(family_size=3), {}, 4),
    "packed": (13, dict(family_size=8), {}, 1),
    "pair": (17, dict(family_size=2, family_size_max=50), {}, 1),
    "wave2": (8, dict(family_size=4), {"FGX_SPLIT": "0"}, 4),
    "deep": (3, dict(family_size=33), {}, 1),
    "indel": (9, dict(family_size=4), {}, 1),
    "wide": (2, dict(family_size=257, read_length=20), {"FGX_DEEP_WIDE": "1"}, 1),
}
MC_FORMS = ["1M", "9999999M", "10000000M", "0M", "00M", "M", "5S", "5M5S", "+5M", " 5M", "", "7", "1234M", "12345M", "123456M", "1234567M", "12345678M", "150M"]
NAME_LENGTHS = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 43, 44, 254]
EDGES = ([f"mc:{f}" for f in MC_FORMS] + [f"mpos:{v}" for v in (-1, 0, (1 << 30) - 1, 1 << 30)] + [f"name:{n}" for n in NAME_LENGTHS] +
         ["no_mi_first", "q0_ff", "all_ff", "paired_no_first_last", "frag_first", "secondary", "rx:255", "rx:256"])

RULES = {
    "mc": "an MC that is not `<n>M` (1 - 7 digits, n > 0) is not the closed form's: the streaming parsers hand the family on (record::mc_single_m == 0 -> odd), "
          "k_family_wave<0> / k_family take it through bam::mate_clip; `<n>M` stays in the head's kernel with record::single_m_mate_clip",
    "mpos": "a mate position outside [0, 2^30) is outside the closed form's range (record::mate_in_range): handed on like a foreign MC; k_family_wave<0> uses bam::mate_clip",
    "name": "the pairing hash (record::name_hash30) takes any length; l_name + 4 > 48 (names of 44 bytes and more) is beyond k_split_parse's head window "
            "(streaming_header_odd's head_window): k_simplex_wave2 takes the family; the other heads keep it",
    "no_mi_first": "the first record must carry the MI tag (record::first_record_odd; vanilla_caller.rs:1897-1908): fatal in the reference, the oracle raises, the product refuses",
    "q0_ff": "a first quality of 0xFF sends the family on (the first one decides in the streaming parsers, vanilla_caller.rs:1119-1124); k_family_wave<0> / k_family look at all of them: real qualities follow, the read is called",
    "all_ff": "absent qualities (all 0xFF) are fatal in the reference (vanilla_caller.rs:1119-1124): the oracle raises, the product refuses",
    "paired_no_first_last": "a paired record without FIRST or LAST is counted but in no end (record::streaming_flags_odd): the streaming parsers hand the family on",
    "frag_first": "an unpaired record with FIRST: k_split_parse alone refuses it (frag_with_mate_flags_odd: the family is routed on), the other streaming parsers keep it in their parse; "
                  "the family then has a fragment end beside its R1 and R2 ends — three consensus reads: k_simplex_wave2 / k_simplex_seg call it, the streaming and the wide kernels "
                  "hand such a family to k_family after the parse (`has_frag && has_pair`), which takes the 66 records of the deep head and not the 514 of the wide head: deferred there",
    "secondary": "a secondary record is refused by the streaming shape (record::streaming_flags_odd); k_family_wave<0> / k_family exclude it from the ends",
    "rx": "an RX value above 255 bytes is reported by aux_walk (oddw): no device kernel takes the family; 255 bytes are taken",
}


def options():
    return fgx_opts.defaults(kind=0, min_reads=1)


def _rename(recs, old, new):
    for r in recs:
        if r.name == old:
            r.name = new


def _set_tag(r, key, value):
    r.tags = [(k, t, (value + b"\0") if k == key else v) for k, t, v in r.tags]


def apply_edge(recs, edge):
    """The edge record is record 0 of the family (its mate keeps its own shape)."""
    kind, _, arg = edge.partition(":")
    r = recs[0]
    if kind == "mc":
        assert r.tag(b"MC") is not None
        _set_tag(r, b"MC", arg.encode())
    elif kind == "mpos":
        r.mate_pos = int(arg)
    elif kind == "name":
        n = int(arg)
        _rename(recs, r.name, (b"edge" * 64)[:n])
    elif kind == "no_mi_first":
        r.tags = [t for t in r.tags if t[0] != b"MI"]
    elif kind == "q0_ff":
        r.qual = b"\xff" + r.qual[1:]
    elif kind == "all_ff":
        r.qual = b"\xff" * r.l_seq
    elif kind == "paired_no_first_last":
        r.flag &= ~0xC0
    elif kind == "frag_first":
        # the first TWO records that carry FIRST become fragments that still carry it.  Two, not one: an end of ONE read with an RX value takes a line of
        # k_family_wave<0>'s UMI phase that reads another lane under a lane condition, which the emulator refuses (the hardware reads any lane's register)
        for f in [x for x in recs if x.flag & 0x40][:2]:
            f.flag = (f.flag & 0x10) | 0x40
            f.mate_ref, f.mate_pos, f.tlen = -1, -1, 0
            f.tags = [t for t in f.tags if t[0] != b"MC"]
    elif kind == "secondary":
        r.flag |= 0x100
    elif kind == "rx":
        assert r.tag(b"RX") is not None
        _set_tag(r, b"RX", b"A" * int(arg))
    else:
        raise KeyError(edge)


def make_batch(head, edge):
    from fgumi_amd import GroupedReads, simulate_grouped_reads
    n, sim, _, n_edge = HEADS[head]
    g = simulate_grouped_reads(n, seed=42, **sim)
    groups = [[Rec(r) for r in g.records(i)] for i in range(g.n_grp)]
    for k, recs in enumerate(groups[-n_edge:]):
        if head == "indel":      # an insertion read (not the edge record): the whole family is the workgroup kernel's
            r = recs[2]
            a = r.l_seq // 2
            r.cigar = [(a << 4) | 0, (2 << 4) | 1, ((r.l_seq - a - 2) << 4) | 0]
        if edge != "plain":
            apply_edge(recs, edge)
    return GroupedReads.from_groups([[r.encode() for r in rs] for rs in groups])


def route(head, edge, mem):
    """One batch through both entries against the oracle; returns the route as a short string."""
    from fgumi_amd._lib import Options, lib
    LR._debug(lib)
    has_wide = hasattr(lib, "fgx_debug_last_wide_families")
    if has_wide:
        lib.fgx_debug_last_wide_families.restype = C.c_uint32
        lib.fgx_debug_last_wide_families.argtypes = [C.c_void_p]
    g = make_batch(head, edge)
    o = options()
    what = f"{head}/{edge}"
    try:
        want = LR._oracle(o, g, None)
    except RuntimeError:
        want = None
    got, err = LR._host_entry(lib, o, g, None)
    if want is None:
        assert got is None, f"{what}: the oracle refuses the batch, the host entry does not"
    else:
        assert got is not None, f"{what}: host entry: {err}"
        LR._same(f"{what} host entry", got, want, False)
    h = lib.fgx_create(C.byref(Options.from_buffer_copy(bytes(o))))
    assert h, lib.fgx_global_error().decode()
    try:
        rc, res, deferred = LR._device_entry(lib, h, g, mem)
        b = (C.c_uint64 * 4)()
        lib.fgx_debug_last_split_builds(h, b)
        ch = (C.c_uint32 * 2)()
        lib.fgx_debug_last_chain.restype = None
        lib.fgx_debug_last_chain.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        lib.fgx_debug_last_chain(h, ch)
        counts = dict(launches=int(ch[0]), routed=int(lib.fgx_debug_last_routed(h)), big=int(lib.fgx_debug_last_big_families(h)), deep=int(lib.fgx_debug_last_deep_families(h)),
                      wide=int(lib.fgx_debug_last_wide_families(h)) if has_wide else 0, builds=list(b)[:3], chunks=int(lib.fgx_debug_last_split_chunks(h)))
    finally:
        lib.fgx_destroy(h)
    if rc != 0:
        assert want is None, f"{what}: device entry refused ({res})"
        return "refused"
    d = set(deferred)
    assert d <= set(range(g.n_grp - HEADS[head][3], g.n_grp)), f"{what}: plain families deferred: {sorted(d)}"
    kept = [i for i in range(g.n_grp) if i not in d]
    if want is None:
        # the oracle refuses the batch: what the device decided may stand, the deferred rest must be refused by the host entry
        assert deferred and LR._host_entry(lib, o, LR._subset(g, deferred), None)[0] is None, f"{what}: the oracle refuses the batch, nothing of the product does"
        return "deferred, refused by the host entry"
    LR._same(f"{what} device entry", res, LR._oracle(o, LR._subset(g, kept), None) if d else want, False)
    stats = res["stats"].copy()
    if deferred:
        got_d, err = LR._host_entry(lib, o, LR._subset(g, deferred), None)
        assert got_d is not None, f"{what}: deferred groups: {err}"
        LR._same(f"{what} deferred groups", got_d, LR._oracle(o, LR._subset(g, deferred), None), False)
        stats += got_d["stats"]
    assert np.array_equal(stats, want["stats"]), (f"{what}: counters do not add up", stats.tolist(), want["stats"].tolist())
    return ("edge deferred" if d else "edge on the device") + " " + " ".join(f"{k}={v}" for k, v in counts.items())


def routes_of_head(head, mem="host"):
    return {e: route(head, e, mem) for e in ["plain"] + EDGES}


def record(head, path, mem="host"):
    """(maintenance) the routes of one head as JSON: how ROUTES was filled, from the commit before the rewrite."""
    with open(path, "w") as f:
        json.dump(routes_of_head(head, mem), f, indent=0)


def check(head, mem="host"):
    got = routes_of_head(head, mem)
    for e, r in got.items():
        print(f"ROUTE {head} {e!r}: {r}")
    table = ROUTES[head] if mem == "host" else {**ROUTES[head], **GPU_ROUTES.get(head, {})}      # (the gpu column is empty: every route is the emulator's)
    bad = {e: (r, table.get(e)) for e, r in got.items() if r != table.get(e)}
    assert not bad, f"{head}: routes changed (got, table): {bad}\nrule: " + "; ".join(sorted({RULES[e.partition(':')[0]] for e in bad if e != 'plain'}))
    assert set(table) == set(got)


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "record_rule_routes.json")) as _f:
    _T = json.load(_f)
ROUTES = _T["emulator"]        # head -> edge -> route, recorded under the wave emulator from the commit before the rewrite
GPU_ROUTES = _T["gpu"]         # head -> edge -> route where the MI355X's differs from the emulator's (the parent commit's library, same run), with the reason in "gpu_why"
