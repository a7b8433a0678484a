"""Indel reads (`I D N`) in the methylation-aware mode (EM-Seq / TAPs) of the duplex and the simplex caller, decided by the device pipeline through the canonical
second pass (FGX_METH_CANON=1): the batches, the crafted molecules and the runner that tests/test_wavemu_methylation_indels.py (CPU, wave emulator)
and tests/test_gpu_methylation_indels.py (GPU) share.

What is checked: with the switch on, a molecule that holds an indel read is rewritten into its canonical form (canon_core.h), which now carries every
record's reference runs, and k_family_wave<1, 1> (duplex) / k_deep_cols<1> (simplex) look a column's reference base up through the anchor's runs.  The batch must come back byte for byte
and counter for counter the oracle's; what is still deferred must be out of the canonical form's scope (the host hook says which molecules are), and
something must have been canonicalised.  Without the switch the first pass's deferrals stay deferred — the parent's behaviour, which the switch-on
assertions fail on."""
import ctypes as C
import os
import random

import numpy as np

import bamutil
import methclip_cases as mc
import methsim

F_PAIRED, F_REVERSE, F_MATE_REVERSE, F_FIRST, F_LAST = 0x1, 0x10, 0x20, 0x40, 0x80


def out_of_scope(o, groups, which):
    """The groups of `which` for which the canonical form's host hook returns out of scope."""
    from fgumi_amd import GroupedReads
    from fgumi_amd._lib import lib
    oos = set()
    for i in which:
        g = GroupedReads.from_groups([groups[i]])
        out = np.zeros(g.blob.size + 16, dtype=np.uint8)
        out_len = np.zeros(max(1, g.n_rec), dtype=np.uint32)
        delta = np.zeros(5, dtype=np.uint64)
        args = (C.addressof(o), g.blob.ctypes.data, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, out.ctypes.data, out_len.ctypes.data, delta.ctypes.data)
        rc = lib.fgx_canon_duplex_host(*args) if o.caller_kind == 1 else lib.fgx_canon_simplex_host(*args, None)
        if rc != 0:
            oos.add(i)
    return oos


def product(o, contigs, g, entry, on_gpu):
    """mc.product, plus fgx_debug_last_deferral: `first_deferred` (groups the first device pass deferred) and `canon` (of which the second pass decided)."""
    from fgumi_amd._lib import Options, Output, lib
    po = Options.from_buffer_copy(bytes(o))
    h = lib.fgx_create(C.byref(po))
    assert h, lib.fgx_global_error().decode()
    try:
        bufs = [C.create_string_buffer(bytes(s), max(1, len(s))) for s in contigs]
        ptrs = (C.c_void_p * len(bufs))(*[C.cast(b, C.c_void_p).value for b in bufs])
        lens = (C.c_uint64 * len(bufs))(*[len(s) for s in contigs])
        assert lib.fgx_set_reference(h, len(bufs), ptrs, lens) == 0, lib.fgx_last_error(h).decode()
        out = Output()
        deferred = None
        if entry == "host":
            rc = lib.fgx_process_batch(h, g.blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, g.grp_first.ctypes.data, g.n_grp, C.byref(out))
            assert rc == 0, lib.fgx_last_error(h).decode()
            data = C.string_at(out.data, out.data_len) if out.data_len else b""
        else:
            nd, dp = C.c_uint32(), C.c_void_p()
            if on_gpu:
                import torch
                from fgumi_amd._lib import hip_memcpy_d2h
                dg = g.to_device()
                torch.cuda.synchronize(dg.blob.device)
                rc = lib.fgx_process_batch_device(h, dg.blob.data_ptr(), dg.blob_len, dg.rec_off.data_ptr(), dg.rec_len.data_ptr(), dg.n_rec, dg.grp_first.data_ptr(), dg.n_grp,
                                                  C.byref(out), C.byref(nd), C.byref(dp))
                assert rc == 0, lib.fgx_last_error(h).decode()
                data = hip_memcpy_d2h(out.data, int(out.data_len)) if out.data_len else b""
                deferred = np.frombuffer(hip_memcpy_d2h(dp.value, 4 * nd.value), dtype=np.uint32).tolist() if nd.value else []
            else:
                blob = np.concatenate([g.blob, np.zeros(64, dtype=np.uint8)])
                rc = lib.fgx_process_batch_device(h, blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, g.grp_first.ctypes.data, g.n_grp,
                                                  C.byref(out), C.byref(nd), C.byref(dp))
                assert rc == 0, lib.fgx_last_error(h).decode()
                data = C.string_at(out.data, out.data_len) if out.data_len else b""
                deferred = list((C.c_uint32 * nd.value).from_address(dp.value)) if nd.value else []
        d2 = (C.c_uint64 * 2)()
        lib.fgx_debug_last_deferral(h, d2)
        return dict(data=data, count=int(out.count), stats=np.array(list(out.stats), dtype=np.uint64), deferred=deferred, first_deferred=int(d2[0]), canon=int(d2[1]))
    finally:
        lib.fgx_destroy(h)


def check_groups(o, contigs, groups, entry, on_gpu, switch=True, min_mm=20, max_oos_share=0.05):
    """`groups` through `entry` against the oracle.  Switch on: deferred within the form's out-of-scope set, something canonicalised, the oracle's bytes and
    counters (device entry: of the groups it did not defer).  Switch off: the indel groups stay deferred, nothing canonicalised."""
    from fgumi_amd import GroupedReads
    assert ("FGX_METH_CANON" in os.environ and os.environ["FGX_METH_CANON"][:1] not in ("", "0")) == switch      # (read per call by the library)
    indel = [i for i, grp in enumerate(groups) if any(mc.has_indel(r) for r in grp)]
    assert indel
    oos = out_of_scope(o, groups, indel)
    assert len(oos) <= max_oos_share * len(indel), (len(oos), len(indel))          # a condition on the INPUT: the seeds are picked so that it holds
    g = GroupedReads.from_groups(groups)
    got = product(o, contigs, g, entry, on_gpu)
    print(f"{entry} entry, switch {'on' if switch else 'off'}: {g.n_grp} groups, {len(indel)} with an indel read, {len(oos)} out of the form's scope; first pass deferred "
          f"{got['first_deferred']}, canonicalised {got['canon']}, left {len(got['deferred']) if got['deferred'] is not None else got['first_deferred'] - got['canon']}")
    left = got["first_deferred"] - got["canon"]
    if switch:
        assert got["canon"] > 0, got["canon"]
        assert left <= len(oos), (left, len(oos))
        if got["deferred"] is not None:
            assert set(got["deferred"]) <= oos, sorted(set(got["deferred"]) - oos)[:10]
    else:
        assert got["canon"] == 0 and 0 < got["first_deferred"] <= len(indel), (got["canon"], got["first_deferred"], len(indel))
        if got["deferred"] is not None:
            assert set(got["deferred"]) <= set(indel)
    kept = groups if got["deferred"] is None else [grp for i, grp in enumerate(groups) if i not in set(got["deferred"])]
    want = mc.oracle(o, contigs, GroupedReads.from_groups(kept))
    n_mm = sum("MM" in bamutil.parse(r)["tags"] for r in mc.split(want["data"]))
    assert n_mm > min_mm, n_mm
    assert got["count"] == want["count"]
    mc.assert_same_records(got["data"], want["data"])
    assert np.array_equal(got["stats"], want["stats"]), (got["stats"].tolist(), want["stats"].tolist())
    return got, want, oos


def GroupedReads_from(groups):
    from fgumi_amd import GroupedReads
    return GroupedReads.from_groups(groups)


def duplex_batch(n_groups, seed):
    rng = methsim.seeded(seed)
    contigs = methsim.genome(rng)
    return contigs, methsim.duplex_groups(rng, contigs, n_groups)


def shared_indel_batch(n_groups, seed):
    """tests/methsim.py's duplex molecules, but every indel read of a molecule carries the SAME deletion or insertion (methsim draws a place per read, so its
    `D` molecules keep one read per end after the alignment filter: under --min-reads above 1 they are rejected either way and the canonical form leaves them
    where they are).  A third of the molecules `D`, a sixth `I`, both on the forward reads of both strands; depth 2 .. 4 per strand."""
    rng = methsim.seeded(seed)
    contigs = methsim.genome(rng)
    groups = []
    for g in range(n_groups):
        ref_id = rng.randrange(len(contigs))
        ref = contigs[ref_id].decode().upper().replace("N", "A")
        L = rng.randint(30, 80)
        p1 = rng.randint(0, len(ref) - 2 * L - 150)
        p2 = p1 + L + rng.randint(-L // 3, 100)
        conv = rng.choice([0.0, 0.5, 1.0])
        kind = rng.choice("MMMDDI")
        a, d = rng.randint(5, L - 8), rng.randint(1, 3)
        ins = "".join(rng.choice("ACGT") for _ in range(d))
        if kind == "D":
            fwd_ref, fwd_cigar = ref[p1:p1 + a] + ref[p1 + a + d:p1 + L + d], f"{a}M{d}D{L - a}M"
        elif kind == "I":
            fwd_ref, fwd_cigar = ref[p1:p1 + a] + ins + ref[p1 + a:p1 + L - d], f"{a}M{d}I{L - a - d}M"
        else:
            fwd_ref, fwd_cigar = ref[p1:p1 + L], f"{L}M"
        rev_ref, rev_cigar = ref[p2:p2 + L], f"{L}M"

        def read(s, top_like):
            s = methsim._convert(rng, s, "C", "T", conv) if top_like else methsim._convert(rng, s, "G", "A", conv)
            return methsim._errors(rng, s, 0.005)
        reads = []
        for i in range(rng.randint(2, 4)):
            reads += [mc._duplex_rec(rng, f"a{g}_{i}", read(fwd_ref, True), fwd_cigar, F_PAIRED | F_FIRST | F_MATE_REVERSE, ref_id, p1, p2, f"{g}/A", rev_cigar),
                      mc._duplex_rec(rng, f"a{g}_{i}", read(rev_ref, True), rev_cigar, F_PAIRED | F_LAST | F_REVERSE, ref_id, p2, p1, f"{g}/A", fwd_cigar)]
        for i in range(rng.randint(2, 4)):
            reads += [mc._duplex_rec(rng, f"b{g}_{i}", read(rev_ref, False), rev_cigar, F_PAIRED | F_FIRST | F_REVERSE, ref_id, p2, p1, f"{g}/B", fwd_cigar),
                      mc._duplex_rec(rng, f"b{g}_{i}", read(fwd_ref, False), fwd_cigar, F_PAIRED | F_LAST | F_MATE_REVERSE, ref_id, p1, p2, f"{g}/B", rev_cigar)]
        groups.append(reads)
    return contigs, groups


def simplex_batch(n_groups, seed, in_header=False):
    rng = methsim.seeded(seed)
    contigs = methsim.genome(rng)
    groups = methsim.simplex_groups(rng, contigs, n_groups)
    if in_header:          # (a BAM file names header contigs only)
        groups = [g for g in groups if bamutil.parse(g[0])["ref_id"] < len(contigs)]
    return contigs, groups


def check_simplex_batch(mode, n_groups, seed, entry, on_gpu, switch=True, kw=None):
    contigs, groups = simplex_batch(n_groups, seed)
    return check_groups(mc.options(0, mode, 1, **(kw or {})), contigs, groups, entry, on_gpu, switch)


def deep_indel_families(seed, n_fam=12, depth=(100, 120)):
    """Fragment families of 100 .. 120 records, a third of the reads with one of three deletions of the family (minority alignments — at most 16 alignment groups
    are in the form's scope —: the filter drops them, and the canonical family keeps more than 64 records — the <256, DEEP_MAX, 1> build of the record kernel,
    with runs).  At most 128 records: in the form's scope."""
    rng = methsim.seeded(seed)
    contigs = methsim.genome(rng)
    groups = []
    for g in range(n_fam):
        contig = contigs[g % len(contigs)]
        L, pos, rev = rng.randint(60, 110), rng.randint(0, len(contig) - 300), g % 2 == 1
        conv = rng.choice([0.3, 0.9])
        ref = contig.decode().upper().replace("N", "A")
        dels = [(rng.randint(5, L - 5), rng.randint(1, 4)) for _ in range(3)]
        reads = []
        for i in range(rng.randint(*depth)):
            if i % 3 == 1:
                a, d = dels[(i // 3) % 3]
                seq, cigar = ref[pos:pos + a] + ref[pos + a + d:pos + L + d], f"{a}M{d}D{L - a}M"
            else:
                seq, cigar = ref[pos:pos + L], f"{L}M"
            seq = methsim._errors(rng, methsim._convert(rng, seq, "C", "T", conv) if not rev else methsim._convert(rng, seq, "G", "A", conv), 0.01)
            reads.append(bamutil.make_record(f"d{g:03d}_{i:04d}", seq, [rng.choice([20, 30, 37]) for _ in seq], flag=F_REVERSE if rev else 0, ref_id=g % len(contigs), pos=pos, cigar=cigar,
                                             tags=[("MI", "Z", f"{g}"), ("RX", "Z", "ACGT")]))
        groups.append(reads)
    return contigs, groups


def canonical_sizes(o, groups):
    """Records the canonical form keeps of each (simplex) family, by the host hook; None: out of scope."""
    from fgumi_amd import GroupedReads
    from fgumi_amd._lib import lib
    out = []
    for grp in groups:
        g = GroupedReads.from_groups([grp])
        buf = np.zeros(g.blob.size + 16, dtype=np.uint8)
        out_len = np.zeros(max(1, g.n_rec), dtype=np.uint32)
        delta = np.zeros(5, dtype=np.uint64)
        rc = lib.fgx_canon_simplex_host(C.addressof(o), g.blob.ctypes.data, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, buf.ctypes.data, out_len.ctypes.data, delta.ctypes.data, None)
        out.append(int((out_len[:g.n_rec] != 0).sum()) if rc == 0 else None)
    return out


def check_duplex_batch(mode, min_reads, n_groups, seed, entry, on_gpu, switch=True, shared=False):
    contigs, groups = shared_indel_batch(n_groups, seed) if shared else duplex_batch(n_groups, seed)
    return check_groups(mc.options(1, mode, min_reads), contigs, groups, entry, on_gpu, switch)


# ---- crafted molecules on methclip_cases.craft_genome(): C at every multiple of 7, G at every other multiple of 11, A elsewhere --------------------------
def _strand_a(rng, mi, n, r1, r2, ref_id=0, tag=""):
    """n A-strand pairs: R1 forward = r1 (seq, cigar, pos), R2 reverse = r2; every MC the mate's CIGAR."""
    out = []
    for i in range(n):
        out += [mc._duplex_rec(rng, f"a{mi}{tag}_{i}", r1[0], r1[1], F_PAIRED | F_FIRST | F_MATE_REVERSE, ref_id, r1[2], r2[2], f"{mi}/A", r2[1]),
                mc._duplex_rec(rng, f"a{mi}{tag}_{i}", r2[0], r2[1], F_PAIRED | F_LAST | F_REVERSE, ref_id, r2[2], r1[2], f"{mi}/A", r1[1])]
    return out


def _strand_b(rng, mi, n, r1, r2, ref_id=0, tag=""):
    """n B-strand pairs: R1 reverse = r1, R2 forward = r2."""
    out = []
    for i in range(n):
        out += [mc._duplex_rec(rng, f"b{mi}{tag}_{i}", r1[0], r1[1], F_PAIRED | F_FIRST | F_REVERSE, ref_id, r1[2], r2[2], f"{mi}/B", r2[1]),
                mc._duplex_rec(rng, f"b{mi}{tag}_{i}", r2[0], r2[1], F_PAIRED | F_LAST | F_MATE_REVERSE, ref_id, r2[2], r1[2], f"{mi}/B", r1[1])]
    return out


FWD_DEL_POS, FWD_DEL_N = 49, 2       # `10M2D10M`, bases C x 10 + T x 10: columns 0 .. 9 at 49 .. 58, columns 10 .. 19 at 61 .. 70; C at 49 56 63 70
INS_POS, INS_N = 49, 3               # `6M3I11M`, bases C x 20: columns 0 .. 5 at 49 .. 54, 6 .. 8 inserted, 9 .. 19 at 55 .. 65; a one-block rule puts column 7 at 56 = C


# Hand-written expectations of the crafted families whose reads are ONE base throughout, so that a count depends on the column's place alone: a read base counts
# as unconverted where the reference shows the strand's cytosine (C on the top strand, G on the bottom one) and the ORIENTED read base is that letter (a reverse
# read's stored bases are complemented: stored G reads as C, stored C as G).  Per family: which record carries the tags under test, the reads counted, the
# strand's letter, the reference position of every column of the anchor — written out by hand from the CIGAR, the position and the strand — and the columns at
# which the genome (C at multiples of 7, G at the other multiples of 11) then shows that letter, by hand as well.
def _walk(*pieces):
    out = []
    for a, b in pieces:            # (a, b): reference positions a .. b inclusive, downwards when a > b; (None, k): k inserted columns
        out += [None] * b if a is None else list(range(a, b + 1)) if a <= b else list(range(a, b - 1, -1))
    return out


HAND = {
    # reverse R2 `20M3D20M` at 100, stored G (oriented C, top strand); its mate starts at 110, so the mate clip cuts the 10 bases at 100 .. 109 off its stored
    # head; reverse start = pos + span - 1 = 100 + 43 - 1 = 142, the deletion 120 .. 122 is jumped
    "rev_anchor_deletion_mate_clip": dict(end="R2", n=2, letter="C", ref=_walk((142, 123), (119, 110)), hits=[2, 9, 16, 20, 27]),          # C at 140 133 126 | 119 112
    # forward `10M2D20M` at 60 and at 63, both 30 long: the LAST one anchors (63 .. 72, 75 .. 94); both reads are counted
    "last_longest_is_the_anchor": dict(end="R1", n=2, letter="C", ref=_walk((63, 72), (75, 94)), hits=[0, 7, 12, 19, 26]),                # C at 63 70 | 77 84 91
    # `20M1D15M` at 60 (35 long, the longest) is a minority alignment and dropped; the anchor is the last `30M` at 61, three reads are counted
    "minority_indel_read_dropped": dict(end="R1", n=3, letter="C", ref=_walk((61, 90)), hits=[2, 9, 16, 23]),                             # C at 63 70 77 84
    # reverse R2 `15M2D15M` at 130, stored G: start 130 + 32 - 1 = 161; its canonical record sits on another reference id
    "r2_anchor_with_an_indel": dict(end="R2", n=2, letter="C", ref=_walk((161, 147), (144, 130)), hits=[0, 7, 14, 19, 26]),                # C at 161 154 147 | 140 133
}
HAND_DUPLEX = dict(HAND)
# reverse R2 `10M5D22M` at 280, stored G: start 280 + 37 - 1 = 316, the contig ends at 299 — columns 0 .. 16 lie outside it
HAND_DUPLEX["run_crossing_the_contig_end"] = dict(end="R2", n=2, letter="C", ref=_walk((316, 295), (289, 280)), hits=[24, 31])                # C at 287 280
HAND_SIMPLEX = dict(HAND)
# reverse FRAGMENTS (bottom strand: G), stored C (oriented G): the same walk; G at 297 and 286
HAND_SIMPLEX["run_crossing_the_contig_end"] = dict(end="R1", n=2, letter="G", ref=_walk((316, 295), (289, 280)), hits=[19, 25])
# reverse fragments `15M2I13M` at 150, stored C: start 150 + 28 - 1 = 177; the inserted columns 13, 14 have no reference base
HAND_SIMPLEX["rev_fragments_with_an_insertion"] = dict(end="R1", n=3, letter="G", ref=_walk((177, 165), (None, 2), (164, 150)), hits=[1, 12])   # G at 176 165 (154 is a C)


def check_hand(name, h, rec):
    """cu / ct / MM / ML of `rec` against the hand-written expectation `h`."""
    g = mc.craft_genome()[0].decode()
    ncol = len(h["ref"])
    at_letter = [p for p, r in enumerate(h["ref"]) if r is not None and 0 <= r < len(g) and g[r] == h["letter"]]
    assert at_letter == h["hits"], (name, at_letter, h["hits"])                              # the two hand-written halves agree
    cu = [h["n"] if p in h["hits"] else 0 for p in range(ncol)]
    t = rec["tags"]
    assert len(rec["seq"]) == ncol and set(rec["seq"]) == {h["letter"]}, (name, rec["seq"])  # every consensus base is the strand's letter
    assert t["cu"][1] == cu and t["ct"][1] == [0] * ncol, (name, t["cu"][1], cu, t["ct"][1])
    skips = [b - a - 1 for a, b in zip([-1] + h["hits"][:-1], h["hits"])]                    # every column holds the tracked letter: the skips are the gaps
    mm = ("C+m" if h["letter"] == "C" else "G-m") + "".join(f",{k}" for k in skips) + ";"
    assert t["MM"][1] == mm and t["ML"][1] == [255] * len(h["hits"]), (name, t["MM"][1], mm, t["ML"][1])   # EM-Seq: unconverted / total


def _by_name(names, data):
    """{family name: {"R1" | "R2": record}} (a fragment's record under "R1")"""
    out = {n: {} for n in names}
    for r in (bamutil.parse(x) for x in mc.split(data)):
        out[names[int(r["tags"]["MI"][1])]]["R2" if r["flag"] & F_LAST else "R1"] = r
    return out


def _pairs(mi, n, r1, r2, q1=30, q2=30, ref_id=0, tag="", duplex=False):
    """n FR pairs: R1 forward = r1 (seq, cigar, pos), R2 reverse = r2, fixed qualities (the overlap pre-correction then has one outcome), MC = the mate's CIGAR."""
    out = []
    for i in range(n):
        tags = [("MI", "Z", f"{mi}/A" if duplex else mi), ("RX", "Z", "ACG-TTA")]
        out += [bamutil.make_record(f"a{mi}{tag}_{i}", r1[0], [q1] * len(r1[0]), flag=F_PAIRED | F_FIRST | F_MATE_REVERSE, ref_id=ref_id, pos=r1[2], mapq=60, cigar=r1[1], mate_ref=ref_id,
                                    mate_pos=r2[2], tags=tags + [("MC", "Z", r2[1])]),
                bamutil.make_record(f"a{mi}{tag}_{i}", r2[0], [q2] * len(r2[0]), flag=F_PAIRED | F_LAST | F_REVERSE, ref_id=ref_id, pos=r2[2], mapq=60, cigar=r2[1], mate_ref=ref_id,
                                    mate_pos=r1[2], tags=tags + [("MC", "Z", r1[1])])]
    return out


def _pair_families(g, duplex):
    """The crafted families that are pairs in both callers' sets (a duplex molecule of /A pairs alone): name -> records."""
    far = (g[200:230], "30M", 200)                       # the plain mate, far enough away: no overlap, no mate clip
    near = (g[20:50], "30M", 20)
    kw = dict(duplex=duplex)
    return {
        # the mates overlap: where they disagree the pre-correction keeps the base of the better quality — the reverse read's (35 against 12)
        "rev_anchor_deletion_mate_clip": _pairs("1", 2, (g[110:150], "40M", 110), ("G" * 40, "20M3D20M", 100), q1=12, q2=35, **kw),
        "r2_anchor_with_an_indel": _pairs("5", 2, near, ("G" * 30, "15M2D15M", 130), **kw),
    }


def crafted_duplex():
    """-> (contigs, molecules, names); molecule i carries MI i"""
    rng = random.Random(19)
    c = mc.craft_genome()
    g = c[0].decode()
    far = (g[200:230], "30M", 200)
    pf = _pair_families(g, True)
    fams = []
    fams.append(("fwd_anchor_10M2D10M", _strand_a(rng, "0", FWD_DEL_N, ("C" * 10 + "T" * 10, "10M2D10M", FWD_DEL_POS), far)))
    fams.append(("rev_anchor_deletion_mate_clip", pf["rev_anchor_deletion_mate_clip"]))
    fams.append(("insertion_over_a_cytosine", _strand_a(rng, "2", INS_N, ("C" * 20, "6M3I11M", INS_POS), far)))
    fams.append(("last_longest_is_the_anchor", _pairs("3", 1, ("C" * 30, "10M2D20M", 60), far, duplex=True) + _pairs("3", 1, ("C" * 30, "10M2D20M", 63), far, tag="x", duplex=True)))
    fams.append(("minority_indel_read_dropped", _pairs("4", 1, ("C" * 35, "20M1D15M", 60), far, tag="m", duplex=True) + _pairs("4", 3, ("C" * 30, "30M", 61), far, duplex=True)))
    fams.append(("r2_anchor_with_an_indel", pf["r2_anchor_with_an_indel"]))
    fams.append(("both_strands_indels", _strand_a(rng, "6", 2, (g[30:45] + g[46:61], "15M1D15M", 30), (g[150:165] + "AC" + g[165:178], "15M2I13M", 150)) +
                 _strand_b(rng, "6", 2, (g[150:165] + "AC" + g[165:178], "15M2I13M", 150), (g[30:45] + g[46:61], "15M1D15M", 30))))
    fams.append(("contig_outside_the_genome", _strand_a(rng, "7", 2, (g[60:70] + g[72:92], "10M2D20M", 60), far, ref_id=5)))
    fams.append(("run_crossing_the_contig_end", _pairs("8", 2, (g[100:130], "30M", 100), ("G" * 32, "10M5D22M", mc.CRAFT_LEN - 20), duplex=True)))
    return c, [f for _, f in fams], [n for n, _ in fams]


def expected_fwd_del():
    g = mc.craft_genome()[0].decode()
    ref = [FWD_DEL_POS + p for p in range(10)] + [FWD_DEL_POS + 12 + p for p in range(10)]
    cu = [FWD_DEL_N if (p < 10 and g[ref[p]] == "C") else 0 for p in range(20)]
    ct = [FWD_DEL_N if (p >= 10 and g[ref[p]] == "C") else 0 for p in range(20)]
    return cu, ct


def expected_ins():
    g = mc.craft_genome()[0].decode()
    ref = [INS_POS + p for p in range(6)] + [None] * 3 + [INS_POS + 6 + p for p in range(11)]
    cu = [INS_N if (r is not None and g[r] == "C") else 0 for r in ref]
    return cu, [0] * 20


def _check_first_two_and_no_contig(recs):
    """The three families of both sets whose reads are not one base throughout: forward `10M2D10M` (C x 10 + T x 10), the insertion, the contig outside the genome."""
    r = recs["fwd_anchor_10M2D10M"]["R1"]["tags"]
    cu, ct = expected_fwd_del()
    assert cu == [2, 0, 0, 0, 0, 0, 0, 2] + [0] * 12 and ct == [0] * 12 + [2, 0, 0, 0, 0, 0, 0, 2], (cu, ct)        # C at 49 56 | 63 70
    assert r["cu"][1] == cu and r["ct"][1] == ct, ("fwd_anchor_10M2D10M", r["cu"], r["ct"])
    # consensus bases: C at columns 0 .. 9, and at 12 and 19 (converted T, normalised); entries at 0, 7 (6 C skipped), 12 (2 skipped), 19; EM-Seq: unconverted / total
    assert r["MM"][1] == "C+m,0,6,2,0;" and r["ML"][1] == [255, 255, 0, 0], ("fwd_anchor_10M2D10M", r["MM"], r["ML"])
    r = recs["insertion_over_a_cytosine"]["R1"]["tags"]
    cu, ct = expected_ins()
    assert cu == [3] + [0] * 9 + [3] + [0] * 6 + [3, 0, 0] and not any(ct), (cu, ct)         # C at 49 | 56 63; nothing under the inserted columns 6 .. 8
    assert r["cu"][1] == cu and r["ct"][1] == ct, ("insertion_over_a_cytosine", r["cu"], r["ct"])
    assert r["MM"][1] == "C+m,0,9,6;", ("insertion_over_a_cytosine", r["MM"])                # 20 consensus C: entries at columns 0, 10 (9 skipped) and 17 (6 skipped)
    for rec in recs["contig_outside_the_genome"].values():                                   # no contig, no annotation
        assert "MM" not in rec["tags"] and "cu" not in rec["tags"], ("contig_outside_the_genome", rec["tags"].keys())


def check_crafted(entry, on_gpu):
    contigs, groups, names = crafted_duplex()
    assert all(any(mc.has_indel(r) for r in grp) for grp in groups)
    o = mc.options(1, 1)
    got, want, oos = check_groups(o, contigs, groups, entry, on_gpu, min_mm=4, max_oos_share=0.0)
    assert got["canon"] == len(groups), (got["canon"], len(groups))
    recs = _by_name(names, got["data"])
    _check_first_two_and_no_contig(recs)
    for name, h in HAND_DUPLEX.items():
        check_hand(name, h, recs[name][h["end"]])


# ---- crafted simplex families on the same genome ------------------------------------------------------------------------------------------------------------
def crafted_simplex():
    """-> (contigs, families, names); family i carries MI i"""
    c = mc.craft_genome()
    g = c[0].decode()
    L = mc.CRAFT_LEN
    pf = _pair_families(g, False)
    fams = []
    fams.append(("fwd_anchor_10M2D10M", mc._frags("0", FWD_DEL_N, "C" * 10 + "T" * 10, "10M2D10M", FWD_DEL_POS)))
    fams.append(("rev_anchor_deletion_mate_clip", pf["rev_anchor_deletion_mate_clip"]))
    fams.append(("insertion_over_a_cytosine", mc._frags("2", INS_N, "C" * 20, "6M3I11M", INS_POS)))
    fams.append(("last_longest_is_the_anchor", mc._frags("3", 1, "C" * 30, "10M2D20M", 60) + mc._frags("3", 1, "C" * 30, "10M2D20M", 63, tag="x")))
    fams.append(("minority_indel_read_dropped", mc._frags("4", 1, "C" * 35, "20M1D15M", 60, tag="m") + mc._frags("4", 3, "C" * 30, "30M", 61)))
    fams.append(("r2_anchor_with_an_indel", pf["r2_anchor_with_an_indel"]))
    fams.append(("rev_fragments_with_an_insertion", mc._frags("6", 3, "C" * 30, "15M2I13M", 150, flag=F_REVERSE)))
    fams.append(("contig_outside_the_genome", [bamutil.make_record(f"f7_{i}", g[60:70] + g[72:92], [30] * 30, flag=0, ref_id=5, pos=60, cigar="10M2D20M", tags=[("MI", "Z", "7"), ("RX", "Z", "ACGT")])
                                               for i in range(2)]))
    fams.append(("run_crossing_the_contig_end", mc._frags("8", 2, "C" * 32, "10M5D22M", L - 20, flag=F_REVERSE)))
    return c, [f for _, f in fams], [n for n, _ in fams]


def check_crafted_simplex(entry, on_gpu):
    contigs, groups, names = crafted_simplex()
    assert all(any(mc.has_indel(r) for r in grp) for grp in groups)
    got, want, oos = check_groups(mc.options(0, 1), contigs, groups, entry, on_gpu, min_mm=4, max_oos_share=0.0)
    assert got["canon"] == len(groups), (got["canon"], len(groups))
    recs = _by_name(names, got["data"])
    _check_first_two_and_no_contig(recs)
    for name, h in HAND_SIMPLEX.items():
        check_hand(name, h, recs[name][h["end"]])
