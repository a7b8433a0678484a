"""Soft- / hard-clipped reads in the methylation-aware mode (EM-Seq / TAPs): the batches, the crafted families and the runner that
tests/test_wavemu_methylation_clips.py (CPU, wave emulator) and tests/test_gpu_methylation_clips.py (GPU) share.

What is checked: a read of the shape H* S* (M|=|X)+ S* H* is, to the reference, ONE M op of T = the lengths of all its ops
(simplify_cigar_from_raw), every query base kept; the call's anchor (the LAST longest source read) puts column p at pos + p (forward)
or at pos + T - 1 - p (reverse).  The device kernels restate that (k_deep_parse<.., .., 1>, k_family_wave<1, 1>), so a batch whose
multi-op records are all of that shape must come back from the device pipeline with nothing deferred, byte for byte and counter for
counter the oracle's, and fgx_debug_last_meth_clipped must count the groups that hold such a record."""
import ctypes as C
import struct

import numpy as np

import bamutil
import fgx_opts
import methsim
import orc

F_PAIRED, F_REVERSE, F_MATE_REVERSE, F_FIRST, F_LAST = 0x1, 0x10, 0x20, 0x40, 0x80


# ---- a small CIGAR reader (bamutil.parse gives the op count only) ------------------------------------------------------------------------
def cigar_of(rec):
    l_name = rec[8]
    n_cig, = struct.unpack_from("<H", rec, 12)
    return [("MIDNSHP=X"[o & 15], o >> 4) for o in struct.unpack_from(f"<{n_cig}I", rec, 32 + l_name)]


def multi_op(rec):
    return len(cigar_of(rec)) > 1


def has_indel(rec):
    return any(k in "IDNP" for k, _ in cigar_of(rec))


def n_clipped_groups(groups):
    """Groups that hold a record of more than one CIGAR op (here: clips around one aligned block)."""
    return sum(any(multi_op(r) for r in g) for g in groups)


# ---- generators: kinds drawn from M and S only, one kind per group, half the groups S ----------------------------------------------------
def simplex_ms_groups(rng, contigs, n_groups, depth=(1, 7), read_len=(26, 90), per_read_clip=None, layouts=("frag", "frag_rev", "pair", "pair_overlap"), long_names=False):
    """tests/methsim.py's simplex layouts (fragments of both orientations, pairs, overlapping pairs) with `M` and `S` reads only: group g is
    an `S` group (every read soft-clipped at both ends, BOTH mates of a pair) when g is odd.  `per_read_clip`: instead, each read is
    clipped with that probability (deep families).  Reads are at least 24 long, so an `S` read is always clipped (methsim._read_from).
    `long_names`: ten-character read names, the running number in the last four — the record kernel's 30-bit pairing hash folds short names that
    differ in two places onto each other (`p0_19` / `p0_21`) and then leaves the family to the general path, which a deep family of such names meets."""
    groups = []
    for g in range(n_groups):
        ref_id = rng.randrange(len(contigs) + (1 if rng.random() < 0.03 else 0))      # now and then a contig outside the header
        contig = contigs[min(ref_id, len(contigs) - 1)]
        L = rng.randint(*read_len)
        pos = rng.randint(0, len(contig) - 10) if rng.random() < 0.9 else len(contig) - rng.randint(1, L)   # may run off the end
        gkind = "S" if g % 2 else "M"
        n = rng.randint(*depth)
        conv = rng.choice([0.0, 0.3, 0.9, 1.0])
        layout = rng.choice(list(layouts))
        reads = []
        for i in range(n):
            def kind():
                return gkind if per_read_clip is None else ("S" if rng.random() < per_read_clip else "M")
            l_i = L if rng.random() < 0.7 else rng.randint(max(24, L - 15), L)
            if layout in ("frag", "frag_rev"):
                seq, cigar = methsim._read_from(rng, contig, pos, l_i, kind(), layout == "frag", conv, 0.01)
                q = [rng.choice([8, 20, 30, 37]) for _ in seq]
                reads.append(bamutil.make_record(f"f{g:04d}_{i:04d}" if long_names else f"f{g}_{i}", seq, q, flag=F_REVERSE if layout == "frag_rev" else 0, ref_id=ref_id, pos=pos, cigar=cigar,
                                                 tags=[("MI", "Z", f"{g}"), ("RX", "Z", "ACGT")]))
            else:
                gap = rng.randint(-l_i // 2, 60) if layout == "pair_overlap" else rng.randint(20, 120)
                pos2 = max(0, pos + gap) if layout == "pair_overlap" else pos + l_i + gap
                s1, c1 = methsim._read_from(rng, contig, pos, l_i, kind(), True, conv, 0.01)
                s2, c2 = methsim._read_from(rng, contig, pos2, l_i, kind(), True, conv, 0.01)
                r1, r2 = bamutil.pair(f"p{g:04d}_{i:04d}" if long_names else f"p{g}_{i}", s1, [rng.choice([20, 30, 37]) for _ in s1], s2, [rng.choice([20, 30, 37]) for _ in s2], f"{g}",
                                      pos1=pos, pos2=pos2, cigar1=c1, cigar2=c2, rx="AAC-GGT", ref_id=ref_id)   # (MC = the mate's real CIGAR)
                reads += [r1, r2]
        groups.append(reads)
    return groups


def _duplex_rec(rng, name, seq, cigar, flag, ref_id, pos, mpos, mi, mc):
    return bamutil.make_record(name, seq, [rng.choice([25, 30, 37]) for _ in seq], flag=flag, ref_id=ref_id, pos=pos, mapq=60, cigar=cigar, mate_ref=ref_id,
                               mate_pos=mpos, tags=[("MI", "Z", mi), ("RX", "Z", "ACG-TTA" if mi.endswith("A") else "TTA-ACG"), ("MC", "Z", mc)])


def duplex_ms_groups(rng, contigs, n_groups, depth=(0, 4), read_len=(25, 80)):
    """tests/methsim.py's duplex molecules with `M` and `S` reads only; in an `S` molecule (odd g) the reverse-strand reads are clipped
    as well as the forward ones, and every record's MC is its mate's real CIGAR."""
    groups = []
    for g in range(n_groups):
        ref_id = rng.randrange(len(contigs))
        contig = contigs[ref_id]
        L = rng.randint(*read_len)
        p1 = rng.randint(0, len(contig) - 2 * L - 150)
        p2 = p1 + L + rng.randint(-L // 3, 100)
        conv = rng.choice([0.0, 0.5, 1.0])
        na, nb = rng.randint(*depth), rng.randint(*depth)
        if na + nb == 0:
            na = 1
        kind = "S" if g % 2 else "M"
        reads = []
        for i in range(na):   # A strand: R1 forward at p1 (top), R2 reverse at p2 (top): C→T
            s1, c1 = methsim._read_from(rng, contig, p1, L, kind, True, conv, 0.005)
            s2, c2 = methsim._read_from(rng, contig, p2, L, kind, True, conv, 0.005)
            reads += [_duplex_rec(rng, f"a{g}_{i}", s1, c1, F_PAIRED | F_FIRST | F_MATE_REVERSE, ref_id, p1, p2, f"{g}/A", c2),
                      _duplex_rec(rng, f"a{g}_{i}", s2, c2, F_PAIRED | F_LAST | F_REVERSE, ref_id, p2, p1, f"{g}/A", c1)]
        for i in range(nb):   # B strand: R1 reverse at p2 (bottom), R2 forward at p1 (bottom): G→A
            s1, c1 = methsim._read_from(rng, contig, p2, L, kind, False, conv, 0.005)
            s2, c2 = methsim._read_from(rng, contig, p1, L, kind, False, conv, 0.005)
            reads += [_duplex_rec(rng, f"b{g}_{i}", s1, c1, F_PAIRED | F_FIRST | F_REVERSE, ref_id, p2, p1, f"{g}/B", c2),
                      _duplex_rec(rng, f"b{g}_{i}", s2, c2, F_PAIRED | F_LAST | F_MATE_REVERSE, ref_id, p1, p2, f"{g}/B", c1)]
        groups.append(reads)
    return groups


def ms_batch(kind, n_groups, seed):
    rng = methsim.seeded(seed)
    contigs = methsim.genome(rng)
    groups = (duplex_ms_groups if kind == 1 else simplex_ms_groups)(rng, contigs, n_groups)
    n_clip = n_clipped_groups(groups)
    assert n_clip > n_groups // 3, (n_clip, n_groups)                  # by construction: every odd group
    assert not any(has_indel(r) for g in groups for r in g)
    return contigs, groups, n_clip


# ---- crafted families on a small genome with cytosines at known places -----------------------------------------------------------------
CRAFT_LEN = 300


def craft_genome():
    """One contig: C at every multiple of 7, G at every other multiple of 11, A elsewhere (neither period divides the shifts a wrong
    rule would make: a lookup off by the hard clips, or by the leading clip, hits other columns)."""
    s = ["A"] * CRAFT_LEN
    for i in range(0, CRAFT_LEN, 11):
        s[i] = "G"
    for i in range(0, CRAFT_LEN, 7):
        s[i] = "C"
    return ["".join(s).encode()]


FWD_POS, FWD_SEQ, FWD_N = 50, "C" * 20 + "T" * 20, 3          # `4S36M`, forward fragments: top strand, C unconverted / T converted
REV_POS, REV_SEQ, REV_N = 100, "C" * 20 + "T" * 17, 3         # `3H2S30M5S1H`, reverse fragments: l_seq 37, T 41; bottom strand — in consensus
                                                              # orientation the read is A x 17 + G x 20: G unconverted / A converted


def _frags(mi, n, seq, cigar, pos, flag=0, quals=30, tag=""):
    return [bamutil.make_record(f"f{mi}{tag}_{i}", seq, [quals] * len(seq), flag=flag, ref_id=0, pos=pos, cigar=cigar,
                                tags=[("MI", "Z", mi), ("RX", "Z", "ACGT")]) for i in range(n)]


def crafted_simplex():
    """-> (contigs, groups, names of the groups in order)"""
    c = craft_genome()
    g = c[0].decode()
    fams = []
    fams.append(("fwd_4S36M", _frags("0", FWD_N, FWD_SEQ, "4S36M", FWD_POS)))
    fams.append(("rev_3H2S30M5S1H", _frags("1", REV_N, REV_SEQ, "3H2S30M5S1H", REV_POS, flag=F_REVERSE)))
    ref40 = g[70:110]
    # the LAST longest read is the only clipped one / the only plain one (forward and reverse)
    fams.append(("last_longest_clipped", _frags("2", 2, ref40, "40M", 70) + _frags("2", 1, ref40, "3S37M", 70, tag="c")))
    fams.append(("last_longest_plain", _frags("3", 2, ref40, "3S37M", 70, tag="c") + _frags("3", 1, ref40, "40M", 70)))
    fams.append(("rev_last_longest_clipped", _frags("4", 2, ref40, "40M", 70, flag=F_REVERSE) + _frags("4", 1, ref40, "2H33M7S", 70, flag=F_REVERSE, tag="c")))
    fams.append(("rev_last_longest_plain", _frags("5", 2, ref40, "2H33M7S", 70, flag=F_REVERSE, tag="c") + _frags("5", 1, ref40, "40M", 70, flag=F_REVERSE)))
    # lookups at the ends of the contig.  Only the far end can be overrun: forward pos + p and reverse pos + T - 1 - p with p < l_seq <= T never fall below 0,
    # so the *_at_0 families are the in-range start (a leading clip at position 0), the *_off_the_end ones the out-of-contig case
    fams.append(("fwd_at_0", _frags("6", 2, FWD_SEQ, "4S36M", 0)))
    fams.append(("fwd_off_the_end", _frags("7", 2, FWD_SEQ, "4S36M", CRAFT_LEN - 10)))
    fams.append(("rev_off_the_end", _frags("8", 2, REV_SEQ, "3H2S30M5S1H", CRAFT_LEN - 20, flag=F_REVERSE)))
    fams.append(("rev_at_0", _frags("9", 2, REV_SEQ, "3H2S30M5S1H", 0, flag=F_REVERSE)))
    # a pair whose mates are both clipped and overlap; MC carries S ops
    pr = []
    for i in range(3):
        pr += list(bamutil.pair(f"p10_{i}", "ACG" + g[60:97], 30, g[70:105] + "TTGCA", 30 - i, "10", pos1=60, pos2=70, cigar1="3S37M", cigar2="35M5S", rx="AAC-GGT"))
    fams.append(("pair_both_clipped_overlap", pr))
    # depth 1
    fams.append(("depth_1", _frags("11", 1, FWD_SEQ, "6S30M4S", 140)))
    # a clip-only CIGAR of 7 ops through = / X (the wavefront kernels read 6; the streaming record kernel 16)
    fams.append(("seven_ops", _frags("12", 2, "TT" + g[150:181] + "CCA", "1H2S10=1X20=3S1H", 150)))
    pr = []
    for i in range(2):
        pr += list(bamutil.pair(f"p13_{i}", "TT" + g[150:181] + "CCA", 30, g[160:190] + "CA", 25, "13", pos1=150, pos2=160, cigar1="1H2S10=1X20=3S1H", cigar2="30M2S", rx="AAC-GGT"))
    fams.append(("seven_ops_pair", pr))
    # members ahead of an anchor that is shorter in query bases but spans more with its hard clips: the anchor is chosen by final length, not by T
    fams.append(("mixed_lengths", _frags("14", 1, g[200:236], "36M", 200, flag=F_REVERSE) + _frags("14", 2, g[200:234], "5H30M4S", 200, flag=F_REVERSE, tag="c")))
    return c, [f for _, f in fams], [n for n, _ in fams]


def crafted_duplex():
    """A clipped reverse anchor on the AB strand of a two-strand molecule, and on a BA-only molecule."""
    import random
    rng = random.Random(9)
    c = craft_genome()
    g = c[0].decode()
    L, p1, p2 = 40, 60, 90
    fams = []

    def strand(mi, suffix, n, rev_cigar, fwd_cigar):
        out = []
        fwd, rev = g[p1:p1 + L], g[p2:p2 + L]
        for i in range(n):
            if suffix == "A":      # R1 forward at p1, R2 reverse at p2
                out += [_duplex_rec(rng, f"a{mi}_{i}", fwd, fwd_cigar, F_PAIRED | F_FIRST | F_MATE_REVERSE, 0, p1, p2, f"{mi}/A", rev_cigar),
                        _duplex_rec(rng, f"a{mi}_{i}", rev, rev_cigar, F_PAIRED | F_LAST | F_REVERSE, 0, p2, p1, f"{mi}/A", fwd_cigar)]
            else:                  # R1 reverse at p2, R2 forward at p1
                out += [_duplex_rec(rng, f"b{mi}_{i}", rev, rev_cigar, F_PAIRED | F_FIRST | F_REVERSE, 0, p2, p1, f"{mi}/B", fwd_cigar),
                        _duplex_rec(rng, f"b{mi}_{i}", fwd, fwd_cigar, F_PAIRED | F_LAST | F_MATE_REVERSE, 0, p1, p2, f"{mi}/B", rev_cigar)]
        return out
    fams.append(("ab_clipped_reverse_anchor", strand("0", "A", 2, "2H3S33M4S1H", "40M") + strand("0", "B", 2, "40M", "40M")))
    fams.append(("ba_only_clipped_reverse_anchor", strand("1", "B", 3, "3H5S35M", "2S38M")))
    fams.append(("both_strands_clipped", strand("2", "A", 2, "4S36M", "36M4S") + strand("2", "B", 2, "1H39M1S", "3S37M")))
    return c, [f for _, f in fams], [n for n, _ in fams]


def expected_fwd_counts():
    """cu / ct of the forward `4S36M` family, by hand: column p lies at pos + p (the leading clip shifts the lookup); where the reference
    shows C, the three reads' C (p < 20) count as unconverted, their T (p >= 20) as converted."""
    g = craft_genome()[0].decode()
    cu = [FWD_N if (p < 20 and g[FWD_POS + p] == "C") else 0 for p in range(40)]
    ct = [FWD_N if (p >= 20 and g[FWD_POS + p] == "C") else 0 for p in range(40)]
    return cu, ct


def expected_rev_counts():
    """cu / ct of the reverse `3H2S30M5S1H` family, by hand: T = 41, column p lies at pos + 40 - p; the call is on the bottom strand (reverse, not
    LAST): where the reference shows G, the reads' A (columns 0 .. 16) count as converted, their G (17 .. 36) as unconverted."""
    g = craft_genome()[0].decode()
    cu = [REV_N if (p >= 17 and g[REV_POS + 40 - p] == "G") else 0 for p in range(37)]
    ct = [REV_N if (p < 17 and g[REV_POS + 40 - p] == "G") else 0 for p in range(37)]
    return cu, ct


# ---- the oracle, the product -----------------------------------------------------------------------------------------------------------------
def options(kind, mode, min_reads=None, **kw):
    if kind == 1:
        o = fgx_opts.defaults(kind=1, methylation_mode=mode, **kw)
        o.duplex_min_reads[0], o.duplex_min_reads[1], o.duplex_min_reads[2] = min_reads or (1, 1, 0)
        return o
    return fgx_opts.defaults(kind=0, methylation_mode=mode, min_reads=min_reads or 1, **kw)


def oracle(o, contigs, g):
    orc.set_reference(contigs)
    try:
        return orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=100 if o.caller_kind == 1 else 50)
    finally:
        orc.set_reference(None)


def split(data):
    from fgumi_amd import split_records
    return split_records(data)


def assert_same_records(got, want):
    if got != want:
        for i, (a, b) in enumerate(zip(split(got), split(want))):
            if a != b:
                raise AssertionError(f"record {i} differs:\n got {bamutil.parse(a)}\nwant {bamutil.parse(b)}")
        raise AssertionError(f"record count / length differs: {len(got)} bytes against {len(want)}")


def product(o, contigs, g, entry, on_gpu):
    """One batch through `entry` ("device": fgx_process_batch_device, "host": fgx_process_batch) of the loaded library.  `on_gpu`: the device
    entry takes tensors in HBM; else (the emulation library) host arrays stand in for them."""
    from fgumi_amd._lib import Options, Output, lib
    for f in ("fgx_debug_last_meth_device", "fgx_debug_last_meth_clipped"):
        getattr(lib, f).restype = C.c_uint32
        getattr(lib, f).argtypes = [C.c_void_p]
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
            d2 = (C.c_uint64 * 2)()
            lib.fgx_debug_last_deferral(h, d2)
            n_def = int(d2[0])
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
            n_def = int(nd.value)
        return dict(data=data, count=int(out.count), stats=np.array(list(out.stats), dtype=np.uint64), n_deferred=n_def, deferred=deferred,
                    meth_device=int(lib.fgx_debug_last_meth_device(h)), meth_clipped=int(lib.fgx_debug_last_meth_clipped(h)))
    finally:
        lib.fgx_destroy(h)


def check_all_on_device(o, contigs, groups, n_clip, entry, on_gpu, min_mm=50):
    """The batch against the oracle; nothing deferred; the clipped groups counted."""
    from fgumi_amd import GroupedReads
    g = GroupedReads.from_groups(groups)
    want = oracle(o, contigs, g)
    recs = [bamutil.parse(r) for r in split(want["data"])]
    n_mm = sum("MM" in r["tags"] for r in recs)
    assert n_mm > min_mm, n_mm                                         # (not an empty comparison)
    got = product(o, contigs, g, entry, on_gpu)
    print(f"{entry} entry: {g.n_grp} groups, {n_clip} with a clipped record; deferred {got['n_deferred']}, on the device {got['meth_device']}, "
          f"clipped and decided there {got['meth_clipped']}; oracle records with MM {n_mm}")
    assert got["n_deferred"] == 0, (got["n_deferred"], got["deferred"][:10] if got["deferred"] else None)
    assert got["meth_device"] == g.n_grp, got["meth_device"]
    assert got["meth_clipped"] == n_clip, (got["meth_clipped"], n_clip)
    assert got["count"] == want["count"]
    assert_same_records(got["data"], want["data"])
    assert np.array_equal(got["stats"], want["stats"]), (got["stats"].tolist(), want["stats"].tolist())
    return want


def check_ms_batch(kind, mode, min_reads, n_groups, seed, entry, on_gpu, kw=None):
    contigs, groups, n_clip = ms_batch(kind, n_groups, seed)
    return check_all_on_device(options(kind, mode, min_reads, **(kw or {})), contigs, groups, n_clip, entry, on_gpu)


def check_crafted(kind, entry, on_gpu):
    contigs, groups, names = crafted_duplex() if kind == 1 else crafted_simplex()
    n_clip = n_clipped_groups(groups)
    assert n_clip == len(groups)
    want = check_all_on_device(options(kind, 1), contigs, groups, n_clip, entry, on_gpu, min_mm=2)
    if kind == 0:
        recs = {r["name"].split(":")[-1]: r for r in (bamutil.parse(x) for x in split(want["data"]))}
        for mi, (cu, ct) in (("0", expected_fwd_counts()), ("1", expected_rev_counts())):
            assert sum(cu) > 0 and sum(ct) > 0, (mi, cu, ct)
            assert recs[mi]["tags"]["cu"][1] == cu and recs[mi]["tags"]["ct"][1] == ct, (mi, recs[mi]["tags"]["cu"], cu, recs[mi]["tags"]["ct"], ct)


def check_plain_counts_nothing(kind, entry, on_gpu):
    """Single-`M` groups only: fgx_debug_last_meth_clipped is 0."""
    contigs, groups, _ = ms_batch(kind, 120, 91)
    groups = [g for g in groups if not any(multi_op(r) for r in g)]
    assert len(groups) >= 50
    check_all_on_device(options(kind, 1), contigs, groups, 0, entry, on_gpu, min_mm=10)
