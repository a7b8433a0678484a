"""The duplex caller's methylation-aware mode (EM-Seq / TAPs) under --max-reads-per-strand, decided by k_family_wave<1, 1, 1> with the record writers'
<1, 1> builds and the tag kernels of duplex_meth.inc, executed on the CPU in 64-lane lock-step (tests/wavemu): one batch through
fgx_process_batch_device of the emulation library against the oracle with a reference set — nothing deferred, bytes, count and all 28 counters equal.

The rule (consensus_call, vanilla_caller.rs:706-779): annotate_and_normalize runs over ALL reads of a read set — the anchor is the last longest read of
the whole set, the unconverted / converted counts run over every read, every read is normalised — and only then the cap picks the `cap` lowest name ranks
as scoring reads; the annotation is truncated to the consensus (the longest scoring read), and the duplex error recount and the consensus UMI keep the
whole, normalised set."""
import ctypes as C

import numpy as np
import pytest

import bamutil
import fgx_opts
import methsim
import orc
from isolated import run_isolated
from test_wavemu import env
from test_wavemu_duplex_methylation import bamutil_split, plain_groups
from test_wavemu_strand_cap import BASE, COL, names_by_rank, set_sizes, with_base


# ---- the two sides ------------------------------------------------------------------------------------------------------------------------------------
def oracle_only(g, contigs, **opts):
    """(parsed records, the oracle's result) of the duplex caller with `contigs` as the reference."""
    o = fgx_opts.defaults(kind=1, **opts)
    orc.set_reference(contigs)
    try:
        want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=100)
    finally:
        orc.set_reference(None)
    return [bamutil.parse(r) for r in bamutil_split(want["data"])], want


def same_on_the_device(lib, g, contigs, want, o):
    """fgx_process_batch_device of the emulation library (host arrays stand in for the tensors in HBM) against the oracle's `want`: nothing deferred, bytes,
    count, the 28 counters, every group through the mode's device pipeline."""
    from fgumi_amd._lib import Options, Output
    lib.fgx_debug_last_meth_device.restype = C.c_uint32
    lib.fgx_debug_last_meth_device.argtypes = [C.c_void_p]
    po = Options.from_buffer_copy(bytes(o))
    h = lib.fgx_create(C.byref(po))
    assert h, lib.fgx_global_error().decode()
    try:
        bufs = [C.create_string_buffer(bytes(s), max(1, len(s))) for s in contigs]
        ptrs = (C.c_void_p * len(bufs))(*[C.cast(b, C.c_void_p).value for b in bufs])
        lens = (C.c_uint64 * len(bufs))(*[len(s) for s in contigs])
        assert lib.fgx_set_reference(h, len(bufs), ptrs, lens) == 0, lib.fgx_last_error(h).decode()
        blob = np.concatenate([g.blob, np.zeros(64, dtype=np.uint8)])
        out, nd, dp = Output(), C.c_uint32(), C.c_void_p()
        rc = lib.fgx_process_batch_device(h, blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, g.grp_first.ctypes.data, g.n_grp,
                                          C.byref(out), C.byref(nd), C.byref(dp))
        assert rc == 0, lib.fgx_last_error(h).decode()
        assert nd.value == 0, f"{nd.value} of {g.n_grp} groups deferred"
        got = C.string_at(out.data, out.data_len) if out.data_len else b""
        if got != want["data"]:
            for i, (a, b) in enumerate(zip(bamutil_split(got), bamutil_split(want["data"]))):
                assert a == b, f"record {i} differs:\n got {bamutil.parse(a)}\nwant {bamutil.parse(b)}"
        assert int(out.count) == want["count"] and got == want["data"]
        assert np.array_equal(np.array(list(out.stats), dtype=np.uint64), want["stats"]), (list(out.stats), want["stats"].tolist())
        assert int(lib.fgx_debug_last_meth_device(h)) == g.n_grp
    finally:
        lib.fgx_destroy(h)


def device_entry(g, contigs, **opts):
    """The emulated kernels against the oracle; returns (parsed records of the oracle, the oracle's result)."""
    from fgumi_amd._lib import lib
    recs, want = oracle_only(g, contigs, **opts)
    same_on_the_device(lib, g, contigs, want, fgx_opts.defaults(kind=1, **opts))
    return recs, want


# ---- the simulated batch --------------------------------------------------------------------------------------------------------------------------------
def sim_batch(seed, n_groups=400):
    """The one-op molecules of methsim's duplex batch at 1 - 6 pairs per strand."""
    from fgumi_amd import GroupedReads
    rng = methsim.seeded(seed)
    contigs = methsim.genome(rng)
    groups = plain_groups(methsim.duplex_groups(rng, contigs, n_groups, depth=(1, 6)))
    return contigs, GroupedReads.from_groups(groups)


def cap_bites(g, cap):
    """Molecules with a read set above the cap, counted from the input."""
    return sum(1 for c in set_sizes(g) if max(c.values()) > cap)


def check_sim(mode, cap, min_reads=(1, 1, 0), seed=71):
    contigs, g = sim_batch(seed)
    assert g.n_grp > 200 and 2 * cap_bites(g, cap) >= g.n_grp, (cap_bites(g, cap), g.n_grp)          # (a condition on the input: the cap bites most molecules)
    recs, _ = device_entry(g, contigs, methylation_mode=mode, duplex_max_reads_per_strand=cap, duplex_min_reads=min_reads)
    tags = [r["tags"] for r in recs]
    assert sum("au" in t and "bu" in t for t in tags) > 100 and sum("MM" in t for t in tags) > 100, len(tags)      # (not an empty comparison)
    if cap == 1:          # the one-member column path: a capped strand's depth is 1 in nearly every record
        assert sum(t["aD"][1] == 1 for t in tags) > 100


@pytest.mark.parametrize("mode", [1, 2], ids=["em_seq", "taps"])
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_cap_bites_most_simulated_molecules(mode, cap):
    run_isolated("test_wavemu_duplex_meth_cap", "check_sim", mode, cap, (1, 1, 0), 70 + mode, env=env(), timeout=1500)


def test_cap_with_deeper_min_reads():
    run_isolated("test_wavemu_duplex_meth_cap", "check_sim", 1, 2, (3, 2, 1), env=env(), timeout=1500)


# ---- crafted molecules ----------------------------------------------------------------------------------------------------------------------------------
# The molecule of tests/test_wavemu_strand_cap.py on a genome: /A pairs have R1 forward at 100 (1-based) and R2 reverse at 400, /B pairs R1 reverse at 400
# and R2 forward at 100; the genome shows LONG (BASE and ten more bases) at both places.  AB-R1 — forward R1 reads: the top strand, C / T against a
# reference C — pairs with BA-R2 — forward R2 reads: the bottom strand, G / A against a reference G — into the R1 duplex record.
LONG = BASE + "ACGTACGTAC"
REF_C = [i for i, b in enumerate(BASE) if b == "C"]          # 1, 6, 10, 15, 16
REF_G = [i for i, b in enumerate(BASE) if b == "G"]


def crafted_genome():
    fill = "AT" * 400
    return [(fill[:99] + LONG + fill[:270] + LONG + fill[:200]).encode()]


def molecule(ab, ba=(("zb0", BASE, 37),), mi="7", ref_id=0, ab_r2=BASE, ba_r2=None):
    """ab: per /A pair (name, R1 sequence, R1 quality[, 1-based start of R1]); ba: per /B pair (name, R1 sequence — reverse, stored in reference
    orientation —, R1 quality); `ba_r2`: the forward R2 of every /B pair."""
    from fgumi_amd import GroupedReads
    recs = []
    for name, s1, q1, *start in ab:
        recs += list(bamutil.pair2(name, s1, q1, ab_r2, 37, mi + "/A", start[0] if start else 100, 400, ref_id=ref_id))
    for name, s1, q1 in ba:
        recs += list(bamutil.pair2(name, s1, q1, ba_r2 or BASE, 37, mi + "/B", 400, 100, rev1=True, rev2=False, ref_id=ref_id))
    return GroupedReads.from_groups([recs])


EM = dict(methylation_mode=1)


def records_of(g):
    """The raw records of a batch, for putting several crafted molecules into one."""
    return [bytes(g.blob[int(o):int(o) + int(n)]) for o, n in zip(g.rec_off, g.rec_len)]


def expect_dropped_read_carries_the_conversion(recs, off):
    """(a) `recs`: the capped run, `off`: the same molecule with the mode off."""
    t = recs[0]["tags"]
    c = REF_C[1]
    assert t["aD"][1] == 2 and t["ad"][1][c] == 2
    assert t["au"][1][c] == 2 and t["at"][1][c] == 1                  # every read of the set: more than the depth of the scoring reads
    assert t["cu"][1][c] == 2 and t["ct"][1][c] == 1                  # (the bottom strand has no cytosine of its own at a reference C)
    assert [t["au"][1][i] + t["at"][1][i] for i in REF_C] == [3] * len(REF_C) and sum(t["at"][1]) == 1
    assert t["cE"][1] == 0.0 and t["aE"][1] == 0.0                    # the recount sees the normalised base
    assert off[0]["tags"]["cE"][1] > 0.0 and "au" not in off[0]["tags"]


def crafted_a(mi="7"):
    s = names_by_rank(3)
    return molecule([(s[0], BASE, 37), (s[1], BASE, 37), (s[2], with_base("T", col=REF_C[1]), 37)], mi=mi)


def check_dropped_read_carries_the_conversion():
    g, ref = crafted_a(), crafted_genome()
    w, _ = device_entry(g, ref, duplex_max_reads_per_strand=2, **EM)
    off, _ = oracle_only(g, ref, duplex_max_reads_per_strand=2)
    expect_dropped_read_carries_the_conversion(w, off)


def expect_dropped_read_counts_in_the_recount(recs, same):
    """(b) `same`: the molecule whose dropped read agrees."""
    t = recs[0]["tags"]
    assert t["aD"][1] == 2 and t["aE"][1] == 0.0 and t["bE"][1] == 0.0 and sum(t["ae"][1]) == 0 and sum(t["be"][1]) == 0
    assert t["cE"][1] > 0.0 and abs(t["cE"][1] - 1.0 / (3 * len(BASE))) < 1e-6          # one error over the depth of the SCORING reads (2 + 1 per column)
    assert "au" in t and "MM" in t
    assert same[0]["tags"]["cE"][1] == 0.0 and same[0]["seq"] == recs[0]["seq"] and same[0]["tags"]["aD"][1] == 2


def crafted_b(agree=False, mi="7"):
    s = names_by_rank(3)
    return molecule([(s[0], BASE, 37), (s[1], BASE, 37), (s[2], BASE if agree else with_base("C", col=7), 37)], mi=mi)          # (BASE[7] = A: no reference cytosine)


def check_dropped_read_disagrees_off_a_cytosine():
    ref = crafted_genome()
    w, _ = device_entry(crafted_b(), ref, duplex_max_reads_per_strand=2, **EM)
    w0, _ = device_entry(crafted_b(agree=True), ref, duplex_max_reads_per_strand=2, **EM)
    expect_dropped_read_counts_in_the_recount(w, w0)


def expect_longest_read_dropped(recs, off):
    """(c) `off`: the cap-off run, whose record and annotation run over the long read."""
    t, n = recs[0]["tags"], len(BASE)
    assert len(recs[0]["seq"]) == n and t["aD"][1] == 2
    for k in ("ad", "ae", "au", "at", "bu", "bt", "cu", "ct"):
        assert len(t[k][1]) == n, (k, t[k])
    assert len(t["ac"][1]) == n and sum(t["au"][1]) == 3 * len(REF_C)                   # every read of the set, inside the consensus only
    to = off[0]["tags"]
    assert len(off[0]["seq"]) == len(LONG) and len(to["au"][1]) == len(LONG) and sum(to["au"][1][n:]) > 0          # the reference C's beyond: no trace above
    assert t["MM"][1] != to["MM"][1]


def crafted_c(mi="7"):
    s = names_by_rank(3)
    return molecule([(s[0], BASE, 37), (s[1], BASE, 37), (s[2], LONG, 37)], ba_r2=LONG, mi=mi)          # the dropped read: longest, last


def check_longest_read_dropped():
    g, ref = crafted_c(), crafted_genome()
    w, _ = device_entry(g, ref, duplex_max_reads_per_strand=2, **EM)
    off, _ = oracle_only(g, ref, **EM)
    expect_longest_read_dropped(w, off)


def crafted_d(anchor_dropped, mi="7"):
    """Two places in one forward set (hostile input the kernel accepts): the read the cap drops lies three bases to the right.  As the longest read it is the
    anchor; one base shorter than the others it is not — the last longest scoring read is."""
    s = names_by_rank(3)
    moved = LONG[3:] if anchor_dropped else LONG[3:3 + len(BASE) - 1]
    return molecule([(s[0], BASE, 37), (s[1], BASE, 37), (s[2], moved, 37, 103)], ba_r2=LONG, mi=mi)


def expect_anchor_over_all_reads(by_dropped, by_scoring):
    a, b = by_dropped[0]["tags"], by_scoring[0]["tags"]
    assert len(by_dropped[0]["seq"]) == len(by_scoring[0]["seq"]) == len(BASE) and a["aD"][1] == b["aD"][1] == 2
    flagged = lambda t: [i for i, (u, v) in enumerate(zip(t["au"][1], t["at"][1])) if u + v]
    assert flagged(b) == REF_C and flagged(a) == [i - 3 for i in [j for j, x in enumerate(LONG) if x == "C"] if 0 <= i - 3 < len(BASE)]
    assert a["cu"][1] != b["cu"][1] and a["MM"][1] != b["MM"][1]


def check_anchor_over_all_reads():
    ref = crafted_genome()
    a, _ = device_entry(crafted_d(True), ref, duplex_max_reads_per_strand=2, **EM)
    b, _ = device_entry(crafted_d(False), ref, duplex_max_reads_per_strand=2, **EM)
    expect_anchor_over_all_reads(a, b)


def crafted_e(mi="7"):
    """C,C,T,T at Q37 (the one-ULP pin of check_rank_order_is_the_summation_order) at COL, where the genome shows a G: nothing is normalised there, so the order
    the scoring reads enter the column in decides the call."""
    s = names_by_rank(5)
    f = {"f0": s[2], "f1": s[3], "f2": s[0], "f3": s[1], "d": s[4]}          # ranks: f2 < f3 < f0 < f1 < d
    read = lambda who, b: (f[who], with_base(b), 37)
    file_order = [read("f0", "C"), read("f1", "C"), read("f2", "T"), read("f3", "T")]
    rank_order = [read("f2", "T"), read("f3", "T"), read("f0", "C"), read("f1", "C")]
    five = file_order[:2] + [read("d", "A")] + file_order[2:]
    return molecule(file_order, mi=mi), molecule(rank_order, mi=mi), molecule(five, mi=mi)


def expect_rank_order_is_the_summation_order(recs, by_file, by_rank):
    assert BASE[COL] == "G" and COL not in REF_C
    assert by_file[0]["tags"]["ac"][1][COL] != by_rank[0]["tags"]["ac"][1][COL], (by_file[0]["tags"]["ac"], by_rank[0]["tags"]["ac"])
    t = recs[0]["tags"]
    assert t["aD"][1] == 4 and "au" in t
    assert t["ac"][1][COL] == by_rank[0]["tags"]["ac"][1][COL] and t["aq"][1][COL] == by_rank[0]["tags"]["aq"][1][COL]


def check_rank_order_is_the_summation_order():
    ref = crafted_genome()
    g_file, g_rank, g_five = crafted_e()
    a, _ = oracle_only(g_file, ref, **EM)
    b, _ = oracle_only(g_rank, ref, **EM)
    w, _ = device_entry(g_five, ref, duplex_max_reads_per_strand=4, **EM)
    expect_rank_order_is_the_summation_order(w, a, b)


def crafted_f(mi="7"):
    s = names_by_rank(3)
    return molecule([(s[0], BASE, 37), (s[1], with_base("T", col=REF_C[0]), 30), (s[2], BASE, 37)], ba=(("zb0", BASE, 37), ("zb1", BASE, 37)), mi=mi)


def check_cap_that_does_not_bite():
    """(f) a cap equal to the largest set, and one above it: the bytes of the cap-off run of the mode."""
    g, ref = crafted_f(), crafted_genome()
    recs, off = oracle_only(g, ref, **EM)
    assert "MM" in recs[0]["tags"] and sum(recs[0]["tags"]["at"][1]) == 1
    for cap in (3, 4):
        _, w = device_entry(g, ref, duplex_max_reads_per_strand=cap, **EM)
        assert w["data"] == off["data"] and np.array_equal(w["stats"], off["stats"])


def crafted_g(ref_id, mi="7"):
    s = names_by_rank(3)
    return molecule([(s[0], BASE, 37), (s[1], BASE, 37), (s[2], with_base("T", col=REF_C[1]), 37)], ref_id=ref_id, mi=mi)


def expect_no_annotation_outside_the_genome(recs, inside):
    t = recs[0]["tags"]
    assert t["aD"][1] == 2                                            # the cap is applied
    assert not any(k in t for k in ("au", "at", "bu", "bt", "cu", "ct", "MM", "ML"))
    assert t["cE"][1] > 0.0                                           # nothing normalised: the dropped read's T is an error of the recount
    assert "au" in inside[0]["tags"] and inside[0]["tags"]["cE"][1] == 0.0


def check_anchor_outside_the_genome():
    ref = crafted_genome()
    w, _ = device_entry(crafted_g(5), ref, duplex_max_reads_per_strand=2, **EM)
    inside, _ = oracle_only(crafted_g(0), ref, duplex_max_reads_per_strand=2, **EM)
    expect_no_annotation_outside_the_genome(w, inside)


def crafted_h(mi="7"):
    """Three /B pairs: BA-R1 is a REVERSE set above a cap of 2 (the regular step compares the stored codes with the complements of the call's bases).  A reverse
    set's bases are compared in read orientation with the reference base as it stands (annotate_simplex_methylation), so a bottom-strand read shows its
    unconverted G where it stores a C over a reference G, and the converted A where it stores a T: the scoring reads (and AB-R2, so that the strands
    agree) store the C, the read the cap drops alone the T."""
    s = names_by_rank(3, prefix="h")
    c, t = with_base("C", col=REF_G[2]), with_base("T", col=REF_G[2])
    return molecule([("za0", BASE, 37)], ba=((s[0], c, 37), (s[1], c, 37), (s[2], t, 37)), ab_r2=c, mi=mi)


def expect_reverse_set(recs, off):
    r2 = next(r for r in recs if r["flag"] & 0x80)                    # the R2 duplex record: AB-R2 with BA-R1
    t = r2["tags"]
    col = len(BASE) - 1 - REF_G[2]
    assert t["bD"][1] == 2 and t["bu"][1][col] == 2 and t["bt"][1][col] == 1 and sum(t["bu"][1]) == 2 and sum(t["bt"][1]) == 1
    assert t["cE"][1] == 0.0
    assert next(r for r in off if r["flag"] & 0x80)["tags"]["cE"][1] > 0.0


def check_reverse_set():
    g, ref = crafted_h(), crafted_genome()
    w, _ = device_entry(g, ref, duplex_max_reads_per_strand=2, **EM)
    off, _ = oracle_only(g, ref, duplex_max_reads_per_strand=2)
    expect_reverse_set(w, off)


def check_per_field_writer():
    """k_emit_duplex<1, 1> — the per-field writer's build for the mode under a cap: under a 70-character read-name prefix the one-store writer refuses every
    record; (a) and (h) once more, their recounts read from the all-reads counts."""
    from test_wavemu_record_writers import writer_counts
    ref, kw = crafted_genome(), dict(duplex_max_reads_per_strand=2, read_name_prefix=b"k" * 70, **EM)
    for g in (crafted_a(), crafted_h()):
        w, want = device_entry(g, ref, **kw)
        assert writer_counts(want["data"]) == (0, want["count"])
        assert all(r["tags"]["cE"][1] == 0.0 for r in w) and sum(sum(r["tags"].get("at", ("", []))[1]) + sum(r["tags"].get("bt", ("", []))[1]) for r in w) == 1


CRAFTED = ["check_dropped_read_carries_the_conversion", "check_dropped_read_disagrees_off_a_cytosine", "check_longest_read_dropped", "check_anchor_over_all_reads",
           "check_rank_order_is_the_summation_order", "check_cap_that_does_not_bite", "check_anchor_outside_the_genome", "check_reverse_set", "check_per_field_writer"]


@pytest.mark.parametrize("check", CRAFTED)
def test_crafted_molecules(check):
    run_isolated("test_wavemu_duplex_meth_cap", check, env=env(), timeout=900)
