"""--max-reads-per-strand decided by the wavefront kernels (k_family_wave<1, 0, 1>, k_family_wave<2>), executed on the CPU in 64-lane lock-step
(tests/wavemu): one batch through fgx_process_batch_device of the emulation library against the oracle — nothing deferred, bytes, count and all 28
counters equal.  The strand callers' caps are not the simplex caller's: the duplex caller scores a set over its `cap` lowest name ranks IN RANK ORDER
and recounts the duplex errors over every read; the CODEC caller caps its R1 list and its R2 list on their own, in file order, and counts what it drops
as Downsampled."""
import ctypes as C

import numpy as np
import pytest

import bamutil
import fgx_opts
import orc
from isolated import run_isolated
from test_wavemu import check_device_entry, env

DUPLEX_SIM = dict(family_size=12, duplex=1)
CODEC_SIM = dict(family_size=4, read_length=300, insert_mean=350, insert_sd=60, codec=1)
REJ_DOWNSAMPLED = 19          # FGX_REJ_DOWNSAMPLED (include/fgumi_amd.h)


def rank(name):
    return orc.lib.orc_read_name_rank(name.encode(), len(name))


def set_sizes(g):
    """Per group: records per /A | /B x R1 | R2, read from the input."""
    out = []
    for gi in range(g.n_grp):
        cnt = {}
        for r in range(int(g.grp_first[gi]), int(g.grp_first[gi + 1])):
            off, ln = int(g.rec_off[r]), int(g.rec_len[r])
            p = bamutil.parse(bytes(g.blob[off:off + ln]))
            key = (p["tags"]["MI"][1][-2:], bool(p["flag"] & 0x40))
            cnt[key] = cnt.get(key, 0) + 1
        out.append(cnt)
    return out


def device_entry(kind, g, **opts):
    """fgx_process_batch_device on host arrays against the oracle: (parsed records of the oracle, the oracle's result).  Asserts nothing deferred, bytes, count, counters."""
    from fgumi_amd import split_records
    from fgumi_amd._lib import Options, Output, lib
    o = fgx_opts.defaults(kind=kind, **opts)
    want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=100)
    po = Options.from_buffer_copy(bytes(o))
    h = lib.fgx_create(C.byref(po))
    assert h, lib.fgx_global_error().decode()
    try:
        blob = np.concatenate([g.blob, np.zeros(64, dtype=np.uint8)])
        out, nd, dp = Output(), C.c_uint32(), C.c_void_p()
        rc = lib.fgx_process_batch_device(h, blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, g.grp_first.ctypes.data, g.n_grp,
                                          C.byref(out), C.byref(nd), C.byref(dp))
        assert rc == 0, lib.fgx_last_error(h).decode()
        assert nd.value == 0, f"{nd.value} of {g.n_grp} groups deferred"
        got = C.string_at(out.data, out.data_len) if out.data_len else b""
        if got != want["data"]:
            for i, (a, b) in enumerate(zip(split_records(got), split_records(want["data"]))):
                assert a == b, f"record {i} differs:\n got {bamutil.parse(a)}\nwant {bamutil.parse(b)}"
        assert int(out.count) == want["count"] and got == want["data"]
        stats = np.ctypeslib.as_array(out.stats, shape=(len(want["stats"]),))
        assert np.array_equal(np.array(stats, dtype=np.uint64), want["stats"]), (list(stats), want["stats"].tolist())
    finally:
        lib.fgx_destroy(h)
    return [bamutil.parse(r) for r in split_records(want["data"])], want


def oracle_only(kind, g, **opts):
    from fgumi_amd import split_records
    o = fgx_opts.defaults(kind=kind, **opts)
    want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=100)
    return [bamutil.parse(r) for r in split_records(want["data"])], want


# ---- simulated batches ---------------------------------------------------------------------------------------------------------------
def check_duplex_sim(cap, min_reads):
    from fgumi_amd import simulate_grouped_reads
    g = simulate_grouped_reads(400, **DUPLEX_SIM)
    # the cap bites every molecule: 12 pairs over two strands leave one strand at least 6, and cap <= 5
    sizes = set_sizes(g)
    assert len(sizes) == 400 and all(max(c.values()) > cap for c in sizes)
    device_entry(1, g, duplex_max_reads_per_strand=cap, duplex_min_reads=min_reads)


def check_codec_sim(cap):
    from fgumi_amd import simulate_grouped_reads
    g = simulate_grouped_reads(400, **CODEC_SIM)
    _, want = device_entry(2, g, codec_max_reads_per_strand=cap, overlapping_consensus=0)
    assert int(want["stats"][3 + REJ_DOWNSAMPLED]) > 0          # the comparison is not empty: the oracle dropped reads


@pytest.mark.parametrize("cap,min_reads", [(1, (1, 1, 0)), (3, (1, 1, 0)), (4, (3, 2, 1))], ids=["cap1", "cap3", "cap4_min_3_2_1"])
def test_duplex_cap_bites_every_simulated_molecule(cap, min_reads):
    run_isolated("test_wavemu_strand_cap", "check_duplex_sim", cap, min_reads, env=env(), timeout=1500)


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_codec_cap_on_simulated_molecules(cap):
    run_isolated("test_wavemu_strand_cap", "check_codec_sim", cap, env=env(), timeout=1500)


# ---- crafted molecules ---------------------------------------------------------------------------------------------------------------
# One duplex molecule: /A pairs have R1 forward at 100 and R2 reverse at 400, /B pairs R1 reverse at 400 and R2 forward at 100 — read set AB-R1 (forward
# reads, stored in read orientation) pairs with BA-R2 into the R1 duplex record.  The crafted columns sit in AB-R1; every reverse read has one length.
BASE = "ACGTTGCAAGCTTAGCCATG"
COL = 5                                  # the crafted column of AB-R1 (BASE[COL] = G)
TIE = ("t11788", "t19616")               # equal fgbio name ranks: the first repeated rank among the names t0, t1, t2, ... (a birthday search over 2^32 values)


def with_base(b, col=COL, seq=BASE):
    return seq[:col] + b + seq[col + 1:]


def duplex_molecule(ab, n_ba=1, mi="7"):
    """ab: (name, R1 sequence, R1 quality) per /A pair."""
    from fgumi_amd import GroupedReads
    recs = []
    for name, s1, q1 in ab:
        recs += list(bamutil.pair2(name, s1, q1, BASE, 37, mi + "/A", 100, 400))
    for i in range(n_ba):
        recs += list(bamutil.pair2(f"zb{i}", BASE, 37, BASE, 37, mi + "/B", 400, 100, rev1=True, rev2=False))
    return GroupedReads.from_groups([recs])


def names_by_rank(n, prefix="r", skip=()):
    """n distinct names, lowest fgbio name rank first."""
    pool = [f"{prefix}{i}" for i in range(4 * n + 8) if f"{prefix}{i}" not in skip]
    pool.sort(key=rank)
    assert len({rank(x) for x in pool[:n]}) == n
    return pool[:n]


def check_rank_order_is_the_summation_order():
    """(a) C,C,T,T at Q37 (the real-data pin of the tie rule: a one-ULP difference decides the call) in a set of five reads under a cap of 4, the names
    chosen so that the survivors' rank order is T,T,C,C while the file shows C,C,T,T."""
    s = names_by_rank(5)
    f = {"f0": s[2], "f1": s[3], "f2": s[0], "f3": s[1], "d": s[4]}          # ranks: f2 < f3 < f0 < f1 < d
    read = lambda who, b: (f[who], with_base(b), 37)
    file_order = [read("f0", "C"), read("f1", "C"), read("f2", "T"), read("f3", "T")]
    rank_order = [read("f2", "T"), read("f3", "T"), read("f0", "C"), read("f1", "C")]
    # the oracle itself is order-sensitive at this column: the same four reads, the cap off, two file orders
    a, _ = oracle_only(1, duplex_molecule(file_order))
    b, _ = oracle_only(1, duplex_molecule(rank_order))
    assert a[0]["tags"]["ac"][1][COL] != b[0]["tags"]["ac"][1][COL], (a[0]["tags"]["ac"], b[0]["tags"]["ac"])
    # the cap on: the fifth read (highest rank, in the middle of the file) is dropped and the other four enter the column by rank
    five = file_order[:2] + [read("d", "A")] + file_order[2:]
    w, _ = device_entry(1, duplex_molecule(five), duplex_max_reads_per_strand=4)
    assert w[0]["tags"]["aD"][1] == 4
    assert w[0]["tags"]["ac"][1][COL] == b[0]["tags"]["ac"][1][COL] and w[0]["tags"]["aq"][1][COL] == b[0]["tags"]["aq"][1][COL]


def check_equal_ranks_keep_file_order():
    """(b) TIE: two names of one rank.  With a third read of a lower rank and a cap of 2, the cap's second place is decided between the tied reads by file
    order — whichever comes first in the file stays, and the call at the crafted column follows it."""
    assert rank(TIE[0]) == rank(TIE[1]) and TIE[0] != TIE[1]
    low = next(n for n in (f"x{i}" for i in range(1000)) if rank(n) < rank(TIE[0]))
    seen = []
    for first, second in (TIE, TIE[::-1]):
        # the read called `first` carries C, the other T (Q40 against the low read's G at Q20: the kept one of the two decides the call)
        ab = [(low, BASE, 20), (first, with_base("C"), 40), (second, with_base("T"), 40)]
        w, _ = device_entry(1, duplex_molecule(ab), duplex_max_reads_per_strand=2)
        assert w[0]["tags"]["aD"][1] == 2 and w[0]["tags"]["ac"][1][COL] == "C"
        seen.append(w[0])
    off, _ = oracle_only(1, duplex_molecule([(low, BASE, 20), (TIE[0], with_base("C"), 40), (TIE[1], with_base("T"), 40)]))
    assert off[0]["tags"]["aD"][1] == 3


def check_longest_read_dropped():
    """(c) the longest read of AB-R1 has the highest rank: under a cap of 2 the single-strand consensus — and the duplex record — is as long as the longest
    SCORING read."""
    s = names_by_rank(3)
    long_read = BASE + "ACGTACGTAC"
    ab = [(s[0], BASE, 37), (s[2], long_read, 37), (s[1], BASE, 37)]
    from fgumi_amd import GroupedReads
    recs = []
    for name, s1, q1 in ab:
        recs += list(bamutil.pair2(name, s1, q1, BASE, 37, "9/A", 100, 400))
    recs += list(bamutil.pair2("zb0", BASE, 37, long_read, 37, "9/B", 400, 100, rev1=True, rev2=False))
    g = GroupedReads.from_groups([recs])
    off, _ = oracle_only(1, g)
    assert len(off[0]["seq"]) == len(long_read)
    w, _ = device_entry(1, g, duplex_max_reads_per_strand=2)
    assert len(w[0]["seq"]) == len(BASE) and w[0]["tags"]["aD"][1] == 2


def check_dropped_read_counts_in_the_recount():
    """(d) the read the cap drops disagrees with the duplex base at a column where no scoring read does: no single-strand error (aE = bE = 0), and cE counts it —
    the recount runs over every source read."""
    s = names_by_rank(3)
    ab = [(s[0], BASE, 37), (s[1], BASE, 37), (s[2], with_base("C", col=7), 37)]          # (BASE[7] = A)
    w, _ = device_entry(1, duplex_molecule(ab), duplex_max_reads_per_strand=2)
    t = w[0]["tags"]
    assert t["aD"][1] == 2 and t["aE"][1] == 0.0 and t["bE"][1] == 0.0 and sum(t["ae"][1]) == 0 and sum(t["be"][1]) == 0
    assert t["cE"][1] > 0.0 and abs(t["cE"][1] - 1.0 / (3 * len(BASE))) < 1e-6          # one error over the depth of the SCORING reads (2 + 1 per column)
    # where the error sits: a duplex record carries no per-base error tag of the duplex call (ad ae bd be ac bc aq bq only), so the column is pinned by
    # difference — the same molecule with the dropped read agreeing at column 7, and nothing else changed, has no error at all
    assert "ce" not in t
    same = [(s[0], BASE, 37), (s[1], BASE, 37), (s[2], BASE, 37)]
    w0, _ = device_entry(1, duplex_molecule(same), duplex_max_reads_per_strand=2)
    assert w0[0]["tags"]["cE"][1] == 0.0 and w0[0]["seq"] == w[0]["seq"] and w0[0]["tags"]["aD"][1] == 2


def check_cap_that_does_not_bite():
    """(f) a cap equal to the largest set, and one above it: the output of the cap-off run."""
    s = names_by_rank(3)
    g = duplex_molecule([(s[0], BASE, 37), (s[1], with_base("C"), 30), (s[2], BASE, 37)], n_ba=2)
    _, off = oracle_only(1, g)
    for cap in (3, 4):
        _, w = device_entry(1, g, duplex_max_reads_per_strand=cap)
        assert w["data"] == off["data"] and np.array_equal(w["stats"], off["stats"])
    from test_oracle_codec import fr_pair
    from fgumi_amd import GroupedReads
    fam = []
    for i in range(3):
        fam += fr_pair(f"t{i}", 1, 11, 35, "30M", "30M")
    gc = GroupedReads.from_groups([fam])
    _, off = oracle_only(2, gc, overlapping_consensus=0)
    for cap in (3, 4):
        _, w = device_entry(2, gc, codec_max_reads_per_strand=cap, overlapping_consensus=0)
        assert w["data"] == off["data"] and np.array_equal(w["stats"], off["stats"])


def check_codec_lists_cap_on_their_own():
    """(e) CODEC.  The R1 list and the R2 list are capped independently.  Inside the wavefront kernel's shape — every record an FR pair of one M op, mates
    adjacent — both lists hold the same templates in the same order under the same names, so they keep the same templates: the crafted batch shows the
    survivors staying in file order (the templates of the two lowest ranks among the FR pairs, wherever they lie in the file — every template carries a base
    and a quality of its own, so the consensus shows which ones stayed) with the dropped reads of BOTH lists counted.
    Lists that keep DIFFERENT templates need the alignment filter to drop a read of one list (here: an R2 with a deletion), which stays the general path's
    (the kernel defers before the cap); that molecule goes through the host entry, which splices both paths, and must equal the oracle too."""
    from test_oracle_codec import fr_pair
    from fgumi_amd import GroupedReads
    from fgumi_amd._lib import Options, Output, lib
    from test_oracle_codec import REF
    s = names_by_rank(6, prefix="c")
    order = [s[4], s[1], s[5], s[3], s[2]]                       # file order of the FR templates; the cap of 2 keeps s[1] and s[2]: the 2nd and the 5th template

    def template(n):
        """Every template shows a base of its own (column 14 + i of the reference, inside both reads) at a quality of its own: which templates a list kept
        can be read from the consensus."""
        i = order.index(n)
        c = 14 + i
        return fr_pair(n, 1, 11, 25 + 3 * i, "30M", "30M", ref=REF[:c] + "ACGT"[("ACGT".index(REF[c]) + 1) % 4] + REF[c + 1:])

    # s[0], the lowest rank of all, is no FR pair (both mates forward): it is in neither list and takes no place under the cap
    not_fr = fr_pair(s[0], 1, 11, 35, "30M", "30M", rev2=False)
    fam = list(not_fr)
    for n in order:
        fam += template(n)
    g = GroupedReads.from_groups([fam])
    w, res = device_entry(2, g, codec_max_reads_per_strand=2, overlapping_consensus=0)
    assert int(res["stats"][3 + REJ_DOWNSAMPLED]) == 6 and w[0]["tags"]["aD"][1] == 2 and w[0]["tags"]["bD"][1] == 2
    # the survivors are the two lowest ranks, not the first two of the file: the cap-off consensus of exactly those two templates, and not that of the first two
    by_rank, _ = oracle_only(2, GroupedReads.from_groups([not_fr + template(s[1]) + template(s[2])]), overlapping_consensus=0)
    by_file, _ = oracle_only(2, GroupedReads.from_groups([not_fr + template(order[0]) + template(order[1])]), overlapping_consensus=0)
    assert (w[0]["seq"], w[0]["quals"]) == (by_rank[0]["seq"], by_rank[0]["quals"]) != (by_file[0]["seq"], by_file[0]["quals"])
    # different templates per list: the R2 of the lowest-ranking template is a minority alignment
    fam = []
    for n in order:
        fam += fr_pair(n, 1, 11, 35, "30M", "12M1D17M" if n == s[1] else "30M")
    g = GroupedReads.from_groups([fam])
    o = fgx_opts.defaults(kind=2, codec_max_reads_per_strand=2, overlapping_consensus=0)
    want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=100)
    assert int(want["stats"][3 + REJ_DOWNSAMPLED]) == 3 + 2      # R1 list 5 -> 2, R2 list 4 -> 2
    po = Options.from_buffer_copy(bytes(o))
    h = lib.fgx_create(C.byref(po))
    assert h, lib.fgx_global_error().decode()
    try:
        out = Output()
        rc = lib.fgx_process_batch(h, g.blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, g.grp_first.ctypes.data, g.n_grp, C.byref(out))
        assert rc == 0, lib.fgx_last_error(h).decode()
        got = C.string_at(out.data, out.data_len) if out.data_len else b""
        assert int(out.count) == want["count"] and got == want["data"]
        assert np.array_equal(np.array(np.ctypeslib.as_array(out.stats, shape=(28,)), dtype=np.uint64), want["stats"])
    finally:
        lib.fgx_destroy(h)


@pytest.mark.parametrize("check", ["check_rank_order_is_the_summation_order", "check_equal_ranks_keep_file_order", "check_longest_read_dropped",
                                   "check_dropped_read_counts_in_the_recount", "check_codec_lists_cap_on_their_own", "check_cap_that_does_not_bite"])
def test_crafted_molecules(check):
    run_isolated("test_wavemu_strand_cap", check, env=env(), timeout=900)
