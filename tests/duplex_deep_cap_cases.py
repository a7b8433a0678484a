"""Inputs and the runner of the tests of --max-reads-per-strand in the deep duplex kernels (tests/test_wavemu_duplex_deep_cap.py on the CPU,
tests/test_gpu_duplex_deep_cap.py on the GPU): duplex molecules of more than 64 records with a set above the cap, which k_duplex_deep_parse used to defer and
the CAP builds of fgumi_amd/csrc/duplex_deep.inc decide under FGX_DUPLEX_DEEP_CAP=1.  Every check compares the device entry and the host entry with the oracle —
bytes, count and all 28 counters — and asserts the path of the device batch: molecules deferred, fgx_debug_last_duplex_deep, fgx_debug_last_duplex_deep_capped,
nothing counted as a simplex big / deep family.  Every check also reads from its own input what the cap does to it (set_sizes, name ranks): a change of the
simulator cannot empty a test silently.  The callers of these checks set the switch; nothing here does."""
import dataclasses
import os

import numpy as np

import bamutil
import duplex_deep_cases as D
from duplex_deep_cases import Case, Caller, check, want_of, assert_equal
from max_reads_cases import READ_THROUGH, rank, with_tied_names
from wide_cases import _rx_value, records_per_family

SWITCH = "FGX_DUPLEX_DEEP_CAP"
SETS = ("AB-R1", "AB-R2", "BA-R1", "BA-R2")


def _records(g, gi):
    return [bytes(r) for r in g.records(gi)]


def _set_of(rec):
    """0 = AB-R1, 1 = AB-R2, 2 = BA-R1, 3 = BA-R2 of a paired record with an MI that ends in /A or /B, else -1."""
    f = D._flag(rec)
    if not (f & D.PAIRED):
        return -1
    s = D._strand(rec)
    if s not in "AB":
        return -1
    return (0 if s == "A" else 2) + (0 if f & D.FIRST else 1)


def _name(rec):
    return bytes(rec[32:32 + rec[8] - 1])


def set_sizes(g):
    """Per molecule: the record counts of the four sets, from the flags and the MI suffix."""
    out = np.zeros((g.n_grp, 4), dtype=np.int64)
    for gi in range(g.n_grp):
        for r in _records(g, gi):
            k = _set_of(r)
            if k >= 0:
                out[gi, k] += 1
    return out


def bitten(g, cap):
    """Per molecule: the sets (0 .. 3) of more than `cap` records."""
    return [[k for k in range(4) if row[k] > cap] for row in set_sizes(g).tolist()]


def scoring(recs, cap):
    """The records of one molecule that the cap leaves for the columns, in file order: of every set of more than `cap` records the `cap` lowest fgbio name
    ranks, ties in file order; every record of the other sets and every record outside the four sets."""
    keep = set(range(len(recs)))
    for k in range(4):
        members = [i for i, r in enumerate(recs) if _set_of(r) == k]
        if len(members) > cap:
            order = sorted(members, key=lambda i: (rank(_name(recs[i])), i))
            keep -= set(order[cap:])
    return [recs[i] for i in sorted(keep)]


def sets_with_a_tie_cut_in_the_middle(g, cap):
    """How many sets of the batch have, in the cap's order (rank, then file order), the read in place `cap` and the read in place `cap` + 1 under one rank."""
    n = 0
    for gi in range(g.n_grp):
        recs = _records(g, gi)
        for k in range(4):
            order = sorted((rank(_name(r)), i) for i, r in enumerate(recs) if _set_of(r) == k)
            n += len(order) > cap and order[cap - 1][0] == order[cap][0]
    return n


class CapCaller(Caller):
    def __init__(self, contigs=None, **opts):
        super().__init__(contigs, **opts)
        import ctypes as C
        self.lib.fgx_debug_last_duplex_deep_capped.restype = C.c_uint32
        self.lib.fgx_debug_last_duplex_deep_capped.argtypes = [C.c_void_p]

    def path(self):
        return dict(super().path(), capped=int(self.lib.fgx_debug_last_duplex_deep_capped(self.h)))


PATH_KEYS = D.PATH_KEYS + ("capped",)


def check_cap(case, capped, want=None, contigs=None):
    """duplex_deep_cases.check with the counter of capped molecules: both entries against the oracle, `case.deferred` molecules deferred, `case.deep` decided by
    the deep kernels, `capped` of them bitten by the cap."""
    want = want or want_of(case, contigs)
    c = CapCaller(contigs, **case.opts)
    try:
        got = c.device(case.g)
        path = {k: got[k] for k in PATH_KEYS}
        print(f"path {path}", flush=True)
        assert path == dict(deferred=case.deferred, duplex_deep=case.deep, big=0, deep=0, capped=capped), (path, case.deferred, case.deep, capped)
        assert got["capped"] <= got["duplex_deep"]
        if case.deferred == 0:
            assert_equal(got, want, "device entry")
        assert_equal(c.host(case.g), want, "host entry")
    finally:
        c.close()
    return want


def _switch_is(value):
    assert os.environ.get(SWITCH) == value, (SWITCH, os.environ.get(SWITCH), value)


def _tags(data):
    from fgumi_amd import split_records
    return [bamutil.parse(r) for r in split_records(data)]


def _cap(n, **more):
    return dict(duplex_max_reads_per_strand=n, **more)


# ---- 1. the feature: two molecules of 40 pairs under a cap of 5 ------------------------------------------------------------------------------------------
def two_molecules():
    g = D._sim(2, family_size=40)
    assert records_per_family(g).tolist() == [80, 80]
    return g


def check_two_molecules_under_a_cap_of_5():
    _switch_is("1")
    g = two_molecules()
    assert all(len(b) >= 1 for b in bitten(g, 5)), set_sizes(g).tolist()
    check_cap(Case(g, opts=_cap(5)), capped=2)


# ---- 2. a cap of 1: every set through the single-read table -------------------------------------------------------------------------------------------------
def check_cap_of_1():
    _switch_is("1")
    g = two_molecules()
    assert set_sizes(g).min() > 1 and all(b == [0, 1, 2, 3] for b in bitten(g, 1)), set_sizes(g).tolist()
    want = check_cap(Case(g, opts=_cap(1)), capped=2)
    recs = _tags(want["data"])
    assert len(recs) == 4 and all(r["tags"]["aD"][1] == 1 and r["tags"]["bD"][1] == 1 for r in recs)


# ---- 3. the edges of biting: M - 1, M, M + 1 ----------------------------------------------------------------------------------------------------------------
def check_edges_of_biting():
    _switch_is("1")
    g = D._sim(1, family_size=40)
    M = int(set_sizes(g).max())
    assert M >= 2
    off = want_of(Case(g))
    for cap, capped in ((M - 1, 1), (M, 0), (M + 1, 0)):
        assert (len(bitten(g, cap)[0]) > 0) == bool(capped)
        want = check_cap(Case(g, opts=_cap(cap)), capped=capped)
        if not capped:
            assert want["data"] == off["data"] and np.array_equal(want["stats"], off["stats"])
        else:
            assert want["data"] != off["data"]


# ---- 4. one strand capped, the other not ---------------------------------------------------------------------------------------------------------------------
def one_strand_capped():
    g = D._sim(2, family_size=60, seed=3)
    recs = _records(g, 0)
    a, b = [r for r in recs if D._strand(r) == "A"], [r for r in recs if D._strand(r) == "B"]
    assert len(a) >= 60 and len(b) >= 8, (len(a), len(b))
    g = D._groups([a[:60] + b[:8], _records(g, 1)[:70]])
    assert set_sizes(g)[0].tolist() == [30, 30, 4, 4] and records_per_family(g).tolist() == [68, 70]
    return g


def check_one_strand_capped(min_reads):
    _switch_is("1")
    g = one_strand_capped()
    assert bitten(g, 8)[0] == [0, 1]                                   # the uncapped BA sets' recount comes from the col_obs copy
    n_capped = sum(len(b) > 0 for b in bitten(g, 8))
    opts = _cap(8) if min_reads is None else _cap(8, duplex_min_reads=min_reads)
    want = check_cap(Case(g, opts=opts), capped=n_capped)
    if min_reads is not None:
        # (3, 2, 1): the depths AFTER the cap decide — 8 and 4 pass; the same molecule under a cap of 1 shows 1 and 1 and is not emitted
        assert want["count"] >= 2
        low = want_of(Case(g, opts=_cap(1, duplex_min_reads=min_reads)))
        assert low["count"] == 0
        check_cap(Case(g, opts=_cap(1, duplex_min_reads=min_reads)), capped=2, want=low)


# ---- 5. the longest read is dropped ----------------------------------------------------------------------------------------------------------------------------
def check_longest_read_dropped():
    """Read-through inserts: final lengths differ inside a set.  Read from the input through the oracle: the molecule cut to its scoring reads gives shorter
    records than the whole molecule (no scoring read of some capped set has the set's greatest final length), and the cap gives those shorter records."""
    _switch_is("1")
    cap = 3
    found = None
    for seed in range(1, 40):
        g = D._sim(1, family_size=40, seed=seed, **READ_THROUGH)
        if not bitten(g, cap)[0]:
            continue
        whole = _tags(want_of(Case(g))["data"])
        cut = _tags(want_of(Case(D._groups([scoring(_records(g, 0), cap)])))["data"])
        if len(whole) == 2 and len(cut) == 2 and any(len(c["seq"]) < len(w["seq"]) for c, w in zip(cut, whole)):
            found = (seed, g, whole, cut)
            break
    assert found, "no seed below 40 drops the longest read of a capped set"
    seed, g, whole, cut = found
    print(f"seed {seed}: record lengths {[len(w['seq']) for w in whole]} without the cap, {[len(c['seq']) for c in cut]} over the scoring reads", flush=True)
    want = check_cap(Case(g, opts=_cap(cap)), capped=1)
    got = _tags(want["data"])
    assert [len(r["seq"]) for r in got] == [len(c["seq"]) for c in cut] and any(len(r["seq"]) < len(w["seq"]) for r, w in zip(got, whole))


# ---- 6. rank order is the summation order -------------------------------------------------------------------------------------------------------------------
def check_rank_order_is_the_summation_order():
    """C, C, T, T at Q37 in one column (the one-ULP pin of tests/test_wavemu_strand_cap.py) in a molecule of 74 records: AB-R1 holds 36 reads, the four crafted
    ones under the four lowest name ranks, in the file C, C, T, T and by rank T, T, C, C; a cap of 4 leaves exactly those four."""
    _switch_is("1")
    from test_wavemu_strand_cap import BASE, COL, duplex_molecule, names_by_rank, oracle_only, with_base
    s = names_by_rank(36)
    f = {"f0": s[2], "f1": s[3], "f2": s[0], "f3": s[1]}                 # ranks: f2 < f3 < f0 < f1 < every other read
    read = lambda who, b: (f[who], with_base(b), 37)
    file_order = [read("f0", "C"), read("f1", "C"), read("f2", "T"), read("f3", "T")]
    rank_order = [read("f2", "T"), read("f3", "T"), read("f0", "C"), read("f1", "C")]
    a, _ = oracle_only(1, duplex_molecule(file_order))
    b, _ = oracle_only(1, duplex_molecule(rank_order))
    assert (a[0]["tags"]["ac"][1][COL], a[0]["tags"]["aq"][1][COL]) != (b[0]["tags"]["ac"][1][COL], b[0]["tags"]["aq"][1][COL])     # the two orders differ
    rest = [(n, with_base("A"), 37) for n in s[4:]]
    g = duplex_molecule(file_order[:2] + rest[:16] + file_order[2:] + rest[16:])
    assert records_per_family(g).tolist() == [74] and set_sizes(g).tolist() == [[36, 36, 1, 1]]
    walk = [_name(r).decode() for r in scoring([r for r in _records(g, 0) if _set_of(r) == 0], 4)]
    assert sorted(walk, key=lambda x: rank(x.encode())) == [f["f2"], f["f3"], f["f0"], f["f1"]] and walk == [f["f0"], f["f1"], f["f2"], f["f3"]]
    want = check_cap(Case(g, opts=_cap(4)), capped=1)
    w = _tags(want["data"])
    assert w[0]["tags"]["aD"][1] == 4
    assert w[0]["tags"]["ac"][1][COL] == b[0]["tags"]["ac"][1][COL] and w[0]["tags"]["aq"][1][COL] == b[0]["tags"]["aq"][1][COL]


# ---- 7. ties ---------------------------------------------------------------------------------------------------------------------------------------------------
def check_ties(overlapping):
    _switch_is("1")
    g = with_tied_names(D._sim(2, family_size=40), run=3)
    sizes = set_sizes(g)
    cap = next(c for c in range(2, int(sizes.max())) if sets_with_a_tie_cut_in_the_middle(g, c) > 0 and all(len(b) for b in bitten(g, c)))
    print(f"cap {cap}: {sets_with_a_tie_cut_in_the_middle(g, cap)} sets cut inside a run of equal ranks", flush=True)
    if overlapping:
        # duplicate names under the pairing by name: only that no molecule is miscalled — one the device entry keeps is the oracle's byte for byte (the
        # record kernel pairs a name's LAST R1 as the reference does, and defers a name it cannot verify), the host entry is the oracle's either way
        c = CapCaller(**_cap(cap))
        try:
            n_def = c.device(g)["deferred"]
        finally:
            c.close()
        assert 0 <= n_def <= 2
        check_cap(Case(g, opts=_cap(cap), deferred=n_def), capped=2 - n_def)
    else:
        check_cap(Case(g, opts=_cap(cap, overlapping_consensus=0)), capped=2)


# ---- 8. the consensus UMI over all reads, in file order ----------------------------------------------------------------------------------------------------
def check_umi_over_all_reads():
    _switch_is("1")
    cap = 6
    g0 = D.umi_disagreement().g
    recs = [bytearray(r) for r in _records(g0, 0)]
    keep = {id(r) for r in scoring(recs, cap)}
    # every read the cap drops carries a disagreeing first RX character; the scoring reads agree
    first = None
    for r in recs:
        o, ln = _rx_value(r)
        if first is None:
            first = r[o] if id(r) in keep else None
    assert first is not None
    other = ord("C") if first == ord("A") else ord("A")
    for r in recs:
        o, ln = _rx_value(r)
        r[o] = first if id(r) in keep else other
    g = D._groups([recs])
    assert bitten(g, cap)[0] == [0, 1, 2, 3]
    want = check_cap(Case(g, opts=_cap(cap)), capped=1)
    only = want_of(Case(D._groups([scoring(_records(g, 0), cap)])))
    rx_all, rx_scoring = [r["tags"]["RX"][1] for r in _tags(want["data"])], [r["tags"]["RX"][1] for r in _tags(only["data"])]
    print(f"RX over all reads {rx_all}, over the scoring reads {rx_scoring}", flush=True)
    assert len(rx_all) == 2 and rx_all != rx_scoring


# ---- 9. the bound under a cap -----------------------------------------------------------------------------------------------------------------------------------
def check_the_bound_under_a_cap():
    _switch_is("1")
    from fgumi_amd import GroupedReads
    case = D.the_bound()                                              # 255 pairs, then 256 pairs
    case = Case(case.g, opts=_cap(60), deferred=1)
    assert all(len(b) for b in bitten(case.g, 60))
    first = Case(GroupedReads.from_groups([case.g.records(0)]), opts=_cap(60))
    want_first = want_of(first)
    cd = D.cd_types(want_first["data"])
    assert len(cd) == 2 and all(t == "c" for t, _ in cd), cd           # depths of at most 2 x 60
    check_cap(first, capped=1, want=want_first)
    c = CapCaller(**case.opts)
    try:
        got = c.device(case.g)
        assert {k: got[k] for k in PATH_KEYS} == dict(deferred=1, duplex_deep=1, big=0, deep=0, capped=1), {k: got[k] for k in PATH_KEYS}
        assert got["data"] == want_first["data"] and got["count"] == want_first["count"]
        assert_equal(c.host(case.g), want_of(case), "host entry")
    finally:
        c.close()


# ---- 10. reverse sets, the per-field writer, options -------------------------------------------------------------------------------------------------------
OPTIONS = {
    "as_it_is": dict(),
    "long_prefix": dict(read_name_prefix=b"p" * 60),                  # k_emit_duplex<0, 1>
    "per_base_tags_off": dict(produce_per_base_tags=0),
    "min_input_base_quality_30": dict(min_input_base_quality=30),
}


def check_reverse_set(name):
    _switch_is("1")
    g = two_molecules()
    cap = 4
    assert all(2 in b for b in bitten(g, cap)), set_sizes(g).tolist()           # BA-R1
    rev = [D._flag(r) & D.REVERSE for r in _records(g, 0) if _set_of(r) == 2]
    assert rev and all(rev)                                              # ... is a reverse set
    check_cap(Case(g, opts=_cap(cap, **OPTIONS[name])), capped=2)


# ---- 11. error rate 20 000 ppm under a cap of 3 ---------------------------------------------------------------------------------------------------------------
def check_error_rate():
    _switch_is("1")
    g = D.pairs(50, 2, 20000).g
    assert all(len(b) for b in bitten(g, 3))
    check_cap(Case(g, opts=_cap(3)), capped=2)


# ---- 12. the switch -----------------------------------------------------------------------------------------------------------------------------------------------
def check_switch_off(value):
    """Unset or "0": line for line the behaviour before the CAP builds — the molecules are deferred, the deep kernels decide none."""
    if value == "unset":
        os.environ.pop(SWITCH, None)                                   # (read per call: a child interpreter cannot inherit "unset")
    _switch_is(None if value == "unset" else value)
    case = Case(two_molecules(), opts=_cap(5), deferred=2)
    assert case.deep == 0
    check_cap(case, capped=0)


def check_switch_is_read_per_call(setenv, delenv):
    g = two_molecules()
    case = Case(g, opts=_cap(5))
    want = want_of(case)
    c = CapCaller(**case.opts)
    try:
        for value, on in (("1", True), ("0", False), ("1", True), (None, False), ("yes", True)):
            delenv(SWITCH) if value is None else setenv(SWITCH, value)
            got = c.device(g)
            path = {k: got[k] for k in PATH_KEYS}
            if on:
                assert path == dict(deferred=0, duplex_deep=2, big=0, deep=0, capped=2), (value, path)
                assert_equal(got, want, "device entry")
            else:
                assert path == dict(deferred=2, duplex_deep=0, big=0, deep=0, capped=0), (value, path)
    finally:
        c.close()


def check_caller_without_a_cap(setenv):
    """A caller WITHOUT a cap: the switch changes neither the launches, nor the synchronisations, nor the bytes."""
    case = D.pairs(40, 2)
    want = want_of(case)
    c = CapCaller()
    try:
        seen = {}
        c.device(case.g)                                               # (a caller's first batch uploads its table images: not part of the comparison)
        for value in ("1", "0"):
            setenv(SWITCH, value)
            got = c.device(case.g)
            assert {k: got[k] for k in PATH_KEYS} == dict(deferred=0, duplex_deep=2, big=0, deep=0, capped=0)
            assert_equal(got, want, f"device entry, switch {value}")
            seen[value] = c.chain()
        print(f"(launches, host synchronisations): {seen}", flush=True)
        assert seen["1"] == seen["0"] and seen["1"][0] > 0, seen
    finally:
        c.close()


def _setenv(k, v):
    os.environ[k] = v


def _delenv(k):
    os.environ.pop(k, None)


def check_switch_is_read_per_call_here():
    check_switch_is_read_per_call(_setenv, _delenv)


def check_caller_without_a_cap_here():
    check_caller_without_a_cap(_setenv)


# ---- 13. still deferred with the switch on -----------------------------------------------------------------------------------------------------------------------
def check_still_deferred(what):
    _switch_is("1")
    g = D._sim(3, family_size=40)
    contigs = D.methylation_contigs() if what == "methylation" else None
    opts = dict(cap_of_0=_cap(0), methylation=_cap(5, methylation_mode=1), trim=_cap(5, trim=1))[what]
    assert all(len(b) for b in bitten(g, 5))
    case = Case(g, opts=opts, deferred=3)
    assert case.deep == 0
    check_cap(case, capped=0, contigs=contigs)


# ---- 14. GPU only: fgx_run_bam on a mixed stream; guard bands --------------------------------------------------------------------------------------------------
def check_run_bam(tmp_dir):
    _switch_is("1")
    from fgumi_amd import DuplexConsensusCaller, bgzf
    case = D.mixed_stream()
    g = case.g
    assert sum(len(b) > 0 for b in bitten(g, 10)) >= 3
    want = want_of(Case(g, opts=_cap(10)))
    c = DuplexConsensusCaller("", "A", [1, 1, 0], cell_tag="CB", overlapping_consensus=True, max_reads_per_strand=10)
    refs = [("chr%d" % (i + 1), 2147483647) for i in range(24)]
    src, dst = os.path.join(tmp_dir, "grouped.bam"), os.path.join(tmp_dir, "consensus.bam")
    bgzf.write_bam(src, bgzf.grouped_input_header(refs), refs, g.blob)
    for chunk in (0, 1 << 16):
        st = c.run_bam(src, dst, chunk_raw_bytes=chunk, threads=8, strip_strand_suffix=True)
        _, _, stream, off, ln = bgzf.read_bam(dst)
        got = b"".join(bytes(stream[int(a) - 4:int(a) + int(b)]) for a, b in zip(off, ln))
        print(f"chunk {chunk}: chunks {st['chunks']}, deferred groups {st['deferred_groups']}, host entry batches {st['host_entry_batches']}", flush=True)
        assert_equal(dict(data=got, count=len(off), stats=np.array(st["stats"][:28], dtype=np.uint64)), want, f"the consensus BAM, chunk_raw_bytes {chunk}")
        assert st["deferred_groups"] == 0 and st["host_entry_batches"] == 0, (st["deferred_groups"], st["host_entry_batches"])
    c.close()


def check_under_guard_bands():
    """(child interpreter, FGX_GUARD_BAND set) one strand capped, the other not — the walk-order rows, and col_obs_all over a deep molecule's columns by the
    count-only pass and by the copy —, then a look at every guarded buffer."""
    import ctypes as C
    from fgumi_amd import lib
    lib.fgx_debug_check_guard_bands.restype = C.c_int
    lib.fgx_debug_check_guard_bands.argtypes = [C.c_char_p, C.c_int]
    check_one_strand_capped(None)
    msg = C.create_string_buffer(600)
    bad = lib.fgx_debug_check_guard_bands(msg, 600)
    assert bad == 0, f"capped deep duplex molecules: {bad} device buffer(s) written outside their bounds: {msg.value.decode()}"
