"""Inputs and the runners of the deep-indel tests (tests/test_canon_deep_core.py and tests/test_wavemu_deep_indels.py on the CPU, tests/test_gpu_deep_indels.py on
the GPU): duplex molecules of 65 .. 512 records whose reads carry indel / skip / pad / clip CIGARs.  With FGX_DEEP_INDELS=1 k_canon_duplex_deep
(fgumi_amd/csrc/canon_deep.inc) rewrites them into their canonical form — byte for byte what the scalar form at 512 records (fgx_canon_duplex_deep_host) computes — and
the deep duplex kernels decide them in the canonical second pass.

The molecules scale tests/test_canon_core.py's record maker and CIGAR tables to k pairs per strand over one template: a majority CIGAR pair and minority reads.  A case is
the molecule's records, the caller's options, and what is claimed of it: in scope or not (checked against the scalar form's status), and how many records the canonical
molecule keeps — above 64 the second pass's deep kernels decide it (fgx_debug_last_deep_indels counts it), up to 64 its k_family_wave<1>."""
import ctypes as C
import dataclasses
import os
import random

import numpy as np

import bamutil
import fgx_opts
import orc
from test_canon_core import C1, C2, TMPL, qlen, rlen

EMULATED = "FGX_LIB" in os.environ


# ---- the record maker (test_canon_core.duplex_indel_molecule's, one template at a time) ---------------------------------------------------------------------------
def template(rng, g, strand, k, cigars, start, insert, mc=True, flat_q=None, low_tail=0, cb=None, name=None, err=0.03, mi=None):
    """Both records of one template: the forward read at `start` with cigars[0], the reverse read ending at start + insert with cigars[1]; /B templates have the
    reverse read as R1.  (Names of eleven characters: the deep kernels pair mates by a 30-bit name hash and defer a molecule two of whose names collide in it, which
    names of four to six characters that differ in their digits do.)  flat_q: every quality that value (disagreeing mates then have equal qualities); low_tail: that many bases at the 3' end of both reads get
    quality 2 (the final length shrinks: the simplified CIGAR becomes a prefix); cb: a CB tag; mi: the MI value when it is not `g`."""
    c1, c2 = cigars
    p2 = start + insert - rlen(c2)

    def seq(p, L):
        return "".join(rng.choice("ACGTN") if rng.random() < err else TMPL[(p + i) % 4000] for i in range(L))
    s1, s2 = seq(start, qlen(c1)), seq(p2, qlen(c2))
    q1 = [flat_q if flat_q is not None else rng.choice([5, 12, 25, 30, 37]) for _ in s1]
    q2 = [flat_q if flat_q is not None else rng.choice([5, 12, 25, 30, 37]) for _ in s2]
    for i in range(low_tail):
        q1[len(q1) - 1 - i] = 2          # the forward read's 3' end is its stored tail
        q2[i] = 2                        # the reverse read's is its stored head
    rx = "ACG-TTA" if strand == "A" else "TTA-ACG"
    fwd = dict(flag=0x1 | 0x2 | 0x20, pos=start, mate_pos=p2)
    rev = dict(flag=0x1 | 0x2 | 0x10, pos=p2, mate_pos=start)
    first, last = (fwd, rev) if strand == "A" else (rev, fwd)
    recs = []
    for seg, d in ((0x40, first), (0x80, last)):
        is_fwd = d is fwd
        s, q, c, mcv = (s1, q1, c1, c2) if is_fwd else (s2, q2, c2, c1)
        tags = [("MI", "Z", f"{g if mi is None else mi}/{strand}"), ("RX", "Z", rx)] + ([("MC", "Z", mcv)] if mc else []) + ([("CB", "Z", cb)] if cb else [])
        recs.append(bamutil.make_record(name or f"mol{g}:{strand}:{k:04d}", s, q, flag=d["flag"] | seg, ref_id=0, pos=d["pos"], cigar=c, mate_ref=0, mate_pos=d["mate_pos"],
                                        tlen=insert if is_fwd else -insert, tags=tags))
    return recs


def molecule(seed, n_a, n_b, major=1, minority=(), g=7, insert=140, start=500, table=None, **kw):
    """n_a /A templates then n_b /B templates with the CIGAR pair table[major]; minority: {template index (over A then B): table index}."""
    rng = random.Random(seed)
    table = table or list(zip(C1, C2))
    minority = dict(minority)
    recs = []
    for t in range(n_a + n_b):
        strand, k = ("A", t) if t < n_a else ("B", t - n_a)
        recs += template(rng, g, strand, k, table[minority.get(t, major)], start, insert, **kw)
    return recs


@dataclasses.dataclass
class Case:
    recs: list
    opts: dict = dataclasses.field(default_factory=dict)
    in_scope: bool = True
    dropped: int = -1          # reads the alignment filter drops (-1: not claimed)
    note: str = ""


DEL = 1            # 40M2D60M / 60M2D40M
INS = 3            # 40M3I57M / 57M3I40M
CLIP_DEL = 5       # 5S35M2D60M / 60M2D35M5S
LATE_DEL = 11      # 39M3D61M / 100M
DEEP_ERR = 0.002   # share of wrong bases in the reads of the molecules of 128 records and more


def sized(n_records):
    """One alignment group over n_records records, half of them on each strand (an odd template count gives /A one more).  (The deeper the molecule, the fewer wrong
    bases a read gets: a molecule most of whose columns disagree overflows its list of the k_call_full pool in a batch this small, and the deep kernels then defer it —
    their rule, which this path does not change.)"""
    t = n_records // 2
    return Case(molecule(100 + n_records, t - t // 2, t // 2, major=DEL, err=DEEP_ERR if n_records > 100 else 0.03), dropped=0)


def size_512():
    """256 templates: a record side holds 256 reads, one more than the deep kernels keep — one minority template leaves 255 survivors a side."""
    return Case(molecule(612, 128, 128, major=DEL, minority={5: INS}, err=DEEP_ERR), dropped=2)


def size_514():
    return Case(molecule(614, 129, 128, major=DEL, err=DEEP_ERR), in_scope=False)


def two_equal_groups(smaller_first):
    """Two groups of 17 + 17 reads per record side: the sizes tie, simp_cmp decides.  The reads of both groups have the same final length, so the first group is the one
    of the first template: smaller_first puts the smaller CIGAR (39M3D.. < 40M2D..) there, else the later group holds it; either way the other 34 records go."""
    a, b = (LATE_DEL, DEL) if smaller_first else (DEL, LATE_DEL)
    minority = {t: b for t in range(34) if t % 2 == 1}
    return Case(molecule(71 + smaller_first, 20, 14, major=a, minority=minority), dropped=34)


def many_groups(n_groups):
    """n_groups alignments on the forward reads' record side (16 are in scope, a 17th is not); the reverse reads all carry 100M."""
    table = [(f"{20 + 3 * i}M1D{80 - 3 * i}M", "100M") for i in range(17)]
    minority = {t: (t % n_groups) for t in range(40)}
    c = Case(molecule(160 + n_groups, 22, 18, major=0, minority=minority, table=table), in_scope=n_groups <= 16)
    if c.in_scope:
        sizes = [sum(1 for t in range(40) if t % n_groups == i) for i in range(n_groups)]
        c.dropped = 40 - max(sizes)                     # (the groups of the forward reads' side tie in size at 16: simp_cmp picks among them)
    return c


def prefixes():
    """Reads whose 3' ends are masked away (quality 2 under min-input-base-quality 10): shorter, and prefixes of the representative."""
    rng = random.Random(5)
    recs = []
    for t in range(36):
        strand, k = ("A", t) if t < 20 else ("B", t - 20)
        recs += template(rng, 7, strand, k, (C1[DEL], C2[DEL]), 500, 140, low_tail=(t * 7) % 45)
    return Case(recs, dropped=0)


def reverse_r1_only():
    """Only /B templates: every R1 is a reverse read."""
    return Case(molecule(9, 0, 35, major=DEL, err=0.01), dropped=0)


def insertion_against_deletion():
    """The forward mate carries an insertion, the reverse mate a deletion, and they overlap by 60 reference positions."""
    table = [("40M3I57M", "60M2D40M")]
    return Case(molecule(12, 18, 17, major=0, table=table), dropped=0)


def nibble_hazard(insert):
    """Odd read lengths; soft clips and the insert size move the shared window's first query offset to odd and even values in either mate."""
    table = [("40M2D59M", "61M2D40M"), ("3S40M2D56M", "61M2D37M3S"), ("4S41M1I53M", "99M")]
    minority = {t: 1 + t % 2 for t in range(0, 35, 5)}
    return Case(molecule(insert, 18, 17, major=0, minority=minority, table=table, insert=insert))


def equal_quality_disagreements():
    """Every quality 30 and one base in eight wrong: mates that disagree do so at equal quality -> N, quality 2."""
    return Case(molecule(14, 17, 17, major=DEL, flat_q=30, err=0.12, insert=120), dropped=0)


def three_records_of_a_name():
    """A third record of one name, a FIRST one, behind the template: the scalar form pairs the LAST record with FIRST and the last without."""
    recs = molecule(15, 17, 17, major=DEL)
    extra = template(random.Random(16), 7, "A", 99, (C1[DEL], C2[DEL]), 500, 140, name="mol7:A:0003")
    return Case(recs + extra[:1] + template(random.Random(17), 7, "A", 98, (C1[DEL], C2[DEL]), 500, 140))


def drops_to_64():
    """66 records of which the filter drops two templates: the canonical molecule has 62 records, k_family_wave<1> of the second pass decides it."""
    return Case(molecule(18, 17, 16, major=DEL, minority={3: INS, 20: INS}), dropped=4)


def first_record_dropped(same_cb):
    """The first /A template is a minority one, so the cell barcode is read from its successor: in scope iff that one carries the same value."""
    rng = random.Random(19)
    recs = []
    for t in range(34):
        strand, k = ("A", t) if t < 17 else ("B", t - 17)
        cb = "ACGT" if (t != 0 or same_cb) else "TTTT"
        recs += template(rng, 7, strand, k, (C1[INS], C2[INS]) if t == 0 else (C1[DEL], C2[DEL]), 500, 140, cb=cb)
    return Case(recs, in_scope=bool(same_cb), dropped=2 if same_cb else -1)


def drops_break_the_gate():
    """Two /B templates with a minority alignment: the filter drops them, the survivors fail min-reads 2 1 1 — the molecule stays where it is."""
    return Case(molecule(20, 33, 2, major=DEL, minority={33: INS, 34: INS}), opts=dict(duplex_min_reads=(2, 1, 1)), in_scope=False)


def biting_cap():
    return Case(molecule(21, 17, 16, major=DEL), opts=dict(duplex_max_reads_per_strand=10), in_scope=False)


def strand_collision():
    """One /A template relabelled /B: its reverse R2 lies on the record side of the /B strand's forward R2s."""
    recs = [bytearray(r) for r in molecule(22, 17, 16, major=DEL)]
    for r in recs[0:2]:
        i = bytes(r).index(b"MIZ7/A")
        r[i + 5] = ord("B")
    return Case([bytes(r) for r in recs], in_scope=False)


def missing_mc():
    """No MC tag on any record: no mate clip."""
    return Case(molecule(23, 17, 17, major=DEL, mc=False, insert=110), dropped=0)


CASES = {
    "66_records": lambda: sized(66), "128_records": lambda: sized(128), "130_records": lambda: sized(130), "510_records": lambda: sized(510), "512_records": size_512,
    "514_records": size_514,
    "two_equal_groups_smaller_first": lambda: two_equal_groups(1), "two_equal_groups_smaller_later": lambda: two_equal_groups(0),
    "16_groups": lambda: many_groups(16), "17_groups": lambda: many_groups(17),
    "prefixes": prefixes, "reverse_r1s": reverse_r1_only, "insertion_against_deletion": insertion_against_deletion,
    "nibbles_insert_141": lambda: nibble_hazard(141), "nibbles_insert_150": lambda: nibble_hazard(150),
    "equal_quality_disagreements": equal_quality_disagreements, "three_records_of_a_name": three_records_of_a_name, "drops_to_64": drops_to_64,
    "first_record_dropped_same_cb": lambda: first_record_dropped(1), "first_record_dropped_other_cb": lambda: first_record_dropped(0),
    "drops_break_the_gate": drops_break_the_gate, "biting_cap": biting_cap, "strand_collision": strand_collision, "missing_mc": missing_mc,
}
# the option sets of tests/test_gpu_duplex_canon.py
OPTION_SETS = [(dict(overlapping_consensus=1), (1, 1, 0)), (dict(overlapping_consensus=0, min_input_base_quality=20), (2, 1, 1)),
               (dict(overlapping_consensus=1, cell_tag=b"\0\0", produce_per_base_tags=0), (1, 1, 1))]


def options_of(case, **more):
    kw = dict(case.opts, **more)
    mr = kw.pop("duplex_min_reads", None)
    o = fgx_opts.defaults(kind=1, **kw)
    if mr:
        o.duplex_min_reads[0], o.duplex_min_reads[1], o.duplex_min_reads[2] = mr
    return o


def with_option_set(case, i):
    kw, mr = OPTION_SETS[i]
    return dataclasses.replace(case, opts=dict(case.opts, duplex_min_reads=mr, **kw), dropped=-1)


# ---- the canonical form: scalar hooks and the kernel's test entry ------------------------------------------------------------------------------------------------
def grouped(recs):
    from fgumi_amd import GroupedReads
    return GroupedReads.from_groups([[bytes(r) for r in recs]])


def canonical(o, recs, entry="fgx_canon_duplex_deep_host"):
    """dict(status, out_len, bodies — the bytes of `out` at every record's offset, prefix included —, delta) of one molecule through `entry`."""
    from fgumi_amd._lib import lib
    g = grouped(recs)
    out = np.zeros(g.blob.size + 16, dtype=np.uint8)
    out_len = np.zeros(max(1, g.n_rec), dtype=np.uint32)
    delta = np.zeros(5, dtype=np.uint64)
    if entry == "fgx_debug_canon_duplex_deep_device":
        st = C.c_int(-1)
        rc = lib.fgx_debug_canon_duplex_deep_device(C.addressof(o), g.blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, out.ctypes.data,
                                                    out_len.ctypes.data, delta.ctypes.data, C.byref(st))
        assert rc == 0, rc
        status = st.value
    else:
        status = getattr(lib, entry)(C.addressof(o), g.blob.ctypes.data, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, out.ctypes.data, out_len.ctypes.data,
                                     delta.ctypes.data)
    recs_out = [bytes(out[int(g.rec_off[i]):int(g.rec_off[i]) + int(out_len[i])]) for i in range(g.n_rec)]
    prefixes = [int(out[int(g.rec_off[i]) - 4:int(g.rec_off[i])].view(np.uint32)[0]) for i in range(g.n_rec)]
    return dict(status=int(status), out_len=out_len.tolist(), recs=recs_out, prefixes=prefixes, delta=delta.tolist())


def check_kernel_against_scalar(case, o=None):
    """k_canon_duplex_deep against the scalar form at 512 records: the status always; in scope also delta, lengths, every byte of every kept record and its prefix."""
    o = o or options_of(case)
    want = canonical(o, case.recs)
    got = canonical(o, case.recs, "fgx_debug_canon_duplex_deep_device")
    print(f"scalar status {want['status']}, delta {want['delta']}, kept {sum(1 for n in want['out_len'] if n)} of {len(case.recs)}", flush=True)
    assert want["status"] == (0 if case.in_scope else 1), ("the case's own claim", want["status"], case.note)
    assert got["status"] == want["status"], (got["status"], want["status"])
    if want["status"] != 0:
        return want
    if case.dropped >= 0:
        assert want["delta"][0] == case.dropped, (want["delta"], case.dropped)
    assert got["delta"] == want["delta"], (got["delta"], want["delta"])
    assert got["out_len"] == want["out_len"]
    for i, (a, b) in enumerate(zip(got["recs"], want["recs"])):
        assert a == b, f"record {i} differs:\n got {bamutil.parse(a)}\nwant {bamutil.parse(b)}"
    assert [p for p, n in zip(got["prefixes"], want["out_len"]) if n] == [n for n in want["out_len"] if n]
    return want


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------------------------
def want_of(o, g):
    return orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=100)


class Caller:
    """A duplex caller of the library under test: both entries over one batch and the path the last batch took."""

    def __init__(self, o):
        from fgumi_amd._lib import Options, lib
        self.lib = lib
        po = Options.from_buffer_copy(bytes(o))
        self.h = lib.fgx_create(C.byref(po))
        assert self.h, lib.fgx_global_error().decode()
        lib.fgx_debug_last_chain.restype = None
        lib.fgx_debug_last_chain.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]

    def close(self):
        if self.h:
            self.lib.fgx_destroy(self.h)
            self.h = None

    def path(self):
        d = (C.c_uint64 * 2)()
        self.lib.fgx_debug_last_deferral(self.h, d)
        return dict(canon=int(d[1]), deep_indels=int(self.lib.fgx_debug_last_deep_indels(self.h)), duplex_deep=int(self.lib.fgx_debug_last_duplex_deep(self.h)))

    def chain(self):
        ch = (C.c_uint32 * 2)()
        self.lib.fgx_debug_last_chain(self.h, ch)
        return int(ch[0]), int(ch[1])

    def device(self, g):
        from fgumi_amd._lib import Output
        lib = self.lib
        out, nd, dp = Output(), C.c_uint32(), C.c_void_p()
        if EMULATED:
            blob = np.concatenate([g.blob, np.zeros(64, dtype=np.uint8)])
            keep = (blob, g.rec_off, g.rec_len, g.grp_first)
            ptrs = (blob.ctypes.data, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.grp_first.ctypes.data)
        else:
            import torch
            dg = g.to_device()
            torch.cuda.synchronize(dg.blob.device)
            keep = dg
            ptrs = (dg.blob.data_ptr(), dg.rec_off.data_ptr(), dg.rec_len.data_ptr(), dg.grp_first.data_ptr())
        rc = lib.fgx_process_batch_device(self.h, ptrs[0], g.blob.size, ptrs[1], ptrs[2], g.n_rec, ptrs[3], g.n_grp, C.byref(out), C.byref(nd), C.byref(dp))
        assert rc == 0, lib.fgx_last_error(self.h).decode()
        if not out.data_len:
            data = b""
        elif EMULATED:
            data = C.string_at(out.data, out.data_len)
        else:
            from fgumi_amd._lib import hip_memcpy_d2h
            data = hip_memcpy_d2h(out.data, out.data_len)
        del keep
        return dict(data=data, count=int(out.count), stats=np.array([int(v) for v in out.stats], dtype=np.uint64), deferred=int(nd.value), **self.path())

    def host(self, g):
        from fgumi_amd._lib import Output
        lib = self.lib
        out = Output()
        rc = lib.fgx_process_batch(self.h, g.blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, g.grp_first.ctypes.data, g.n_grp, C.byref(out))
        assert rc == 0, lib.fgx_last_error(self.h).decode()
        data = C.string_at(out.data, out.data_len) if out.data_len else b""
        return dict(data=data, count=int(out.count), stats=np.array([int(v) for v in out.stats], dtype=np.uint64), **self.path())


def assert_equal(got, want, what):
    from fgumi_amd import split_records
    if got["data"] != want["data"]:
        for i, (a, b) in enumerate(zip(split_records(got["data"]), split_records(want["data"]))):
            if a != b:
                raise AssertionError(f"{what}: record {i} differs:\n got {bamutil.parse(a)}\nwant {bamutil.parse(b)}")
        raise AssertionError(f"{what}: record count / length differs")
    assert got["count"] == want["count"], (what, got["count"], want["count"])
    assert np.array_equal(got["stats"], want["stats"]), (what, got["stats"].tolist(), want["stats"].tolist())


def check_end_to_end(case, o=None, kept=None):
    """FGX_DEEP_INDELS=1 (set by the test): both entries against the oracle — bytes, count, all 28 counters — and the path: an in-scope molecule is not deferred, is
    counted into the canonical molecules, and into fgx_debug_last_deep_indels iff its canonical form keeps more than 64 records; one out of scope stays deferred."""
    assert os.environ.get("FGX_DEEP_INDELS") == "1"
    o = o or options_of(case)
    g = grouped(case.recs)
    want = want_of(o, g)
    if kept is None:
        sc = canonical(o, case.recs)
        assert sc["status"] == (0 if case.in_scope else 1), sc["status"]
        kept = sum(1 for n in sc["out_len"] if n)
    indels = 1 if case.in_scope and kept > 64 else 0
    c = Caller(o)
    try:
        got = c.device(g)
        path = {k: got[k] for k in ("deferred", "canon", "deep_indels", "duplex_deep")}
        print(f"device entry {path}; canonical records {kept}", flush=True)
        assert got["duplex_deep"] == 0, path
        if case.in_scope:
            assert got["deferred"] == 0 and got["canon"] == 1 and got["deep_indels"] == indels, path
            assert_equal(got, want, "device entry")
        else:
            assert got["deferred"] == 1 and got["deep_indels"] == 0, path
        hg = c.host(g)
        assert hg["deep_indels"] == indels and hg["canon"] == (1 if case.in_scope else 0), {k: hg[k] for k in ("canon", "deep_indels")}
        assert_equal(hg, want, "host entry")
    finally:
        c.close()
