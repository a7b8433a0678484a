"""Inputs and the runner of the deep CODEC tests (tests/test_wavemu_codec_deep.py on the CPU, tests/test_gpu_codec_deep.py on the GPU): CODEC molecules of
more than 64 records, which k_family_wave<2> defers and the streaming kernels of fgumi_amd/csrc/codec_deep.inc decide up to 254 records under
FGX_CODEC_DEEP=1.  Every batch is built once from the simulator's CODEC molecules (`family_size=N, codec=1` gives a molecule of N templates = 2 N records,
mates adjacent, every template at the molecule's position), cut to size with GroupedReads.from_groups or changed in place, and says EXACTLY how many of its
molecules the new kernels decide and how many the device entry defers: a test that tolerated "some deferred" would hide a path that never ran."""
import ctypes as C
import dataclasses
import os

import numpy as np

import duplex_deep_cases as DD
import fgx_opts
import orc
from duplex_deep_cases import _flag, _groups, _set_flag, _tag_value, _with_cigar
from max_reads_cases import READ_THROUGH
from wide_cases import _rx_value, assert_equal, records_per_family, with_low_qualities

EMULATED = DD.EMULATED
# FGX_REJ_* (include/fgumi_amd.h)
REJ_INSUFFICIENT_READS, REJ_INSUFFICIENT_OVERLAP, REJ_INDEL_ERROR, REJ_CLIP_OVERLAP_FAILED, REJ_NOT_PRIMARY_FR_PAIR, REJ_DOWNSAMPLED = 1, 12, 14, 15, 18, 19
PAIRED, PROPER, UNMAPPED, MATE_UNMAPPED, REVERSE, MATE_REVERSE, FIRST, LAST, SECONDARY = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80, 0x100
SIM = dict(insert_mean=200, insert_sd=30)                        # 150-base reads: the two strands share about 100 positions


@dataclasses.dataclass
class Case:
    g: object                  # GroupedReads
    opts: dict = dataclasses.field(default_factory=dict)
    deferred: int = 0          # molecules the device entry defers
    deep: int = -1             # molecules the new kernels decide; -1: every molecule of more than 64 records that is not deferred
    capped: int = 0            # ... of which the cap dropped a read

    def __post_init__(self):
        if self.deep < 0:
            self.deep = int((records_per_family(self.g) > 64).sum()) - self.deferred


def _sim(n, **kw):
    from fgumi_amd import simulate_grouped_reads
    return simulate_grouped_reads(n, codec=1, **dict(SIM, **kw))


def _recs(g, gi):
    return [bytearray(r) for r in g.records(gi)]


def _i32(rec, o):
    return int.from_bytes(rec[o:o + 4], "little", signed=True)


def _put_i32(rec, o, v):
    rec[o:o + 4] = int(v).to_bytes(4, "little", signed=True)


def _move(pair, fwd_pos=None, rev_pos=None):
    """The template's forward / reverse mate moved to a 0-based position in place, each mate's mate-position field with it."""
    f, r = (pair[0], pair[1]) if not (_flag(pair[0]) & REVERSE) else (pair[1], pair[0])
    assert not (_flag(f) & REVERSE) and (_flag(r) & REVERSE)
    if fwd_pos is not None:
        _put_i32(f, 4, fwd_pos); _put_i32(r, 24, fwd_pos)
    if rev_pos is not None:
        _put_i32(r, 4, rev_pos); _put_i32(f, 24, rev_pos)


def _with_l_seq(rec, n):
    """The record cut to its first n bases: SEQ, QUAL and the one CIGAR op."""
    l_name, n_cig, l_seq = rec[8], rec[12] | (rec[13] << 8), int.from_bytes(rec[16:20], "little")
    assert n_cig == 1 and n <= l_seq
    s0 = 32 + l_name + 4
    q0 = s0 + (l_seq + 1) // 2
    seq = bytearray(rec[s0:s0 + (n + 1) // 2])
    if n & 1:
        seq[-1] &= 0xF0
    out = bytearray(rec[:s0]) + seq + bytearray(rec[q0:q0 + n]) + bytearray(rec[q0 + l_seq:])
    out[16:20] = n.to_bytes(4, "little")
    out[32 + l_name:32 + l_name + 4] = ((n << 4) | (rec[32 + l_name] & 15)).to_bytes(4, "little")
    return out


def _seq_qual(rec):
    l_name, n_cig, l_seq = rec[8], rec[12] | (rec[13] << 8), int.from_bytes(rec[16:20], "little")
    s0 = 32 + l_name + 4 * n_cig
    return s0, s0 + (l_seq + 1) // 2, l_seq


def _set_base(rec, i, code):
    s0, _, _ = _seq_qual(rec)
    b = rec[s0 + (i >> 1)]
    rec[s0 + (i >> 1)] = (b & 0x0F) | (code << 4) if not (i & 1) else (b & 0xF0) | code


# ---- 1 / 2. the lower edge (32 pairs are k_family_wave's, 33 pairs the new kernels') and the edge between the record kernel's two builds ------------------
def lower_edge():
    g = _sim(2, family_size=33)
    return Case(_groups([g.records(0)[:64], g.records(1)]))


def build_edge():
    g = _sim(2, family_size=65)
    c = Case(_groups([g.records(0)[:128], g.records(1)]))
    assert records_per_family(c.g).tolist() == [128, 130] and c.deep == 2
    return c


# ---- 3. integer tag types: cD is type c up to 127 and type C above ------------------------------------------------------------------------------------------
def pairs(n_pairs, n_molecules=1, err=1000, **opts):
    return Case(_sim(n_molecules, family_size=n_pairs, error_rate_ppm=err), opts=opts)


cd_types = DD.cd_types


# ---- 4. the bound: 127 pairs are decided, 128 pairs are deferred ----------------------------------------------------------------------------------------
def the_bound():
    g = _sim(2, family_size=128)
    c = Case(_groups([g.records(0)[:254], g.records(1)]), deferred=1)
    assert records_per_family(c.g).tolist() == [254, 256] and c.deep == 1
    return c


# ---- 6. the long tail and its option matrix ---------------------------------------------------------------------------------------------------------------
def long_tail(n=3, **sim):
    g = _sim(n, **dict(dict(family_size=40, family_size_max=120), **sim))
    assert records_per_family(g).min() >= 80 and records_per_family(g).max() <= 240
    return g


def poor_3prime_ends(g):
    """Every third record ends (in sequencing order: the 3' end of a reverse read is the start of SEQ) in ten bases that are N or of quality 2 — a CODEC
    source read keeps them: no trailing-N strip, no mask."""
    blob = np.array(g.blob, copy=True)
    for k, o in enumerate(np.asarray(g.rec_off, dtype=np.int64)[::3]):
        o = int(o)
        rec = bytearray(blob[o:o + 4096].tobytes())
        s0, q0, l_seq = _seq_qual(rec)
        rev = bool(_flag(rec) & REVERSE)
        for i in (range(10) if rev else range(l_seq - 10, l_seq)):
            if k & 1:
                _set_base(rec, i, 15)
            rec[q0 + i] = 2
        blob[o:o + q0 + l_seq] = np.frombuffer(bytes(rec[:q0 + l_seq]), dtype=np.uint8)
    return dataclasses.replace(g, blob=blob)


OPTION_MATRIX = {
    "per_base_tags_on": dict(produce_per_base_tags=1),
    "per_base_tags_off": dict(produce_per_base_tags=0),
    "cell_tag_off": dict(cell_tag=b"\0\0"),
    "min_reads_per_strand_1": dict(codec_min_reads_per_strand=1),
    "min_reads_per_strand_3": dict(codec_min_reads_per_strand=3),
    "min_reads_above_the_molecule": dict(codec_min_reads_per_strand=200),
    "min_duplex_length_above_the_overlap": dict(codec_min_duplex_length=500),
    "outer_bases_and_single_strand_masks": dict(codec_has_outer_bases_qual=1, codec_outer_bases_qual=5, codec_outer_bases_length=7, codec_has_single_strand_qual=1,
                                                codec_single_strand_qual=9),
    "min_input_base_quality_30": dict(min_input_base_quality=30),     # with low qualities in the reads: the oracle does not mask a CODEC source read
    "poor_3prime_ends": dict(),
    "long_prefix": dict(read_name_prefix=b"p" * 60),                  # the per-field record writer
}
OPTION_COUNTER = {"min_reads_above_the_molecule": REJ_INSUFFICIENT_READS, "min_duplex_length_above_the_overlap": REJ_INSUFFICIENT_OVERLAP}


def option_case(name):
    g = long_tail()
    if name == "min_input_base_quality_30":
        g = with_low_qualities(g)
    if name == "poor_3prime_ends":
        g = poor_3prime_ends(g)
    return Case(g, opts=OPTION_MATRIX[name])


# ---- 7. geometry --------------------------------------------------------------------------------------------------------------------------------------------
def read_through():
    return Case(long_tail(**READ_THROUGH))


def deepest_clip():
    """Every reverse mate moved (in place) so that it ends one base behind its forward mate's start: the forward reads keep two bases, the least the overlap
    clip leaves of an FR pair (a forward read that starts at or behind its mate's last base is not FR) — "clipped to nothing" does not exist for this shape."""
    recs = _recs(_sim(1, family_size=40), 0)
    for t in range(0, len(recs), 2):
        f = recs[t] if not (_flag(recs[t]) & REVERSE) else recs[t + 1]
        _move(recs[t:t + 2], rev_pos=_i32(f, 4) + 2 - 150)
    return Case(_groups([recs]))


def abutting_strands():
    """IndelErrorBetweenStrands, crafted by moving `pos` in place (the simulator's strands always overlap): every reverse mate starts right behind its
    forward mate's end, so the overlap window is empty — with --min-duplex-length 0 it passes that gate, and the read positions at its two ends are
    htsjdk's out-of-range 0 on one strand each."""
    recs = _recs(_sim(1, family_size=40), 0)
    for t in range(0, len(recs), 2):
        f = recs[t] if not (_flag(recs[t]) & REVERSE) else recs[t + 1]
        _move(recs[t:t + 2], rev_pos=_i32(f, 4) + 150)
    return Case(_groups([recs]), opts=dict(codec_min_duplex_length=0))


def clip_overlap_failed():
    """ClipOverlapFailed, crafted by cutting the reverse mates to 100 bases and moving `pos` in place: in the first template the reverse mate lies inside the
    forward one (which is clipped to 110 bases), in the others it ends with it (150 and 100 bases) — the longest forward read is a later template's, the
    longest reverse read the first template's, and that one ends 40 bases ahead of the forward read: the consensus would be shorter than a strand."""
    recs = _recs(_sim(1, family_size=40), 0)
    out = []
    for t in range(0, len(recs), 2):
        f, r = (recs[t], recs[t + 1]) if not (_flag(recs[t]) & REVERSE) else (recs[t + 1], recs[t])
        r = _with_l_seq(r, 100)
        pair = [f, r] if f is recs[t] else [r, f]
        _move(pair, rev_pos=_i32(f, 4) + (10 if t == 0 else 50))
        out += pair
    return Case(_groups([out]))


# ---- 8. templates ------------------------------------------------------------------------------------------------------------------------------------------------
def _not_fr(pair, how):
    if how == 0:                                                   # MATE_UNMAPPED on both mates
        for r in pair:
            _set_flag(r, _flag(r) | MATE_UNMAPPED)
    else:                                                          # both mates on the forward strand
        for r in pair:
            _set_flag(r, _flag(r) & ~(REVERSE | MATE_REVERSE))


def some_templates_not_fr():
    recs = _recs(_sim(1, family_size=50), 0)
    for k, t in enumerate(range(6, 100, 14)):
        _not_fr(recs[t:t + 2], k & 1)
    return Case(_groups([recs]))


def one_fr_template(iupac=False):
    """All templates but one are not FR: sets of one read, the single-read table.  `iupac`: an IUPAC code in that lone read — the general path's."""
    recs = _recs(_sim(1, family_size=40), 0)
    for k, t in enumerate(range(0, 80, 2)):
        if t != 30:
            _not_fr(recs[t:t + 2], k & 1)
    if iupac:
        _set_base(recs[30], 20, 3)                                 # M = A or C
    return Case(_groups([recs]), deferred=1 if iupac else 0)


# ---- 9. not this path's ---------------------------------------------------------------------------------------------------------------------------------
NOT_THIS_PATH = ("deletion", "soft_clip", "secondary", "fragment", "mates_not_adjacent", "three_records_with_one_name", "both_mates_first", "unequal_read_lengths")


def not_this_path(what):
    recs = _recs(_sim(1, family_size=40), 0)
    r = recs[10]
    l_seq = int.from_bytes(r[16:20], "little")
    if what == "deletion":
        recs[10] = _with_cigar(r, [(40 << 4) | 0, (2 << 4) | 2, ((l_seq - 40) << 4) | 0])
    elif what == "soft_clip":
        recs[10] = _with_cigar(r, [(5 << 4) | 4, ((l_seq - 5) << 4) | 0])
    elif what == "secondary":
        _set_flag(r, _flag(r) | SECONDARY)
    elif what == "fragment":
        for r in recs[10:12]:
            _set_flag(r, _flag(r) & ~(PAIRED | PROPER | MATE_UNMAPPED | MATE_REVERSE | FIRST | LAST))
    elif what == "mates_not_adjacent":
        recs[11], recs[12] = recs[12], recs[11]
    elif what == "three_records_with_one_name":
        a, b = recs[10], recs[12]
        assert a[8] == b[8]
        b[32:32 + b[8]] = a[32:32 + a[8]]
    elif what == "both_mates_first":
        for r in recs[10:12]:
            _set_flag(r, (_flag(r) | FIRST) & ~LAST)
    else:
        k = 10 if _flag(recs[10]) & FIRST else 11
        recs[k] = _with_l_seq(recs[k], l_seq - 10)
    return Case(_groups([recs]), deferred=1)


# ---- 10. UMIs ----------------------------------------------------------------------------------------------------------------------------------------------------
def umi_disagreement():
    """More than 100 records, every third template's RX changed in its first character: a UMI character through the likelihoods (and k_call_full)."""
    recs = _recs(_sim(1, family_size=100, error_rate_ppm=2000), 0)
    for t in range(0, 100, 3):
        for r in recs[2 * t:2 * t + 2]:
            o, ln = _rx_value(r)
            r[o] = ord("C") if r[o] == ord("A") else ord("A")
    return Case(_groups([recs]))


def _without_rx(r):
    o, ln = _rx_value(r)
    return r[:o - 3] + r[o + ln + 1:]


def no_rx():
    return Case(_groups([[_without_rx(r) for r in _recs(_sim(1, family_size=50), 0)]]))


def rx_on_some_records():
    recs = _recs(_sim(1, family_size=50), 0)
    return Case(_groups([[r if k % 5 in (1, 3) else _without_rx(r) for k, r in enumerate(recs)]]))


def umi_of_unequal_length():
    """A molecule one of whose reads carries an RX one character shorter (the general path's: the reference refuses it) beside a molecule as it came."""
    g = _sim(2, family_size=50)
    m0 = _recs(g, 0)
    o, ln = _rx_value(m0[20])
    del m0[20][o + ln - 1]
    return Case(_groups([m0, g.records(1)]), deferred=1)


def cell_barcode_only_on_an_r2():
    """No record but one R2 carries the cell barcode: "first record, R1s then R2s, that carries a non-empty value"."""
    recs = _recs(_sim(1, family_size=40), 0)
    k = 31 if not (_flag(recs[31]) & FIRST) else 30
    recs[k] = recs[k] + bytearray(b"CBZACGTTGCA\0")
    return Case(_groups([recs]))


# ---- 11. --max-reads-per-strand ---------------------------------------------------------------------------------------------------------------------------
def cap(n_pairs, cap, n_molecules=2):
    bites = 0 <= cap < n_pairs
    return Case(_sim(n_molecules, family_size=n_pairs, error_rate_ppm=5000), opts=dict(codec_max_reads_per_strand=cap), capped=n_molecules if bites and cap > 0 else 0)


# ---- 12. options that keep the path off ---------------------------------------------------------------------------------------------------------------------
def path_off_case(what):
    g = _sim(3, family_size=40)
    return Case(g, opts=dict(trim=dict(trim=1), rejects=dict(track_rejects=1))[what], deferred=3)


# ---- 13 / 14. a shallow batch; a mixed stream -----------------------------------------------------------------------------------------------------------------
def shallow():
    return Case(_sim(300, family_size=6))


def mixed_stream():
    small = _sim(1000, family_size=1, family_size_max=5, error_rate_ppm=5000)
    big = _sim(3, family_size=127, seed=7, error_rate_ppm=5000)
    deep = [big.records(0)[:66], big.records(1)[:180], big.records(2)]       # 66, 180 and 254 records
    groups = [small.records(i) for i in range(500)] + deep + [small.records(i) for i in range(500, 1000)]
    c = Case(_groups(groups))
    assert sorted(records_per_family(c.g).tolist())[-3:] == [66, 180, 254] and c.deep == 3
    return c


# ---- the runner -----------------------------------------------------------------------------------------------------------------------------------------
def options_of(case, **more):
    return fgx_opts.defaults(kind=2, **dict(dict(overlapping_consensus=0), **case.opts, **more))


def want_of(case, **more):
    return orc.process(options_of(case, **more), case.g.blob, case.g.rec_off, case.g.rec_len, case.g.grp_first, batch_groups=1000)


class Caller(DD.Caller):
    """A CODEC caller of the library under test (the product's on the GPU, the wave emulator's when FGX_LIB names it): duplex_deep_cases.Caller's two entries
    over one batch, and the path of the last device batch with the two counters of codec_deep.inc."""

    def __init__(self, **opts):
        from fgumi_amd._lib import Options, lib
        self.lib = lib
        self._o = fgx_opts.defaults(kind=2, **dict(dict(overlapping_consensus=0), **opts))
        po = Options.from_buffer_copy(bytes(self._o))
        self.h = lib.fgx_create(C.byref(po))
        assert self.h, lib.fgx_global_error().decode()
        for f in ("fgx_debug_last_big_families", "fgx_debug_last_deep_families", "fgx_debug_last_duplex_deep", "fgx_debug_last_codec_deep", "fgx_debug_last_codec_deep_capped"):
            getattr(lib, f).restype = C.c_uint32                  # (a library without codec_deep.inc has no such counter: the test fails here)
            getattr(lib, f).argtypes = [C.c_void_p]
        lib.fgx_debug_last_chain.restype = None
        lib.fgx_debug_last_chain.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]

    def path(self):
        lib = self.lib
        return dict(DD.Caller.path(self), codec_deep=int(lib.fgx_debug_last_codec_deep(self.h)), codec_deep_capped=int(lib.fgx_debug_last_codec_deep_capped(self.h)))


PATH_KEYS = ("deferred", "codec_deep", "codec_deep_capped", "duplex_deep", "big", "deep")


def assert_path(got, deferred, deep, capped):
    path = {k: got[k] for k in PATH_KEYS}
    assert path == dict(deferred=deferred, codec_deep=deep, codec_deep_capped=capped, duplex_deep=0, big=0, deep=0), (path, deferred, deep, capped)


def check(case, want=None):
    """Both entries against the oracle, and the path of the device batch: `case.deferred` molecules deferred, `case.deep` decided by the new kernels, `case.capped`
    of them with a read dropped by the cap, nothing counted as a simplex big / deep family or a deep duplex molecule.  With nothing deferred the device entry's
    bytes, count and 28 counters are the oracle's; the host entry's always are."""
    want = want or want_of(case)
    c = Caller(**case.opts)
    try:
        got = c.device(case.g)
        print(f"path { {k: got[k] for k in PATH_KEYS} }", flush=True)
        assert_path(got, case.deferred, case.deep, case.capped)
        if case.deferred == 0:
            assert_equal(got, want, "device entry")
        assert_equal(c.host(case.g), want, "host entry")
    finally:
        c.close()
    return want


def check_deferred_beside_decided(case, want_decided):
    """`case`: two molecules, one deferred — the device entry's bytes are the oracle's for the other molecule alone (`want_decided`)."""
    c = Caller(**case.opts)
    try:
        got = c.device(case.g)
        assert_path(got, 1, 1, case.capped)
        assert got["data"] == want_decided["data"] and got["count"] == want_decided["count"]
    finally:
        c.close()
