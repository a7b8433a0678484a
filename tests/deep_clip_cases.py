"""Inputs and the runner of the FGX_DEEP_CLIPS=1 tests (tests/test_wavemu_deep_clips.py on the CPU, tests/test_gpu_deep_clips.py on the GPU): simplex families and
duplex molecules of more than 64 records that hold soft- / hard-clipped reads (H* S* (M|=|X)+ S* H*, up to 16 ops).  With the switch unset one such read sends
the group to k_family or to the deferred list; with it the clip-taking builds of the streaming record kernels (k_deep_parse<.., .., 1> outside the
methylation-aware mode, k_duplex_deep_parse<.., .., .., 1>) decide it, and fgx_debug_last_deep_clipped counts it.

Every case compares both entries with the oracle — bytes, count and all 28 counters — and asserts the path of the device batch: the deferred count, the
groups the streaming kernels decided (`duplex_deep` / `deep`) and the new counter.  Read names are of fixed width (the record kernels leave a group whose
30-bit name hashes collide, which short running names do in deep groups); a batch holds a handful of groups."""
import contextlib
import ctypes as C
import dataclasses
import os
import random

import numpy as np

import bamutil
import duplex_deep_cases as D
import fgx_opts
import methclip_cases as mc
import methsim
import orc
from wide_cases import assert_equal, records_per_family

EMULATED = "FGX_LIB" in os.environ
REJ_ZERO_LENGTH = D.REJ_ZERO_LENGTH
PAIRED, PROPER, UNMAPPED, MATE_UNMAPPED, REVERSE, MATE_REVERSE, FIRST, LAST = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80
OV_BASES, OV_AGREE, OV_DISAGREE, OV_CORRECTED = 24, 25, 26, 27          # fgx_output.stats: the overlapping-bases counters


@dataclasses.dataclass
class Case:
    g: object                  # GroupedReads
    kind: int = 1              # 1 duplex, 0 simplex
    opts: dict = dataclasses.field(default_factory=dict)
    deferred: int = 0          # groups the device entry defers
    deep: int = 0              # groups the streaming kernels decide (fgx_debug_last_duplex_deep / fgx_debug_last_deep_families)
    clipped: int = 0           # fgx_debug_last_deep_clipped
    env: dict = dataclasses.field(default_factory=lambda: dict(FGX_DEEP_CLIPS="1"))    # the switches of the batch (FGX_DEEP_CLIPS absent: unset)
    contigs: object = None     # methylation-aware mode: the reference


SWITCHES = ("FGX_DEEP_CLIPS", "FGX_DUPLEX_DEEP_CAP")


@contextlib.contextmanager
def switches(env):
    """The switches are read per call: set for the batches inside, put back afterwards."""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def unset(case, **changes):
    """The same batch with FGX_DEEP_CLIPS unset."""
    return dataclasses.replace(case, env={k: v for k, v in case.env.items() if k != "FGX_DEEP_CLIPS"}, **changes)


def _groups(groups):
    from fgumi_amd import GroupedReads
    return GroupedReads.from_groups([[bytes(r) for r in recs] for recs in groups])


def multi_groups(groups, above=64):
    """Groups of more than `above` records that hold a record of more than one CIGAR op."""
    return sum(len(g) > above and any(mc.multi_op(r) for r in g) for g in groups)


# ---- reads from a CIGAR -----------------------------------------------------------------------------------------------------------------------------------
def read_of(rng, contig, pos, cigar, err=0.003):
    """Stored bases of a read aligned at 0-based `pos` with `cigar`: aligned ops copy the reference, soft clips and insertions are random bases."""
    ref = contig.decode().upper().replace("N", "A")
    seq, p = [], pos
    for op in bamutil.cigar_ops(cigar):
        k, n = "MIDNSHP=X"[op & 15], op >> 4
        if k in "M=X":
            seq.append((ref[p:p + n] + "A" * n)[:n])
            p += n
        elif k in "SI":
            seq.append("".join(rng.choice("ACGT") for _ in range(n)))
        elif k in "DN":
            p += n
    s = "".join(seq)
    return "".join(rng.choice("ACGT") if rng.random() < err else b for b in s)


def plain(L):
    return f"{L}M"


SHAPES = {
    "leading": lambda L: f"5S{L - 5}M",
    "trailing": lambda L: f"{L - 6}M6S",
    "both": lambda L: f"3S{L - 7}M4S",
    "hard_and_soft": lambda L: f"2H3S{L - 7}M4S1H",                       # (2H3S33M4S1H at 40 bases)
    "eq_x_blocks": lambda L: f"1H2S10=1X{L - 16}=3S1H",                    # (1H2S10=1X20=3S1H at 36 bases)
    "sixteen_ops": lambda L: "1H1S" + "2=1X" * 5 + f"{L - 18}=1X" + "1S1H",        # H S (= X) x 6 S H
    "seventeen_ops": lambda L: "1H1S" + "2=1X" * 5 + f"{L - 20}=1X2M" + "1S1H",
    "only_soft_clips": lambda L: f"{L}S",
    "nine_ops": lambda L: "1H1S" + "2=1X" * 2 + f"{L - 9}=1X" + "1S",    # (its mate's MC then holds nine ops)
}


def folded(cigar):
    """`cigar` with its = and X ops folded into M and neighbours merged: the same read to every rule of the mate clip, in fewer ops (an MC of more than eight
    ops is a reason of its own to hand a molecule on)."""
    out = []
    for op in bamutil.cigar_ops(cigar):
        k, n = "MIDNSHPMM"[op & 15], op >> 4
        if out and out[-1][0] == k:
            out[-1][1] += n
        else:
            out.append([k, n])
    return "".join(f"{n}{k}" for k, n in out)


def _n_ops(cigar):
    return len(bamutil.cigar_ops(cigar))


assert [_n_ops(SHAPES[k](60)) for k in ("sixteen_ops", "seventeen_ops", "nine_ops")] == [16, 17, 9]


def hash30(name):
    """record_core.h's name_hash30, the low 30 bits the record kernels pair mates by (a filter: equal hashes under different names send the group on)."""
    M = 0xFFFFFFFF

    def rotl(v, r):
        return ((v << r) | (v >> (32 - r))) & M

    def w32(o):
        return int.from_bytes(name[o:o + 4], "little")
    n = len(name)
    h, i = n, 0
    while i + 8 <= n:
        h = rotl(h, 5) ^ w32(i)
        h = (rotl(h, 11) + w32(i + 4)) & M
        i += 8
    if i < n:
        v = name[-8:] if n >= 8 else name + bytes(8 - n)
        h = rotl(h, 5) ^ int.from_bytes(v[:4], "little")
        h = (rotl(h, 11) + int.from_bytes(v[4:], "little")) & M
    return (h ^ (h >> 15) ^ (h << 7)) & 0x3FFFFFFF


def distinct_names(stem, n):
    """n names `<stem>_<4 digits>` with distinct pairing hashes: running numbers, those left out whose hash an earlier name of the group has."""
    names, seen, k = [], set(), 0
    while len(names) < n:
        name = f"{stem}_{k:04d}"
        k += 1
        if hash30(name.encode()) not in seen:
            seen.add(hash30(name.encode()))
            names.append(name)
    assert k <= 9999
    return names


def _q(rng, seq):
    return [rng.choice([25, 30, 37]) for _ in seq]


def duplex_molecule(rng, contig, g, na, nb, L, p1, p2, cigar_of=None, clip_share=0.0, ref_id=0, mc_of=None):
    """A duplex molecule of 2 (na + nb) records, tests/methclip_cases.py's layout with ten-character names: the /A templates first (R1 forward at p1, R2 reverse at
    p2), then the /B templates (R1 reverse at p2, R2 forward at p1), mates adjacent; every MC is the mate's real CIGAR (or `mc_of` of it).  `cigar_of(strand, i, first)` names the
    CIGAR shape (a key of SHAPES) of one read, or None; else each read is clipped (a shape drawn from the first four) with probability `clip_share`."""
    def cig(strand, i, first):
        name = cigar_of(strand, i, first) if cigar_of else (rng.choice(["leading", "trailing", "both", "hard_and_soft"]) if rng.random() < clip_share else None)
        return SHAPES[name](L) if name else plain(L)

    reads, names = [], distinct_names(f"d{g:04d}", na + nb)
    for strand, n in (("A", na), ("B", nb)):
        for i in range(n):
            c1, c2 = cig(strand, i, True), cig(strand, i, False)
            name = names[i + (na if strand == "B" else 0)]
            mi = f"{g}/{strand}"
            rx = "ACG-TTA" if strand == "A" else "TTA-ACG"
            if strand == "A":
                pos1, pos2, f1, f2 = p1, p2, PAIRED | FIRST | MATE_REVERSE, PAIRED | LAST | REVERSE
            else:
                pos1, pos2, f1, f2 = p2, p1, PAIRED | FIRST | REVERSE, PAIRED | LAST | MATE_REVERSE
            s1, s2 = read_of(rng, contig, pos1, c1), read_of(rng, contig, pos2, c2)
            assert len(s1) == L and len(s2) == L, (c1, c2, L)
            for seq, c, f, pos, mpos, mcig in ((s1, c1, f1, pos1, pos2, c2), (s2, c2, f2, pos2, pos1, c1)):
                reads.append(bamutil.make_record(name, seq, _q(rng, seq), flag=f, ref_id=ref_id, pos=pos, mapq=60, cigar=c, mate_ref=ref_id, mate_pos=mpos,
                                                 tags=[("MI", "Z", mi), ("RX", "Z", rx), ("MC", "Z", mc_of(mcig) if mc_of else mcig)]))
    return reads


def _genome(seed):
    rng = random.Random(seed)
    return rng, methsim.genome(rng)


# ---- duplex 1 / 10: the existing soft-clip case ---------------------------------------------------------------------------------------------------------------
def soft_clip_of_the_existing_tests():
    c = D.not_this_path("soft_clip")
    assert records_per_family(c.g).tolist() == [80]
    return Case(c.g, deep=1, clipped=1)


def still_deferred(what):
    c = D.not_this_path(what)
    return Case(c.g, deferred=1)


# ---- duplex 2: sizes, a clipped read in each of the four sets ---------------------------------------------------------------------------------------------------
def _four_sets(strand, i, first):
    """Template 1 of each strand: both mates clipped — one read of AB-R1, AB-R2, BA-R1 and BA-R2 each."""
    return ("leading" if first else "both") if i == 1 else None


def sized(n_records):
    rng, contigs = _genome(1000 + n_records)
    na = (n_records // 2 + 1) // 2
    nb = n_records // 2 - na
    recs = duplex_molecule(rng, contigs[0], 0, na, nb, 60, 500, 530, _four_sets)
    assert len(recs) == n_records and sum(mc.multi_op(r) for r in recs) == 4
    if n_records <= 64:
        return Case(_groups([recs]))            # k_family_wave<1>'s, and the canonical second pass's: nothing of this path
    if n_records >= 512:                        # 256 reads on a record side: deferred for the bound, beside a molecule that stays
        stay = duplex_molecule(rng, contigs[1], 1, 17, 16, 60, 700, 720, _four_sets)
        return Case(_groups([stay, recs]), deferred=1, deep=1, clipped=1)
    return Case(_groups([recs]), deep=1, clipped=1)


# ---- duplex 3: clip shapes, each on a forward and a reverse read, on R1 and R2, on /A and /B -----------------------------------------------------------------------
TAKEN_SHAPES = ("leading", "trailing", "both", "hard_and_soft", "eq_x_blocks", "sixteen_ops")
DEFERRED_SHAPES = ("seventeen_ops", "only_soft_clips", "nine_ops")


def shaped(shape):
    rng, contigs = _genome(2000 + sorted(SHAPES).index(shape))

    def where(strand, i, first):       # /A: template 1's R1 (forward), template 2's R2 (reverse); /B: template 1's R1 (reverse), template 2's R2 (forward)
        return shape if (i == 1 and first) or (i == 2 and not first) else None
    # (sixteen / seventeen ops: the mates' MC in the folded form, so that the number of the read's own ops decides alone; nine ops: the real CIGAR as MC)
    recs = duplex_molecule(rng, contigs[0], 0, 20, 20, 64, 900, 930, where, mc_of=folded if shape in ("sixteen_ops", "seventeen_ops") else None)
    assert sum(mc.multi_op(r) for r in recs) == 4 or shape == "only_soft_clips"
    if shape in TAKEN_SHAPES:
        return Case(_groups([recs]), deep=1, clipped=1)
    return Case(_groups([recs]), deferred=1)


# ---- duplex 4: overlap ---------------------------------------------------------------------------------------------------------------------------------------
def overlap_with_leading_clips():
    """The mates' aligned blocks overlap by half a read and every forward read has a leading clip: its query offset is not its reference offset."""
    rng, contigs = _genome(3001)
    recs = duplex_molecule(rng, contigs[0], 0, 22, 20, 70, 1200, 1235, lambda strand, i, first: "leading" if (strand == "A") == first else None)
    return Case(_groups([recs]), deep=1, clipped=1)


def blocks_apart_reads_not():
    """`100M50S` at 1000 beside a reverse mate `150M` at 1110: pos .. pos + l_seq of the mates overlap, the aligned blocks do not."""
    rng, contigs = _genome(3002)
    contig, reads, names = contigs[0], [], distinct_names("d0000", 100)
    for strand, n in (("A", 20), ("B", 20)):
        for i in range(n):
            name, mi, rx = names[i + (0 if strand == "A" else 50)], f"0/{strand}", "ACG-TTA" if strand == "A" else "TTA-ACG"
            fwd, rev = read_of(rng, contig, 1000, "100M50S"), read_of(rng, contig, 1110, "150M")
            first_is_fwd = strand == "A"
            for is_first in (True, False):
                is_fwd = is_first == first_is_fwd
                seq, cig, pos, mpos, mcig = (fwd, "100M50S", 1000, 1110, "150M") if is_fwd else (rev, "150M", 1110, 1000, "100M50S")
                flag = PAIRED | (FIRST if is_first else LAST) | (MATE_REVERSE if is_fwd else REVERSE)
                reads.append(bamutil.make_record(name, seq, _q(rng, seq), flag=flag, ref_id=0, pos=pos, mapq=60, cigar=cig, mate_ref=0, mate_pos=mpos,
                                                 tags=[("MI", "Z", mi), ("RX", "Z", rx), ("MC", "Z", mcig)]))
    return Case(_groups([reads]), deep=1, clipped=1)


# ---- duplex 5: read-through: an insert of 100 under reads of 150, the adapter bases soft-clipped ----------------------------------------------------------------
def read_through():
    rng, contigs = _genome(3003)
    contig, reads, names = contigs[1], [], distinct_names("d0000", 100)
    for strand, n in (("A", 21), ("B", 19)):
        for i in range(n):
            name, mi, rx = names[i + (0 if strand == "A" else 50)], f"0/{strand}", "ACG-TTA" if strand == "A" else "TTA-ACG"
            fwd, rev = read_of(rng, contig, 2000, "100M50S"), read_of(rng, contig, 2000, "50S100M")
            first_is_fwd = strand == "A"
            for is_first in (True, False):
                is_fwd = is_first == first_is_fwd
                seq, cig, mcig = (fwd, "100M50S", "50S100M") if is_fwd else (rev, "50S100M", "100M50S")
                flag = PAIRED | (FIRST if is_first else LAST) | (MATE_REVERSE if is_fwd else REVERSE)
                reads.append(bamutil.make_record(name, seq, _q(rng, seq), flag=flag, ref_id=1, pos=2000, mapq=60, cigar=cig, mate_ref=1, mate_pos=2000,
                                                 tags=[("MI", "Z", mi), ("RX", "Z", rx), ("MC", "Z", mcig)]))
    return Case(_groups([reads]), deep=1, clipped=1)


# ---- duplex 6 / 7: the option matrix and the strand cap on molecules with a tenth / a third of their reads clipped ----------------------------------------------------
OPTION_MATRIX = {k: D.OPTION_MATRIX[k] for k in ("overlapping_off", "min_input_base_quality_30", "min_reads_3_2_1", "per_base_tags_off", "long_prefix", "reads_of_300_bases")}


def _tail(seed, L, share, pairs=((25, 15), (40, 30), (70, 50))):
    rng, contigs = _genome(seed)
    groups = []
    for g, (na, nb) in enumerate(pairs):
        p1 = 300 + 900 * g
        groups.append(duplex_molecule(rng, contigs[g % len(contigs)], g, na, nb, L, p1, p1 + L - rng.randint(5, L // 3), clip_share=share, ref_id=g % len(contigs)))
    return groups


def option_case(name):
    groups = _tail(4001, 300 if name == "reads_of_300_bases" else 75, 0.1)
    n = [len(g) for g in groups]
    assert n == [80, 140, 240] and multi_groups(groups) == 3
    return Case(_groups(groups), opts=OPTION_MATRIX[name], deep=3, clipped=3)


def strand_cap():
    groups = _tail(4002, 70, 0.3, pairs=((40, 40),))
    return Case(_groups(groups), opts=dict(duplex_max_reads_per_strand=10), deep=1, clipped=1, env=dict(FGX_DEEP_CLIPS="1", FGX_DUPLEX_DEEP_CAP="1"))


# ---- duplex 8: a mixed stream -----------------------------------------------------------------------------------------------------------------------------------
def mixed_stream():
    small = D._sim(2000, family_size=1, family_size_max=5, error_rate_ppm=5000)
    rng, contigs = _genome(4003)
    plain_mol = D._sim(1, family_size=45, seed=9).records(0)
    clipped = duplex_molecule(rng, contigs[0], 7001, 30, 25, 80, 400, 440, clip_share=0.1)
    with_del = duplex_molecule(rng, contigs[1], 7002, 25, 25, 80, 400, 440, lambda strand, i, first: None)
    r = bytearray(with_del[10])
    with_del[10] = bytes(D._with_cigar(r, [(40 << 4) | 0, (2 << 4) | 2, (40 << 4) | 0]))
    groups = [small.records(i) for i in range(1000)] + [plain_mol, clipped, with_del] + [small.records(i) for i in range(1000, 2000)]
    assert multi_groups([clipped]) == 1
    return Case(_groups(groups), deferred=1, deep=2, clipped=1)


# ---- simplex 11: families of 66, 128, 130 and 500 records (an end holds at most 255 reads: the largest family of fragments has 250) -----------------------------------
LAYOUTS = ("frag", "frag_rev", "pair", "pair_overlap")


def simplex_sizes(layout):
    rng, contigs = _genome(5000 + LAYOUTS.index(layout))
    is_pair = layout.startswith("pair")
    sizes = (66, 128, 130, 500) if is_pair else (66, 128, 130, 250)
    groups = []
    for n in sizes:
        d = n // 2 if is_pair else n
        groups += mc.simplex_ms_groups(rng, contigs, 1, depth=(d, d), read_len=(60, 110), per_read_clip=0.1, layouts=(layout,), long_names=True)
    groups = [_renamed(g, k) for k, g in enumerate(groups)]      # (simplex_ms_groups numbers the groups of one call: MI and names of the k-th call become its own)
    assert [len(g) for g in groups] == list(sizes) and multi_groups(groups) == 4
    return Case(_groups(groups), kind=0, deep=4, clipped=4)


def _renamed(group, k):
    """The family as group k: MI `k`, and names `<f|p><k, 4 digits>_<4 digits>` with distinct pairing hashes (mates keep sharing theirs)."""
    old = list(dict.fromkeys(bytes(r[32:32 + r[8] - 1]) for r in group))
    assert all(len(n) == 10 for n in old)
    new = dict(zip(old, distinct_names(f"{chr(old[0][0])}{k:04d}", len(old))))
    out = []
    for rec in group:
        r = bytearray(rec)
        r[32:42] = new[bytes(r[32:42])].encode()
        o, ln = D._tag_value(r, b"MI")
        assert bytes(r[o:o + ln]) == b"0" and 0 <= k <= 9
        r[o] = ord("0") + k
        out.append(bytes(r))
    return out


def simplex_sizes_unset(layout):
    """Today's routes: up to 128 records k_family, above that the deferred list."""
    c = simplex_sizes(layout)
    return unset(c, deep=0, clipped=0, deferred=int((records_per_family(c.g) > 128).sum()))


# ---- simplex 12: --max-reads 50 on a family of 700 records ------------------------------------------------------------------------------------------------------------
def under_max_reads():
    rng, contigs = _genome(5010)
    groups = [_renamed(mc.simplex_ms_groups(rng, contigs, 1, depth=(700, 700), read_len=(60, 110), per_read_clip=0.1, layouts=("frag",), long_names=True)[0], 0)]
    n_multi = sum(mc.multi_op(r) for r in groups[0])
    assert len(groups[0]) == 700 and 40 < n_multi < 110          # (a tenth: clipped reads among the 50 survivors and among the 650 dropped reads)
    return Case(_groups(groups), kind=0, opts=dict(max_reads=50), deep=1, clipped=1)


# ---- simplex 13: clipped R1s with unmapped R2s --------------------------------------------------------------------------------------------------------------------
def _r1_mapped_r2_unmapped(rng, contig, n_pairs, mapped_r2_at=()):
    reads, names = [], distinct_names("u0000", n_pairs)
    for i in range(n_pairs):
        c1 = SHAPES[rng.choice(["leading", "both", "hard_and_soft"])](70) if i % 3 == 0 else plain(70)
        s1 = read_of(rng, contig, 600, c1)
        s2 = "".join(rng.choice("ACGT") for _ in range(70))
        name, tags = names[i], [("MI", "Z", "0"), ("RX", "Z", "AAC-GGT")]
        if i in mapped_r2_at:
            r1, r2 = bamutil.pair(name, s1, _q(rng, s1), read_of(rng, contig, 800, "70M"), _q(rng, s2), "0", pos1=600, pos2=800, cigar1=c1, cigar2="70M", rx="AAC-GGT")
        else:
            r1 = bamutil.make_record(name, s1, _q(rng, s1), flag=PAIRED | FIRST | MATE_UNMAPPED, ref_id=0, pos=600, cigar=c1, mate_ref=0, mate_pos=600, tags=tags)
            r2 = bamutil.make_record(name, s2, _q(rng, s2), flag=PAIRED | LAST | UNMAPPED, ref_id=0, pos=600, mapq=0, mate_ref=0, mate_pos=600, tags=tags)
        reads += [r1, r2]
    return reads


def clipped_r1_unmapped_r2():
    rng, contigs = _genome(5020)
    recs = _r1_mapped_r2_unmapped(rng, contigs[0], 80)
    assert len(recs) == 160 and sum(mc.multi_op(r) for r in recs) == 27
    return Case(_groups([recs]), kind=0, deep=1, clipped=1)


def mixed_end_beside_a_clipped_read():
    """One R2 of the 80 is mapped: its end mixes mapped and unmapped reads — handed on as today (160 records: the deferred list)."""
    rng, contigs = _genome(5021)
    recs = _r1_mapped_r2_unmapped(rng, contigs[0], 80, mapped_r2_at=(40,))
    return Case(_groups([recs]), kind=0, deferred=1)


# ---- simplex 14: a clipped read beside a deletion read ------------------------------------------------------------------------------------------------------------
def clip_beside_deletion(n_records):
    rng, contigs = _genome(5030 + n_records)
    recs = mc.simplex_ms_groups(rng, contigs, 1, depth=(n_records, n_records), read_len=(70, 90), per_read_clip=0.1, layouts=("frag",), long_names=True)[0]
    k = next(i for i, r in enumerate(recs) if not mc.multi_op(r))
    L = int.from_bytes(recs[k][16:20], "little")
    recs[k] = bytes(D._with_cigar(bytearray(recs[k]), [(30 << 4) | 0, (2 << 4) | 2, ((L - 30) << 4) | 0]))
    assert any(mc.multi_op(r) and not mc.has_indel(r) for r in recs)
    return Case(_groups([recs]), kind=0, deferred=1 if n_records > 128 else 0)


# ---- simplex 15: the methylation-aware mode -----------------------------------------------------------------------------------------------------------------------
def methylation_batch():
    contigs, groups, n_clip = mc.ms_batch(0, 60, 97)
    return contigs, groups, n_clip


# ---- the runner -----------------------------------------------------------------------------------------------------------------------------------------------
def options_of(case):
    return fgx_opts.defaults(kind=case.kind, **case.opts)


def want_of(case):
    orc.set_reference(case.contigs)
    try:
        return orc.process(options_of(case), case.g.blob, case.g.rec_off, case.g.rec_len, case.g.grp_first, batch_groups=100 if case.kind == 1 else 50)
    finally:
        orc.set_reference(None)


class Caller(D.Caller):
    """duplex_deep_cases.Caller for either caller kind, with the new counter (and the capped molecules) in the path."""

    def __init__(self, kind=1, contigs=None, **opts):
        super().__init__(contigs, **dict(opts, caller_kind=kind))
        for f in ("fgx_debug_last_deep_clipped", "fgx_debug_last_duplex_deep_capped", "fgx_debug_last_meth_clipped"):
            getattr(self.lib, f).restype = C.c_uint32
            getattr(self.lib, f).argtypes = [C.c_void_p]

    def path(self):
        lib = self.lib
        return dict(super().path(), clipped=int(lib.fgx_debug_last_deep_clipped(self.h)), capped=int(lib.fgx_debug_last_duplex_deep_capped(self.h)),
                    meth_clipped=int(lib.fgx_debug_last_meth_clipped(self.h)))


PATH_KEYS = ("deferred", "duplex_deep", "big", "deep", "clipped", "capped")


def assert_path(case, got):
    path = {k: got[k] for k in PATH_KEYS}
    print(f"path {path}", flush=True)
    assert got["deferred"] == case.deferred and got["clipped"] == case.clipped, (path, case.deferred, case.clipped)
    if case.kind == 1:
        assert got["duplex_deep"] == case.deep and got["big"] == 0 and got["deep"] == 0, (path, case.deep)
    else:
        assert got["deep"] == case.deep and got["duplex_deep"] == 0, (path, case.deep)


def check(case, want=None):
    """Both entries against the oracle under the case's switches, and the path of the device batch.  With nothing deferred the device entry's bytes, count and
    28 counters are the oracle's; the host entry's always are."""
    want = want or want_of(case)
    with switches(case.env):
        c = Caller(case.kind, case.contigs, **case.opts)
        try:
            got = c.device(case.g)
            assert_path(case, got)
            if case.deferred == 0:
                assert_equal(got, want, "device entry")
            assert_equal(c.host(case.g), want, "host entry")
        finally:
            c.close()
    return want, got


def check_deferred_beside_decided(case, keep):
    """`case` defers some molecules: the device entry's bytes and count are the oracle's for the molecules `keep` alone; the host entry's for the whole batch."""
    from fgumi_amd import GroupedReads
    want_kept = want_of(dataclasses.replace(case, g=GroupedReads.from_groups([case.g.records(i) for i in keep])))
    want, got = check(case)
    assert got["data"] == want_kept["data"] and got["count"] == want_kept["count"]
    return want


def chains(g, envs, kind=1, **opts):
    """(launches, host synchronisations, path) of the batch under each of `envs`, on one caller whose first batch (it uploads the table images) is not compared."""
    c = Caller(kind, **opts)
    try:
        with switches({}):
            c.device(g)
        out = []
        for env in envs:
            with switches(env):
                got = c.device(g)
                out.append((c.chain(), {k: got[k] for k in PATH_KEYS}, got))
        return out
    finally:
        c.close()


# ---- the checks both test files run (tests/test_wavemu_deep_clips.py in child interpreters on the emulation library, tests/test_gpu_deep_clips.py on the GPU) ----
def check_case(name, *args):
    return check(globals()[name](*args))


def check_size(n_records):
    case = sized(n_records)
    if n_records >= 512:
        assert records_per_family(case.g).tolist() == [66, 512]
        check_deferred_beside_decided(case, keep=[0])
    else:
        check(case)


def check_overlap_with_leading_clips():
    case = overlap_with_leading_clips()
    want = want_of(case)
    ov = [int(want["stats"][k]) for k in (OV_BASES, OV_AGREE, OV_DISAGREE, OV_CORRECTED)]
    print(f"the oracle's overlapping-bases counters: {ov}", flush=True)
    assert all(v > 0 for v in ov), ov                                  # (not an empty comparison)
    check(case, want)


def check_blocks_apart():
    """A span taken from l_seq would find 40 shared positions per pair here; the aligned blocks share none, and the oracle corrects nothing."""
    case = blocks_apart_reads_not()
    want = want_of(case)
    assert int(want["stats"][OV_AGREE]) + int(want["stats"][OV_DISAGREE]) == 0, want["stats"].tolist()
    check(case, want)


def check_read_through():
    """The aligned blocks of a pair are the same 100 positions: every one of them is an overlapping base (40 pairs x 100), no read is trimmed to nothing
    (ZeroLengthAfterTrimming 0), and the mate clip cuts the 50 soft-clipped adapter bases of every read: the consensus records are 100 bases long, not 150."""
    from fgumi_amd import split_records
    case = read_through()
    want = want_of(case)
    st = want["stats"]
    lens = [len(bamutil.parse(r)["seq"]) for r in split_records(want["data"])]
    print(f"the oracle: ZeroLengthAfterTrimming {int(st[3 + REJ_ZERO_LENGTH])}, overlapping bases {int(st[OV_BASES])}, corrected {int(st[OV_CORRECTED])}, record lengths {lens}", flush=True)
    assert int(st[3 + REJ_ZERO_LENGTH]) == 0 and int(st[OV_BASES]) == 40 * 100 and int(st[OV_CORRECTED]) > 0, st.tolist()
    assert lens == [100, 100], lens
    check(case, want)


def check_strand_cap():
    want, got = check(strand_cap())
    assert got["capped"] >= 1, got["capped"]


def check_path_off(what):
    """--trim, --rejects, the methylation-aware mode with the switch on: the outcome of tests/duplex_deep_cases.py's cases, as with it unset."""
    import pytest
    contigs = D.methylation_contigs() if what == "methylation" else None
    case = D.path_off_case(what)
    with switches(dict(FGX_DEEP_CLIPS="1")):
        if what != "rejects":
            D.check(case, contigs=contigs)
            return
        want = D.want_of(case)
        c = Caller(1, **case.opts)
        try:
            with pytest.raises(AssertionError, match="defers"):
                c.device(case.g)
            got = c.host(case.g)
            assert got["duplex_deep"] == 0 and got["big"] == 0 and got["deep"] == 0 and got["clipped"] == 0, got
            assert_equal(got, want, "host entry")
        finally:
            c.close()


def check_switch_unset():
    """Unset, "0" and "": the soft-clip molecule is deferred as before and the counter is 0."""
    case = soft_clip_of_the_existing_tests()
    want = want_of(case)
    for env in ({}, dict(FGX_DEEP_CLIPS="0"), dict(FGX_DEEP_CLIPS="")):
        check(dataclasses.replace(case, env=env, deferred=1, deep=0, clipped=0), want)


def check_unchanged_chain(what):
    """A batch without a deep molecule, and one without a clipped read: the same kernel launches and host synchronisations with the switch on and unset."""
    case = D.shallow() if what == "shallow" else D.pairs(40, 2)
    want = D.want_of(case)
    (ch_on, path_on, got_on), (ch_off, path_off, got_off) = chains(case.g, [dict(FGX_DEEP_CLIPS="1"), {}])
    print(f"(launches, host synchronisations): on {ch_on}, unset {ch_off}; path on {path_on}", flush=True)
    assert ch_on == ch_off and ch_on[0] > 0, (ch_on, ch_off)
    assert path_on == path_off and path_on["clipped"] == 0 and path_on["deferred"] == 0, (path_on, path_off)
    assert path_on["duplex_deep"] == (0 if what == "shallow" else 2)
    assert_equal(got_on, want, "device entry, switch on")
    assert_equal(got_off, want, "device entry, switch unset")


def check_methylation_mode():
    """The methylation-aware mode with the switch on: every family on the mode's kernels, fgx_debug_last_meth_clipped the clipped families — as with the switch
    unset — and the new counter 0."""
    contigs, groups, n_clip = methylation_batch()
    g = _groups(groups)
    case = Case(g, kind=0, opts=dict(methylation_mode=1), deep=g.n_grp, clipped=0, contigs=contigs)
    want = want_of(case)
    seen = []
    for env in (dict(FGX_DEEP_CLIPS="1"), {}):
        _, got = check(dataclasses.replace(case, env=env), want)
        assert got["meth_clipped"] == n_clip, (got["meth_clipped"], n_clip)
        seen.append({k: got[k] for k in PATH_KEYS + ("meth_clipped",)})
    assert seen[0] == seen[1], seen
