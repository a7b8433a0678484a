"""Inputs of the unmapped-read tests of the simplex kernels (tests/test_wavemu_unmapped.py on the CPU, tests/test_gpu_unmapped.py on the GPU).

For the simplex caller an unmapped record is a read without a CIGAR (create_source_read, vanilla_caller.rs:1080-1190): it takes no clip against its mate, no
part in the overlap step, and an end that holds mapped AND unmapped source reads loses the unmapped ones (drop_unmapped_if_any_mapped, :1206-1232, counted as
Unmapped).  `unmap` rewrites records of a grouped batch the way an aligner leaves a read it could not place; the crafted batches put such records where each
rule of the reference decides something."""
import dataclasses

import numpy as np

REJ_INSUFFICIENT, REJ_UNMAPPED, REJ_ZERO_LENGTH, REJ_ORPHAN, REJ_DOWNSAMPLED = 1, 3, 11, 13, 19      # FGX_REJ_* (include/fgumi_amd.h)
OVERLAP = slice(24, 28)                                                                              # the four CorrectionStats counters


def _rd(blob, o, width):
    v = np.zeros(len(o), dtype=np.int64)
    for k in range(width):
        v |= blob[o + k].astype(np.int64) << (8 * k)
    return v


def _wr(blob, o, width, v):
    v = np.asarray(v, dtype=np.int64) & ((1 << (8 * width)) - 1)
    for k in range(width):
        blob[o + k] = ((v >> (8 * k)) & 0xFF).astype(np.uint8)


def flags_of(g):
    return _rd(g.blob, np.asarray(g.rec_off, dtype=np.int64) + 14, 2)


def family_of(g):
    """Family index of every record."""
    return np.repeat(np.arange(g.n_grp, dtype=np.int64), np.diff(np.asarray(g.grp_first, dtype=np.int64)))


def index_in_family(g):
    return np.arange(g.n_rec, dtype=np.int64) - np.asarray(g.grp_first, dtype=np.int64)[family_of(g)]


def mates(g):
    """Record index of every record's mate (the other primary record of its name with the other of FIRST / LAST), -1 where there is none."""
    m = np.full(g.n_rec, -1, dtype=np.int64)
    fl = flags_of(g)
    for gi in range(g.n_grp):
        seen = {}
        for r in range(int(g.grp_first[gi]), int(g.grp_first[gi + 1])):
            f = int(fl[r])
            if not (f & 1) or (f & 0x900):
                continue
            o = int(g.rec_off[r])
            key = (bytes(g.blob[o + 32:o + 32 + int(g.blob[o + 8]) - 1]), 1 if (f & 0x40) else 2)
            other = (key[0], 3 - key[1])
            if other in seen:
                m[r], m[seen[other]] = seen[other], r
            seen[key] = r
    return m


def adjacent_mates(g):
    """The simulator's layout: the two mates of a template are adjacent, every family starts at an even record."""
    return np.arange(g.n_rec, dtype=np.int64) ^ 1


def unmap(g, which, placed=False, keep_reverse=True, mate=None):
    """The batch with the records `which` (bool[n_rec]) unmapped: CIGAR stripped, 0x4 set (0x8 on their mates), mapping quality 0, ref_id / pos -1 or — `placed` —
    the mate's original values (what aligners give an unmapped read whose mate is mapped; between two unmapped mates it shows a full shared span to whoever
    compares positions), REVERSE kept or cleared (`keep_reverse`: bool or bool[n_rec]); blob, rec_off, rec_len rebuilt.  Vectorised: no loop over records."""
    which = np.asarray(which, dtype=bool)
    mate = adjacent_mates(g) if mate is None else np.asarray(mate, dtype=np.int64)
    blob = np.array(g.blob, copy=True)
    off = np.asarray(g.rec_off, dtype=np.int64)
    ln = np.asarray(g.rec_len, dtype=np.int64)
    idx = np.flatnonzero(which)
    o = off[idx]
    ref0, pos0, fl0 = _rd(blob, off, 4), _rd(blob, off + 4, 4), _rd(blob, off + 14, 2)       # every record, before any change
    nc = _rd(blob, o + 12, 2)
    l_name = blob[o + 8].astype(np.int64)
    kr = np.broadcast_to(np.asarray(keep_reverse, dtype=bool), (g.n_rec,))
    clear_rev = which & ~kr
    fl = fl0.copy()
    fl[idx] |= 0x4
    fl[clear_rev] &= ~0x10
    has_mate = mate >= 0
    m_un = np.zeros(g.n_rec, dtype=bool)
    m_un[has_mate] = which[mate[has_mate]]
    fl[m_un] |= 0x8
    m_cr = np.zeros(g.n_rec, dtype=bool)
    m_cr[has_mate] = clear_rev[mate[has_mate]]
    fl[m_cr] &= ~0x20
    _wr(blob, off + 14, 2, fl)
    mi = mate[idx]
    take = placed & (mi >= 0)
    _wr(blob, o, 4, np.where(take, ref0[np.maximum(mi, 0)], -1))
    _wr(blob, o + 4, 4, np.where(take, pos0[np.maximum(mi, 0)], -1))
    blob[o + 9] = 0
    _wr(blob, o + 12, 2, np.zeros(len(o), dtype=np.int64))
    cut = 4 * nc
    pre = o >= 4
    _wr(blob, o[pre] - 4, 4, ln[idx][pre] - cut[pre])                                       # the block_size prefix
    keep = np.ones(blob.size, dtype=bool)
    for k in range(int(cut.max()) if len(cut) else 0):
        sel = cut > k
        keep[o[sel] + 32 + l_name[sel] + k] = False
    gone = np.concatenate([[0], np.cumsum(~keep)])                                          # bytes removed before each position
    new_len = ln.copy()
    new_len[idx] -= cut
    return dataclasses.replace(g, blob=np.ascontiguousarray(blob[keep]), rec_off=(off - gone[off]).astype(np.uint64), rec_len=new_len.astype(np.uint32))


def select_records(g, keep_rec):
    """The batch without the records where `keep_rec` is False (families keep their indices; one may become empty)."""
    from fgumi_amd import GroupedReads
    keep_rec = np.asarray(keep_rec, dtype=bool)
    groups = []
    for gi in range(g.n_grp):
        recs = g.records(gi)
        a = int(g.grp_first[gi])
        groups.append([r for k, r in enumerate(recs) if keep_rec[a + k]])
    return GroupedReads.from_groups(groups)


def as_fragments(g):
    """The R1 records of a pair batch as unpaired fragments (PAIRED, PROPER, MATE_UNMAPPED, MATE_REVERSE, FIRST, LAST cleared): an end of one strand per family."""
    f = select_records(g, (flags_of(g) & 0x40) != 0)
    blob = np.array(f.blob, copy=True)
    o = np.asarray(f.rec_off, dtype=np.int64) + 14
    _wr(blob, o, 2, _rd(blob, o, 2) & ~(0x1 | 0x2 | 0x8 | 0x20 | 0x40 | 0x80))
    return dataclasses.replace(f, blob=blob)


def set_qualities(g, recs, q):
    """The batch with every quality of the records `recs` (bool[n_rec]) set to `q`."""
    blob = np.array(g.blob, copy=True)
    o = np.asarray(g.rec_off, dtype=np.int64)[np.asarray(recs, dtype=bool)]
    l_seq = _rd(blob, o + 16, 4)
    q0 = o + 32 + blob[o + 8].astype(np.int64) + 4 * _rd(blob, o + 12, 2) + (l_seq + 1) // 2
    for k in range(int(l_seq.max()) if len(o) else 0):
        sel = l_seq > k
        blob[q0[sel] + k] = q
    return dataclasses.replace(g, blob=blob)


# ---- which records to unmap -------------------------------------------------------------------------------------------------------------------------

def everything(g):
    return np.ones(g.n_rec, dtype=bool)


def all_r2(g):
    """"R1s mapped, R2s unmapped": every end is uniform by flag."""
    return (flags_of(g) & 0x80) != 0


def every_third_pair(g):
    """Both mates of pairs 0, 3, 6, ... of every family (the simulator's layout): both ends hold mapped and unmapped reads."""
    return (index_in_family(g) // 2) % 3 == 0


def r1_of_all_pairs_but_the_first(g):
    return ((flags_of(g) & 0x40) != 0) & (index_in_family(g) // 2 >= 1)


# ---- crafted mixed-end batches (from simulated pair families; read_length 50 at an insert of 70: the mates overlap where they are mapped) ---------------

SHORT = dict(read_length=50, insert_mean=70, insert_sd=5)


def mixed_every_third_pair(n_families=20, depth=5, **sim):
    from fgumi_amd import simulate_grouped_reads
    g = simulate_grouped_reads(n_families, family_size=depth, **{**SHORT, **sim})
    return g, unmap(g, every_third_pair(g))


def mixed_one_mapped_two_unmapped(n_families=20):
    """R1 end: 1 mapped + 2 unmapped reads, R2 end: 3 mapped reads.  At --min-reads 2 the R1 end passes the first two checks with 3 reads, loses its 2 unmapped reads
    (Unmapped) and fails with 1 (InsufficientReads); the R2 end is an orphan."""
    from fgumi_amd import simulate_grouped_reads
    g = simulate_grouped_reads(n_families, family_size=3, **SHORT)
    return g, unmap(g, r1_of_all_pairs_but_the_first(g), placed=True)


def mixed_only_mapped_read_trims_away(n_families=20, low_quality=2):
    """R1 end: one mapped read whose bases are all below --min-input-base-quality + 2 unmapped reads; R2 end: unmapped (no overlap step touches the mapped R1).  The
    mapped read is ZeroLengthAfterTrimming before the drop is evaluated: the unmapped reads stay, nothing counts as Unmapped."""
    from fgumi_amd import simulate_grouped_reads
    g = simulate_grouped_reads(n_families, family_size=3, **SHORT)
    first_r1 = ((flags_of(g) & 0x40) != 0) & (index_in_family(g) // 2 == 0)
    g = set_qualities(g, first_r1, low_quality)
    return g, unmap(g, ~first_r1)
