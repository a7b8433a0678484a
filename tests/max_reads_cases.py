"""Inputs of the --max-reads tests of the streaming kernels (tests/test_wavemu_max_reads.py on the CPU, tests/test_gpu_max_reads_deep.py on the GPU): what the
cap does to a batch, read from the batch itself — record counts per end, fgbio name ranks — and the batches that are not the simulator's as it stands."""
import dataclasses

import numpy as np

import orc

REJ_DOWNSAMPLED = 19          # FGX_REJ_DOWNSAMPLED (include/fgumi_amd.h)
READ_THROUGH = dict(read_length=151, insert_mean=170, insert_sd=40, error_rate_ppm=20000)      # final lengths differ inside an end


def rank(name):
    return orc.lib.orc_read_name_rank(bytes(name), len(name))


def _records(g, gi):
    """(record index, end: 0 fragment / 1 R1 / 2 R2, name) of every record of family gi."""
    out = []
    for r in range(int(g.grp_first[gi]), int(g.grp_first[gi + 1])):
        o = int(g.rec_off[r])
        flag = int(g.blob[o + 14]) | (int(g.blob[o + 15]) << 8)
        end = 0 if not (flag & 1) else 1 if (flag & 0x40) else 2
        out.append((r, end, bytes(g.blob[o + 32:o + 32 + int(g.blob[o + 8]) - 1])))
    return out


def end_sizes(g):
    """Per family: records per end (fragment, R1, R2)."""
    sizes = np.zeros((g.n_grp, 3), dtype=np.int64)
    for gi in range(g.n_grp):
        for _, end, _ in _records(g, gi):
            sizes[gi, end] += 1
    return sizes


def families_the_cap_bites(g, cap):
    """How many families have an end of more than `cap` records."""
    return int((end_sizes(g).max(axis=1) > cap).sum())


def with_tied_names(g, run=3):
    """The batch with every run of `run` consecutive templates of a family under ONE read name (the first template's; the simulator's names have one length, and
    the mates of a template are adjacent): equal fgbio name ranks inside every end, in file order."""
    blob = np.array(g.blob, copy=True)
    for gi in range(g.n_grp):
        recs = _records(g, gi)
        assert len(recs) % 2 == 0 and all(recs[i][2] == recs[i + 1][2] and {recs[i][1], recs[i + 1][1]} == {1, 2} for i in range(0, len(recs), 2))
        for t in range(len(recs) // 2):
            name = recs[2 * (t - t % run)][2]
            for r, _, old in recs[2 * t:2 * t + 2]:
                assert len(old) == len(name)
                o = int(g.rec_off[r]) + 32
                blob[o:o + len(name)] = np.frombuffer(name, dtype=np.uint8)
    return dataclasses.replace(g, blob=blob)


def families_with_a_tie_cut_in_the_middle(g, cap):
    """How many families have an end where the read in place `cap` of the cap's order (rank, then file order) has the rank of the read in place `cap` + 1: the
    cap keeps some reads of a group of equal ranks and drops the others."""
    n = 0
    for gi in range(g.n_grp):
        recs = _records(g, gi)
        hit = False
        for end in range(3):
            order = sorted((rank(name), r) for r, e, name in recs if e == end)
            hit = hit or (len(order) > cap and order[cap - 1][0] == order[cap][0])
        n += hit
    return n


def methylation_batch(seed, n_groups):
    """(contigs, GroupedReads) of tests/methsim.py's simplex groups whose records are each one CIGAR op."""
    import bamutil
    import methsim
    from fgumi_amd import GroupedReads
    rng = methsim.seeded(seed)
    contigs = methsim.genome(rng)
    groups = [g for g in methsim.simplex_groups(rng, contigs, n_groups) if all(bamutil.parse(r)["n_cigar"] == 1 for r in g)]
    return contigs, GroupedReads.from_groups(groups)
