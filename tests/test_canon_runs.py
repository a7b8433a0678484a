"""The REFERENCE RUNS the canonical form of a duplex molecule emits for the methylation-aware mode (canon_core.h `ref_runs_of`, FGX_METH_CANON=1).

A canonical record is `<len>M` at its old position, R2 on another reference id: it no longer says where its bases lie.  The mode's annotation needs
exactly that of the call's anchor read (query_to_ref_positions, methylation.rs:116-178), so the canonical pass emits it per surviving record as a short
list of aligned runs.  The claim checked here, through the oracle: for every surviving record the runs expand to what the reference computes from the
ORIGINAL record — its simplified CIGAR (S H = X folded into M, adjacent ops merged), reversed for a reverse read and truncated to the source read's final
length, against the folded original and the original position.  The test rebuilds those CIGARs in Python from the original record and the canonical
record's bases; nothing of the product's walk is reused."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import bamutil
import fgx_opts
import orc
import test_canon_core as tcc
from fgumi_amd import GroupedReads
from fgumi_amd._lib import lib

WORDS = 34                       # FGX_CANON_RUNS_WORDS
OTHER_REF_XOR = 0x20000000


def canonicalise_with_runs(o, group):
    """-> (status, [(original record, canonical record or None, runs dict or None)])"""
    g = GroupedReads.from_groups([group])
    out = np.zeros(g.blob.size + 16, dtype=np.uint8)
    out_len = np.zeros(max(1, g.n_rec), dtype=np.uint32)
    delta = np.zeros(5, dtype=np.uint64)
    runs = np.zeros(max(1, g.n_rec) * WORDS, dtype=np.uint32)
    rc = lib.fgx_canon_duplex_runs_host(C.addressof(o), g.blob.ctypes.data, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, out.ctypes.data, out_len.ctypes.data,
                                        delta.ctypes.data, runs.ctypes.data)
    res = []
    for i in range(g.n_rec):
        if rc != 0 or not out_len[i]:
            res.append((group[i], None, None))
            continue
        w = runs[i * WORDS:(i + 1) * WORDS]
        n = int(w[1]) & 0x7FFFFFFF
        rr = [(int(w[2 + 4 * k]), int(w[3 + 4 * k]), int(np.array([w[4 + 4 * k], w[5 + 4 * k]], dtype=np.uint32).view(np.int64)[0])) for k in range(n)]
        res.append((group[i], bytes(out[int(g.rec_off[i]):int(g.rec_off[i]) + int(out_len[i])]), dict(ref_id=int(np.int32(w[0])), rev=bool(w[1] >> 31), runs=rr)))
    return rc, res


def expand(r, n_query):
    pos = [None] * n_query
    step = -1 if r["rev"] else 1
    for q0, ln, ref0 in r["runs"]:
        for j in range(ln):
            if q0 + j < n_query:
                assert pos[q0 + j] is None, "runs overlap"
                pos[q0 + j] = ref0 + step * j
    return pos


def fold(ops):
    """simplify_cigar: S H = X -> M, adjacent ops of a kind merged; [(kind, length)]"""
    out = []
    for k, n in ops:
        k = "M" if k in "SH=X" else k
        if out and out[-1][0] == k:
            out[-1] = (k, out[-1][1] + n)
        else:
            out.append((k, n))
    return out


def truncate(ops, length):
    out, left = [], length
    for k, n in ops:
        if left <= 0:
            break
        if k in "MI":
            t = min(n, left)
            out.append((k, t))
            left -= t
        else:
            out.append((k, n))
    return out


def cigar_str(ops):
    return "".join(f"{n}{k}" for k, n in ops)


def raw_cigar(rec):
    l_name = rec[8]
    n_cig, = struct.unpack_from("<H", rec, 12)
    return [("MIDNSHP=X"[o & 15], o >> 4) for o in struct.unpack_from(f"<{n_cig}I", rec, 32 + l_name)]


def final_length(canon, min_bq):
    """create_source_read on the canonical record (clip already cut): trailing no-calls / masked bases of the ORIENTED read are stripped."""
    p = bamutil.parse(canon)
    seq, q = p["seq"], p["quals"]
    if p["flag"] & 0x10:
        seq, q = seq[::-1], q[::-1]
    fl = len(seq)
    while fl > 0 and (seq[fl - 1] == "N" or q[fl - 1] < min_bq):
        fl -= 1
    return fl


def check_group(o, group, seen):
    rc, res = canonicalise_with_runs(o, group)
    if rc != 0:
        return 0
    n = 0
    for orig, canon, r in res:
        if canon is None:
            continue
        po, pc = bamutil.parse(orig), bamutil.parse(canon)
        rev = bool(po["flag"] & 0x10)
        assert r["rev"] == rev
        assert r["ref_id"] == (po["ref_id"] if po["pos"] >= 0 else -1)
        if po["flag"] & 0x80:
            assert pc["ref_id"] == po["ref_id"] ^ OTHER_REF_XOR          # the canonical record itself no longer names the contig
        folded = fold(raw_cigar(orig))
        fl = final_length(canon, o.min_input_base_quality)
        simp = truncate(folded[::-1] if rev else folded, fl)
        if fl == 0:
            assert r["runs"] == []
            continue
        want = orc.meth_query_to_ref_positions(cigar_str(simp), po["pos"], rev, cigar_str(folded))
        assert len(want) == fl
        assert expand(r, fl) == want, (cigar_str(raw_cigar(orig)), po["pos"], rev, fl, r, want)
        kinds = {k for k, _ in raw_cigar(orig)}
        seen["rev" if rev else "fwd"] += 1
        seen["clipped_by_mate"] += len(pc["seq"]) < len(po["seq"])
        for k in "DINHS":
            seen[k] += k in kinds
        seen["clip_beside_indel"] += bool(kinds & set("SH")) and bool(kinds & set("DIN"))
        n += 1
    return n


def short_insert_molecule(rng, g):
    """tests/test_canon_core.py's molecules with inserts below the read length: both mates run past each other's start, so the mate clip cuts them."""
    start = rng.randint(10, 3000)
    insert = rng.choice([70, 85, 95, 110])
    major = rng.randrange(len(tcc.C1))
    recs = []
    for strand in "AB":
        for k in range(rng.choice([1, 2, 3])):
            ci = major if rng.random() < 0.8 else rng.randrange(len(tcc.C1))
            c1, c2 = tcc.C1[ci], tcc.C2[ci]
            p2 = max(0, start + insert - tcc.rlen(c2))
            s1 = "".join(tcc.TMPL[(start + i) % 4000] for i in range(tcc.qlen(c1)))
            s2 = "".join(tcc.TMPL[(p2 + i) % 4000] for i in range(tcc.qlen(c2)))
            q1 = [rng.choice([5, 25, 30, 37]) for _ in s1]
            q2 = [rng.choice([5, 25, 30, 37]) for _ in s2]
            fwd = dict(flag=0x1 | 0x2 | 0x20, pos=start, mate_pos=p2)
            rev = dict(flag=0x1 | 0x2 | 0x10, pos=p2, mate_pos=start)
            first, last = (fwd, rev) if strand == "A" else (rev, fwd)
            for seg, d in ((0x40, first), (0x80, last)):
                is_fwd = d is fwd
                s, q, c, mc = (s1, q1, c1, c2) if is_fwd else (s2, q2, c2, c1)
                recs.append(bamutil.make_record(f"m{g}{strand}{k}", s, q, flag=d["flag"] | seg, ref_id=1, pos=d["pos"], cigar=c, mate_ref=1, mate_pos=d["mate_pos"],
                                                tlen=insert if is_fwd else -insert, tags=[("MI", "Z", f"{g}/{strand}"), ("RX", "Z", "ACG-TTA"), ("MC", "Z", mc)]))
    return recs


def new_seen():
    return dict(fwd=0, rev=0, clipped_by_mate=0, D=0, I=0, N=0, H=0, S=0, clip_beside_indel=0)


@pytest.mark.parametrize("seed", range(4))
def test_runs_of_canonical_duplex_records_equal_query_to_ref_positions(seed):
    rng = random.Random(4100 + seed)
    seen, n = new_seen(), 0
    for g in range(120):
        o = tcc.options(rng)
        mol = tcc.duplex_indel_molecule(rng, g) if g % 2 else short_insert_molecule(rng, g)
        if mol:
            n += check_group(o, mol, seen)
    print(n, seen)
    assert n > 300
    assert all(v > 10 for v in seen.values()), seen      # forward, reverse, cut by the mate clip, D I N, hard and soft clips, clips beside an indel


@pytest.mark.parametrize("seed", range(3))
def test_runs_of_hostile_records(seed):
    """The hostile groups of the general-path fuzz: whatever the form accepts must satisfy the claim."""
    rng = random.Random(7300 + seed)
    seen, n = new_seen(), 0
    for g in range(150):
        o = tcc.options(rng)
        mol = tcc.fuzz.random_group(rng, g, "duplex", rng.random() < 0.5)
        if mol:
            n += check_group(o, mol, seen)
    assert n > 40


def test_crafted_runs():
    """By hand: `5S20M2D10M3I12M4H` (l_seq 50) at pos 1000."""
    o = fgx_opts.defaults(kind=1, min_input_base_quality=0)
    o.duplex_min_reads[0], o.duplex_min_reads[1], o.duplex_min_reads[2] = 1, 1, 0
    c1, c2 = "5S20M2D10M3I12M4H", "50M"
    s1, s2 = "ACGT" * 12 + "AC", "TGCA" * 12 + "TG"
    for rev1 in (False, True):
        f1 = 0x1 | 0x40 | (0x10 if rev1 else 0x20)
        f2 = 0x1 | 0x80 | (0x20 if rev1 else 0x10)
        mol = [bamutil.make_record("t", s1, [30] * 50, flag=f1, ref_id=2, pos=1000, cigar=c1, mate_ref=2, mate_pos=3000, tags=[("MI", "Z", "7/A"), ("MC", "Z", c2)]),
               bamutil.make_record("t", s2, [30] * 50, flag=f2, ref_id=2, pos=3000, cigar=c2, mate_ref=2, mate_pos=1000, tags=[("MI", "Z", "7/A"), ("MC", "Z", c1)])]
        rc, res = canonicalise_with_runs(o, mol)
        assert rc == 0
        r = res[0][2]
        assert r["ref_id"] == 2 and r["rev"] == rev1
        if not rev1:      # folded: 25M 2D 10M 3I 16M — the leading clip lies BEFORE pos on the reference's one-M view
            assert r["runs"] == [(0, 25, 1000), (25, 10, 1027), (38, 12, 1037)]        # (the 4 hard-clipped bases are not in the read: truncated to l_seq 50)
        else:             # span = 25 + 2 + 10 + 16 = 53: the first column lies at 1052 and the walk runs down the reversed CIGAR 16M 3I 10M 2D 25M
            assert r["runs"] == [(0, 16, 1052), (19, 10, 1036), (29, 21, 1024)]
        assert res[1][2]["ref_id"] == 2 and res[1][2]["runs"] == [(0, 50, 3049 if not rev1 else 3000)]
