"""reject_core.h `canon_simplex_family` on the host: the canonical form of simplex families with indel / skip / pad CIGARs — the claim of
tests/test_canon_core.py, for the simplex caller, with the methylation-aware mode OFF, through the oracle alone: for every in-scope family F, the
reference's result for the canonical family C(F) — every read one `<len>M` op, no MC tag, overlap-corrected and clipped bases, R2 on another reference
id — plus the statistics the canonicalisation counted itself (reads the alignment filter dropped, the overlap pre-step's CorrectionStats) IS the
reference's result for F: bytes, record count, the 28 counters.  The order of the reference's gates is part of the claim: a read the reference counts as
InsufficientReads must not be counted as MinorityAlignment.

Second claim (the methylation-aware mode's hand-over): the reference runs emitted beside every surviving record expand to the oracle's
query_to_ref_positions on CIGARs this test rebuilds itself from the original record (tests/test_canon_runs.py has the duplex form's)."""
import ctypes as C
import random

import numpy as np
import pytest

import bamutil
import fgx_opts
import orc
import test_canon_core as tcc
import test_canon_runs as tcr
import test_general_path_fuzz as fuzz
from fgumi_amd import GroupedReads
from fgumi_amd._lib import lib

MINORITY = 3 + 6


def canonicalise(o, group, with_runs=False):
    """-> (status, canonical records, delta5[, per input record: (original, canonical or None, runs or None)])"""
    g = GroupedReads.from_groups([group])
    out = np.zeros(g.blob.size + 16, dtype=np.uint8)
    out_len = np.zeros(max(1, g.n_rec), dtype=np.uint32)
    delta = np.zeros(5, dtype=np.uint64)
    runs = np.zeros(max(1, g.n_rec) * tcr.WORDS, dtype=np.uint32)
    rc = lib.fgx_canon_simplex_host(C.addressof(o), g.blob.ctypes.data, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, out.ctypes.data, out_len.ctypes.data,
                                    delta.ctypes.data, runs.ctypes.data)
    recs = [bytes(out[int(g.rec_off[i]):int(g.rec_off[i]) + int(out_len[i])]) for i in range(g.n_rec) if out_len[i]] if rc == 0 else []
    if not with_runs:
        return rc, recs, delta
    res = []
    for i in range(g.n_rec):
        if rc != 0 or not out_len[i]:
            res.append((group[i], None, None))
            continue
        w = runs[i * tcr.WORDS:(i + 1) * tcr.WORDS]
        n = int(w[1]) & 0x7FFFFFFF
        rr = [(int(w[2 + 4 * k]), int(w[3 + 4 * k]), int(np.array([w[4 + 4 * k], w[5 + 4 * k]], dtype=np.uint32).view(np.int64)[0])) for k in range(n)]
        res.append((group[i], bytes(out[int(g.rec_off[i]):int(g.rec_off[i]) + int(out_len[i])]), dict(ref_id=int(np.int32(w[0])), rev=bool(w[1] >> 31), runs=rr)))
    return rc, recs, delta, res


def oracle(o, groups):
    g = GroupedReads.from_groups(groups)
    return orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=50)


def check_family(o, group, seen=None):
    rc, canon, delta, res = canonicalise(o, group, True)
    if rc != 0:
        return False
    want = oracle(o, [group])
    got = oracle(o, [canon]) if canon else dict(data=b"", count=0, stats=np.zeros(28, dtype=np.uint64))
    assert got["data"] == want["data"], ("records differ", [bamutil.parse(r) for r in group])
    assert got["count"] == want["count"]
    st = got["stats"].copy()
    st[0] += delta[0]; st[2] += delta[0]; st[MINORITY] += delta[0]
    assert not got["stats"][24:28].any()          # the canonical family's mates sit on different references: no second correction
    st[24:28] += delta[1:5]
    assert np.array_equal(st, want["stats"]), (st.tolist(), want["stats"].tolist(), delta.tolist(), [(bamutil.parse(r)["flag"], tcr.cigar_str(tcr.raw_cigar(r))) for r in group])
    for r in canon:
        p = bamutil.parse(r)
        assert p["n_cigar"] == (1 if p["seq"] else 0) and "MC" not in p["tags"]
    # the reference runs of the survivors
    for orig, can, r in res:
        if can is None:
            continue
        po = bamutil.parse(orig)
        rev = bool(po["flag"] & 0x10)
        assert r["rev"] == rev and r["ref_id"] == (po["ref_id"] if po["pos"] >= 0 else -1)
        folded = tcr.fold(tcr.raw_cigar(orig))
        fl = tcr.final_length(can, o.min_input_base_quality)
        if fl == 0:
            continue
        simp = tcr.truncate(folded[::-1] if rev else folded, fl)
        want_pos = orc.meth_query_to_ref_positions(tcr.cigar_str(simp), po["pos"], rev, tcr.cigar_str(folded))
        assert tcr.expand(r, fl) == want_pos, (tcr.cigar_str(tcr.raw_cigar(orig)), po["pos"], rev, fl, r)
        if seen is not None:
            kinds = {k for k, _ in tcr.raw_cigar(orig)}
            seen["rev" if rev else "fwd"] += 1
            seen["clipped_by_mate"] += len(bamutil.parse(can)["seq"]) < len(po["seq"])
            for k in "DINHS":
                seen[k] += k in kinds
            seen["clip_beside_indel"] += bool(kinds & set("SH")) and bool(kinds & set("DIN"))
    return True


CIG = ["{L}M", "{a}M2D{b}M", "{a}M3I{c}M", "4S{d}M", "{a}M10N{b}M", "3S{e}M1D{b}M", "2H{L}M", "{a}M1D{f}M2S"]


def cigar(kind, L):
    a = L // 3
    return CIG[kind].format(L=L, a=a, b=L - a, c=L - a - 3, d=L - 4, e=a - 3, f=L - a - 2)


def simplex_indel_family(rng, g):
    """Fragments (either strand), pairs or overlapping pairs over one template; mostly one alignment per end, a minority alignment now and then; depth 1 .. 7."""
    layout = rng.choice(["frag", "frag_rev", "pair", "pair_overlap", "pair_short_insert"])
    L = rng.randint(30, 90)
    start = rng.randint(10, 3000)
    major1, major2 = rng.randrange(len(CIG)), rng.choice([0, 0, 1, 3])
    recs = []
    for k in range(rng.randint(1, 7)):
        k1 = major1 if rng.random() < 0.8 else rng.randrange(len(CIG))
        k2 = major2 if rng.random() < 0.85 else rng.randrange(len(CIG))
        Lk = L if rng.random() < 0.75 else rng.randint(max(24, L - 12), L)
        c1, c2 = cigar(k1, Lk), cigar(k2, Lk)

        def seq(p, n):
            return "".join(rng.choice("ACGTN") if rng.random() < 0.03 else tcc.TMPL[(p + i) % 4000] for i in range(n))

        def quals(n):
            return [rng.choice([5, 12, 25, 30, 37]) for _ in range(n)]
        if layout in ("frag", "frag_rev"):
            recs.append(bamutil.make_record(f"f{g}_{k}", seq(start, tcc.qlen(c1)), quals(tcc.qlen(c1)), flag=0x10 if layout == "frag_rev" else 0, ref_id=0, pos=start, cigar=c1,
                                            tags=[("MI", "Z", f"{g}"), ("RX", "Z", rng.choice(["ACGT", "ACGA"]))]))
        else:
            insert = {"pair": 3 * L, "pair_overlap": L + rng.randint(0, L // 2), "pair_short_insert": max(10, L - rng.randint(5, 20))}[layout]
            p2 = max(0, start + insert - tcc.rlen(c2))
            r1, r2 = bamutil.pair(f"p{g}_{k}", seq(start, tcc.qlen(c1)), quals(tcc.qlen(c1)), seq(p2, tcc.qlen(c2)), quals(tcc.qlen(c2)), f"{g}", pos1=start, pos2=p2,
                                  cigar1=c1, cigar2=c2, rx="AAC-GGT")
            recs += [r1, r2] if rng.random() < 0.93 else [rng.choice([r1, r2])]
    return recs


def options(rng):
    return fgx_opts.defaults(kind=0, overlapping_consensus=rng.randint(0, 1), min_input_base_quality=rng.choice([0, 10, 20, 30]), produce_per_base_tags=rng.randint(0, 1),
                             min_reads=rng.choice([1, 1, 2, 3]), max_reads=rng.choice([-1, -1, 3]), cell_tag=rng.choice([b"CB", b"\0\0"]))


@pytest.mark.parametrize("seed", range(6))
def test_canonical_indel_families_give_the_original_result(seed):
    rng = random.Random(1900 + seed)
    seen = tcr.new_seen()
    in_scope = dropped = 0
    for g in range(300):
        o = options(rng)
        fam = simplex_indel_family(rng, g)
        if check_family(o, fam, seen):
            in_scope += 1
            dropped += int(canonicalise(o, fam)[2][0])
    print(in_scope, dropped, seen)
    assert in_scope > 220 and dropped > 30, (in_scope, dropped)
    assert all(v > 10 for v in seen.values()), seen


@pytest.mark.parametrize("seed", range(6))
def test_canonical_hostile_families_give_the_original_result_or_stay_out_of_scope(seed):
    rng = random.Random(8000 + seed)
    ok = 0
    for g in range(150):
        o = options(rng)
        fam = fuzz.random_group(rng, g, "simplex", rng.random() < 0.5)
        if not fam:
            continue
        try:
            oracle(o, [fam])
        except RuntimeError:
            continue                                   # (the reference refuses the batch: either path raises downstream)
        ok += check_family(o, fam)
    assert ok > 40, ok


def test_out_of_scope_shapes():
    rng = random.Random(5)
    fam = simplex_indel_family(rng, 0)
    assert canonicalise(fgx_opts.defaults(kind=0, min_reads=1), fam)[0] == 0
    assert canonicalise(fgx_opts.defaults(kind=0, min_reads=1, trim=1), fam)[0] == 1                                        # --trim
    un = bamutil.make_record("u", "ACGT", [30] * 4, flag=0x4, cigar="", tags=[("MI", "Z", "0")])
    assert canonicalise(fgx_opts.defaults(kind=0, min_reads=1), fam + [un])[0] == 1                                         # an unmapped record
    for f in (0x100, 0x800):
        sec = bamutil.make_record("s", "ACGTACGTAC", [30] * 10, flag=f, pos=5, cigar="10M", tags=[("MI", "Z", "0")])
        assert canonicalise(fgx_opts.defaults(kind=0, min_reads=1), fam + [sec])[0] == 1                                    # secondary / supplementary
    big = [bamutil.make_record(f"b{i}", "ACGTACGTAC", [30] * 10, flag=0, pos=5, cigar="4M1D6M", tags=[("MI", "Z", "0")]) for i in range(129)]
    assert canonicalise(fgx_opts.defaults(kind=0, min_reads=1), big)[0] == 1 and canonicalise(fgx_opts.defaults(kind=0, min_reads=1), big[:128])[0] == 0   # more than 128 records
    ops17 = bamutil.make_record("o", "A" * 26, [30] * 26, flag=0, pos=5, cigar="2M1D" * 8 + "10M", tags=[("MI", "Z", "0")])
    assert canonicalise(fgx_opts.defaults(kind=0, min_reads=1), [ops17])[0] == 1                                            # more than 16 ops
    groups17 = [bamutil.make_record(f"g{i}", "A" * 40, [30] * 40, flag=0, pos=5, cigar=f"{2 + i}M1D{38 - i}M", tags=[("MI", "Z", "0")]) for i in range(17)]
    assert canonicalise(fgx_opts.defaults(kind=0, min_reads=1), groups17)[0] == 1 and canonicalise(fgx_opts.defaults(kind=0, min_reads=1), groups17[:16])[0] == 0   # 17 alignment groups
    assert canonicalise(fgx_opts.defaults(kind=0, min_reads=3), big[:2])[0] == 1                                            # a group below --min-reads
