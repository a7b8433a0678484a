#!/usr/bin/env python3
"""The methylation-aware mode in the device-resident pipeline: simulate-shaped families resident in HBM, a random genome under their coordinates
(contig 0; the simulator places molecule m at 1000 + 1000 m), EM-Seq mode, through `fgx_process_batch_device`.  Prints one JSON line.

  --caller simplex (default; the streaming kernels of simplex_deep.inc): raw reads/s with the mode and with the mode off (the record / column split
      pipeline on the same batch).
  --caller duplex (k_family_wave<1, 1> + duplex_meth.inc; BASELINE configs[2] shape, 6 + 6 pairs per molecule): `em_seq`, `mode_off` on the same
      batch (the ceiling: the same kernels without the annotation), and `host_entry_opt_out`: the first --host-sample molecules of the batch through
      the host entry with FGX_METH_DEVICE=0 — the general path, which was the only way such a caller ran before —, --opt-out-runs times.  The simulated
      reads are unrelated to the random genome, so about one read base in sixteen is rewritten: the normalisation and the artifact rule are live.

  --clip-fraction F (both callers): that share of the reads carries soft clips at both ends (`aSbMcS`, a and c 1 .. 9 bases; pos moves to the first
      aligned base, the mate's MC and mate position follow) — what an aligner gives a bisulfite / EM-Seq library.  The line then also carries
      `clipped_families_on_the_device` (fgx_debug_last_meth_clipped).  --repeats N: the em_seq / mode_off legs N times, alternating.
  --indel-fraction F (both callers; instead of --clip-fraction): that share of the reads carries a deletion (`aMdDbM`, d 1 .. 3 bases; the mate's MC follows).
      In the mode such a family / molecule is deferred by the first device pass; with FGX_METH_CANON=1 in the environment the canonical second pass decides it on the
      device.  The line carries `canonicalised_molecules` (fgx_debug_last_deferral) beside `deferred_families`.
  --max-reads-per-strand N (duplex): the caller's per-strand read cap in every leg — k_family_wave<1, 1, 1> in the mode, <1, 0, 1> with the mode off; the
      line carries the cap.  With 6 + 6 pairs per molecule a cap below 6 bites every molecule.  Together with --host-entry-only (FGX_LIB on a library whose
      device pipeline defers such molecules): what its users got, the device pass and the deferred subset on the general path.
  --batch-cache DIR: a comparison of two libraries (FGX_LIB) alternates PROCESSES over one batch; simulating and clipping 16 M reads on the host takes
      minutes per process and the measurement a second, so the batch and the genome are kept as .npy files in DIR (the caller's to delete) between them.

  python tools/bench_methylation_device.py [--caller duplex] [--families 1000000] [--depth 8] [--steps 5] [--clip-fraction 0.1]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fgumi_amd import DuplexConsensusCaller, MethylationMode, VanillaUmiConsensusCaller, VanillaUmiConsensusOptions, lib, simulate_grouped_reads  # noqa: E402


def timed(c, dg, steps):
    c.process_batch_device(dg)                     # warm-up (allocations, images)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = c.process_batch_device(dg)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, out


def clip_reads(g, fraction, seed=11):
    """`fraction` of the batch's reads soft-clipped at both ends, in place of their single `<L>M` op.  The simulator writes mates next to each other
    (records 2j, 2j + 1) and ends every record with MC:Z:<L>M MQ:c; clips of one digit each keep a three-digit aligned block of a 118 .. 999-base read, so
    every rewritten MC value is 4 bytes longer and the new blob is the old one with 8 bytes inserted behind the op of a clipped read and 4 before the
    NUL of its mate's MC."""
    from fgumi_amd import GroupedReads
    n = int(g.n_rec)
    assert n % 2 == 0
    # (a generator per array: the first k families of a larger batch get the same clips as a batch of k families)
    clipped = np.random.default_rng(seed).random(n) < fraction
    lead, trail = np.random.default_rng(seed + 1).integers(1, 10, n), np.random.default_rng(seed + 2).integers(1, 10, n)
    off, ln = g.rec_off.astype(np.int64), g.rec_len.astype(np.int64)
    blob = g.blob.copy()

    def u32_at(p):
        return blob[p[:, None] + np.arange(4)].astype(np.uint32) @ (1 << (8 * np.arange(4, dtype=np.uint32)))

    def put_u32(p, v):
        blob[p[:, None] + np.arange(4)] = ((v[:, None].astype(np.uint32) >> (8 * np.arange(4, dtype=np.uint32))) & 0xFF).astype(np.uint8)
    L = u32_at(off[:1] + 16)[0]
    assert 118 <= L <= 999, L
    cig = off + 32 + blob[off + 8].astype(np.int64)
    mc = off + ln - 4 - 2 - 3                                   # the digits of MC:Z:<L>M, ahead of "M", NUL and MQ:c
    # every record is the simulator's: one `<L>M` op, and MC:Z:<L>M where the tail of the record should hold it
    want_mc = np.frombuffer(b"MCZ%dM\0" % L, dtype=np.uint8)
    assert (blob[off + 12] == 1).all() and (blob[off + 13] == 0).all() and (u32_at(cig) == (L << 4)).all() and \
        (blob[(mc - 3)[:, None] + np.arange(len(want_mc))] == want_mc).all(), "not the simulator's record layout"
    c = np.flatnonzero(clipped)
    m = c ^ 1                                                   # their mates
    a, z = lead[c].astype(np.uint32), trail[c].astype(np.uint32)
    al = (L - a - z).astype(np.uint32)
    put_u32(cig[c], (a << 4) | 4)
    put_u32(off[c] + 4, u32_at(off[c] + 4) + a)                 # pos: the first aligned base
    put_u32(off[m] + 24, u32_at(off[m] + 24) + a)               # ... which is the mate's mate position
    blob[off[c] + 12] = 3                                       # n_cigar_op
    text = np.stack([48 + a, np.full(len(c), ord("S")), 48 + al // 100, 48 + al // 10 % 10, 48 + al % 10, np.full(len(c), ord("M")), 48 + z, np.full(len(c), ord("S"))], axis=1).astype(np.uint8)
    blob[mc[m][:, None] + np.arange(4)] = text[:, :4]
    ops = np.stack([al << 4, (z << 4) | 4], axis=1).astype("<u4").view(np.uint8).reshape(len(c), 8)
    at = np.concatenate([np.repeat(cig[c] + 4, 8), np.repeat(mc[m] + 4, 4)])
    vals = np.concatenate([ops.reshape(-1), text[:, 4:].reshape(-1)])
    grow = np.zeros(n, dtype=np.int64)
    grow[c] += 8
    np.add.at(grow, m, 4)
    put_u32(off - 4, (ln + grow).astype(np.uint32))             # block_size
    order = np.argsort(at, kind="stable")
    new_blob = np.insert(blob, at[order], vals[order])
    new_off = off + np.concatenate([[0], np.cumsum(grow)[:-1]])
    return GroupedReads(new_blob, new_off.astype(g.rec_off.dtype), (ln + grow).astype(g.rec_len.dtype), g.grp_first), int(clipped.sum())


def indel_reads(g, fraction, seed=21):
    """`fraction` of the batch's reads with a deletion, `aMdDbM` in place of their single `<L>M` op (same bases, same position).  a and b keep two digits each
    (three for b in reads of 199 bases and more), so every rewritten MC value grows by the same number of bytes: the new blob is the old one with 8 bytes
    inserted behind the op of an indel read and the longer text in its mate's MC, as in clip_reads."""
    from fgumi_amd import GroupedReads
    n = int(g.n_rec)
    assert n % 2 == 0
    chosen = np.random.default_rng(seed).random(n) < fraction
    off, ln = g.rec_off.astype(np.int64), g.rec_len.astype(np.int64)
    blob = g.blob.copy()

    def u32_at(p):
        return blob[p[:, None] + np.arange(4)].astype(np.uint32) @ (1 << (8 * np.arange(4, dtype=np.uint32)))

    def put_u32(p, v):
        blob[p[:, None] + np.arange(4)] = ((v[:, None].astype(np.uint32) >> (8 * np.arange(4, dtype=np.uint32))) & 0xFF).astype(np.uint8)
    L = int(u32_at(off[:1] + 16)[0])
    assert 118 <= L <= 999, L
    a_lo, a_hi = (10, 99) if L >= 199 else (L - 99, 99)
    bd = 3 if L >= 199 else 2
    a_all = np.random.default_rng(seed + 1).integers(a_lo, a_hi + 1, n)
    d_all = np.random.default_rng(seed + 2).integers(1, 4, n)
    cig = off + 32 + blob[off + 8].astype(np.int64)
    mc = off + ln - 4 - 2 - 3
    want_mc = np.frombuffer(b"MCZ%dM\0" % L, dtype=np.uint8)
    assert (blob[off + 12] == 1).all() and (blob[off + 13] == 0).all() and (u32_at(cig) == (L << 4)).all() and \
        (blob[(mc - 3)[:, None] + np.arange(len(want_mc))] == want_mc).all(), "not the simulator's record layout"
    c = np.flatnonzero(chosen)
    m = c ^ 1
    a, d = a_all[c].astype(np.uint32), d_all[c].astype(np.uint32)
    b = (L - a).astype(np.uint32)
    put_u32(cig[c], a << 4)
    blob[off[c] + 12] = 3
    bt = [48 + b // 100, 48 + b // 10 % 10, 48 + b % 10] if bd == 3 else [48 + b // 10, 48 + b % 10]
    text = np.stack([48 + a // 10, 48 + a % 10, np.full(len(c), ord("M")), 48 + d, np.full(len(c), ord("D"))] + bt + [np.full(len(c), ord("M"))], axis=1).astype(np.uint8)
    blob[mc[m][:, None] + np.arange(4)] = text[:, :4]           # over "<L>M"; the rest is inserted behind it
    extra = text.shape[1] - 4
    ops = np.stack([(d << 4) | 2, b << 4], axis=1).astype("<u4").view(np.uint8).reshape(len(c), 8)
    at = np.concatenate([np.repeat(cig[c] + 4, 8), np.repeat(mc[m] + 4, extra)])
    vals = np.concatenate([ops.reshape(-1), text[:, 4:].reshape(-1)])
    grow = np.zeros(n, dtype=np.int64)
    grow[c] += 8
    np.add.at(grow, m, extra)
    put_u32(off - 4, (ln + grow).astype(np.uint32))
    order = np.argsort(at, kind="stable")
    new_blob = np.insert(blob, at[order], vals[order])
    new_off = off + np.concatenate([[0], np.cumsum(grow)[:-1]])
    return GroupedReads(new_blob, new_off.astype(g.rec_off.dtype), (ln + grow).astype(g.rec_len.dtype), g.grp_first), int(chosen.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--caller", choices=["simplex", "duplex"], default="simplex")
    ap.add_argument("--families", type=int, default=1000000)
    ap.add_argument("--depth", type=int, default=None, help="pairs per family (simplex: 8) / per molecule, both strands (duplex: 12 = 6 + 6)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=50000, help="duplex: molecules of the opt-out leg (the first ones of the batch)")
    ap.add_argument("--opt-out-runs", type=int, default=3)
    ap.add_argument("--clip-fraction", type=float, default=0.0, help="share of the reads that carries soft clips at both ends")
    ap.add_argument("--indel-fraction", type=float, default=0.0, help="share of the reads that carries a deletion (not together with --clip-fraction)")
    ap.add_argument("--repeats", type=int, default=1, help="runs of the em_seq / mode_off legs, alternating (the line then holds lists)")
    ap.add_argument("--max-reads-per-strand", type=int, default=None, help="duplex: --max-reads-per-strand of the caller, in every leg")
    ap.add_argument("--batch-cache", default=None, help="directory that keeps the simulated (and clipped) batch and the genome between runs of the same shape")
    ap.add_argument("--host-entry-only", action="store_true", help="only the host-entry leg over the first --host-sample families (device pass + deferred subset)")
    a = ap.parse_args()
    duplex = a.caller == "duplex"
    depth = a.depth if a.depth is not None else (12 if duplex else 8)
    import ctypes as C
    lib.fgx_debug_last_meth_device.restype = C.c_uint32
    lib.fgx_debug_last_meth_device.argtypes = [C.c_void_p]
    lib.fgx_debug_last_meth_clipped.restype = C.c_uint32
    lib.fgx_debug_last_meth_clipped.argtypes = [C.c_void_p]
    sim = dict(family_size=depth, duplex=1) if duplex else dict(family_size=depth)
    from fgumi_amd import GroupedReads
    assert not (a.clip_fraction > 0 and a.indel_fraction > 0), "--clip-fraction or --indel-fraction"
    assert a.max_reads_per_strand is None or duplex, "--max-reads-per-strand is the duplex caller's"
    key = os.path.join(a.batch_cache, f"{a.caller}_{a.families}_{depth}_{a.clip_fraction}" + (f"_indel{a.indel_fraction}" if a.indel_fraction > 0 else "")) if a.batch_cache else None
    lib.fgx_debug_last_deferral.restype = None
    lib.fgx_debug_last_deferral.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]

    def canonicalised(c):
        d2 = (C.c_uint64 * 2)()
        lib.fgx_debug_last_deferral(c._h, d2)
        return int(d2[1])
    if key and os.path.exists(key + "_genome.npy"):
        g = GroupedReads(*[np.load(f"{key}_{f}.npy") for f in ("blob", "rec_off", "rec_len", "grp_first")])
        n_clipped = int(np.load(key + "_n_clipped.npy"))
        genome = np.load(key + "_genome.npy").tobytes()
    else:
        g = simulate_grouped_reads(a.families, **sim)
        n_clipped = 0
        if a.clip_fraction > 0:
            g, n_clipped = clip_reads(g, a.clip_fraction)
        if a.indel_fraction > 0:
            g, n_clipped = indel_reads(g, a.indel_fraction)
        rng = np.random.default_rng(7)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=1000 + a.families * 1000 + 2000, dtype=np.uint8)].tobytes()
        if key:
            try:
                os.makedirs(a.batch_cache, exist_ok=True)
                for f in ("blob", "rec_off", "rec_len", "grp_first"):
                    np.save(f"{key}_{f}.npy", getattr(g, f))
                np.save(key + "_n_clipped.npy", np.int64(n_clipped))
                np.save(key + "_genome.npy", np.frombuffer(genome, dtype=np.uint8))   # (written last: its presence says the batch is complete)
            except OSError as e:
                print(f"batch cache not written: {e}", file=sys.stderr)
    dg = g.to_device()
    n_reads = int(g.n_rec)
    what = f"{a.families} duplex molecules x {depth // 2} + {depth - depth // 2} pairs x 150 bp" if duplex else f"{a.families} families x {depth} pairs x 150 bp"
    line = {"workload": f"{what}, device-resident, EM-Seq mode, {len(genome) >> 20} MiB genome in HBM", "caller": a.caller, "raw_reads": n_reads,
            "clip_fraction": a.clip_fraction, "clipped_reads": n_clipped if a.indel_fraction == 0 else 0, "indel_fraction": a.indel_fraction,
            "indel_reads": n_clipped if a.indel_fraction > 0 else 0, "FGX_METH_CANON": os.environ.get("FGX_METH_CANON")}
    if a.max_reads_per_strand is not None:
        line["max_reads_per_strand"] = a.max_reads_per_strand

    def make(mode):
        if duplex:
            return DuplexConsensusCaller("", "A", [1, 1, 1], cell_tag="CB", overlapping_consensus=True, methylation_mode=int(mode) if mode is not None else 0,
                                         max_reads_per_strand=a.max_reads_per_strand)
        kw = dict(min_reads=1, min_consensus_base_quality=2, cell_tag="CB")
        if mode is not None:
            kw["methylation_mode"] = mode
        return VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(**kw), overlapping_consensus=True)

    def head(n_s):
        """The first n_s families of the batch (a prefix of every array)."""
        from fgumi_amd import GroupedReads
        r = int(g.grp_first[n_s])
        end = int(g.rec_off[r - 1]) + int(g.rec_len[r - 1])
        return GroupedReads(g.blob[:end].copy(), g.rec_off[:r].copy(), g.rec_len[:r].copy(), g.grp_first[:n_s + 1].copy())

    if a.host_entry_only:
        # device pass + deferred subset on the general path: what a batch with deferred families costs through fgx_process_batch
        lib.fgx_debug_last_deferral.restype = None
        lib.fgx_debug_last_deferral.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        n_s = min(a.host_sample, a.families)
        gs = head(n_s)
        c = make(MethylationMode.EmSeq)
        c.set_reference({"chr1": genome}, ["chr1"])
        c.process_batch(head(min(n_s, 2000)))                   # warm-up
        runs = []
        for _ in range(a.opt_out_runs):
            t0 = time.perf_counter()
            out = c.process_batch(gs)
            runs.append(round(int(gs.n_rec) / (time.perf_counter() - t0)))
        d2 = (C.c_uint64 * 2)()
        lib.fgx_debug_last_deferral(c._h, d2)
        line["host_entry"] = {"families": n_s, "raw_reads": int(gs.n_rec), "raw_reads_per_s_runs": runs, "consensus_records": int(out.count), "deferred_families": int(d2[0]),
                              "canonicalised_molecules": int(d2[1]),
                              "clipped_families_on_the_device": int(lib.fgx_debug_last_meth_clipped(c._h))}
        c.close()
        print(json.dumps(line))
        return

    legs = (("em_seq", MethylationMode.EmSeq), ("mode_off", None))
    callers = {}
    for name, mode in legs:
        callers[name] = make(mode)
        if mode is not None:
            callers[name].set_reference({"chr1": genome}, ["chr1"])
    rates = {name: [] for name, _ in legs}
    for _ in range(max(1, a.repeats)):
        for name, mode in legs:
            c = callers[name]
            dt, out = timed(c, dg, a.steps)
            rates[name].append(round(n_reads / dt))
            line[name] = {"ms_per_step": round(dt * 1e3, 2), "raw_reads_per_s": round(n_reads / dt), "consensus_records": int(out.count), "output_bytes": int(out.data_len),
                          "deferred_families": int(out.n_deferred),
                          ("molecules_in_the_mode_on_the_device" if duplex else "families_on_the_streaming_kernels"): int(lib.fgx_debug_last_meth_device(c._h)),
                          "clipped_families_on_the_device": int(lib.fgx_debug_last_meth_clipped(c._h)), "canonicalised_molecules": canonicalised(c)}
            if duplex:
                line[name]["kernel_ms"] = round(float(c.last_timing["kernels"]), 2)
    for name, _ in legs:
        if a.repeats > 1:
            line[name]["raw_reads_per_s_runs"] = rates[name]
        callers[name].close()
    if duplex and a.clip_fraction == 0 and a.indel_fraction == 0:
        # the same molecules (the simulator is a function of the molecule's index) through the host entry with the device mode switched off
        n_s = min(a.host_sample, a.families)
        gs = simulate_grouped_reads(n_s, **sim)
        os.environ["FGX_METH_DEVICE"] = "0"
        try:
            c = make(MethylationMode.EmSeq)
            c.set_reference({"chr1": genome}, ["chr1"])
            c.process_batch(gs.subset(0, min(n_s, 2000)))       # warm-up
            runs = []
            for _ in range(a.opt_out_runs):
                t0 = time.perf_counter()
                out = c.process_batch(gs)
                dt = time.perf_counter() - t0
                runs.append(round(int(gs.n_rec) / dt))
            assert int(lib.fgx_debug_last_meth_device(c._h)) == 0
            c.close()
        finally:
            del os.environ["FGX_METH_DEVICE"]
        line["host_entry_opt_out"] = {"molecules": n_s, "raw_reads": int(gs.n_rec), "raw_reads_per_s_runs": runs, "consensus_records": int(out.count)}
        line["em_seq_over_opt_out_max"] = round(line["em_seq"]["raw_reads_per_s"] / max(runs), 1)
        line["em_seq_over_mode_off"] = round(line["em_seq"]["raw_reads_per_s"] / line["mode_off"]["raw_reads_per_s"], 3)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
