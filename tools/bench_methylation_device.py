#!/usr/bin/env python3
"""The methylation-aware mode in the device-resident pipeline: simulate-shaped families resident in HBM, a random genome under their coordinates
(contig 0; the simulator places molecule m at 1000 + 1000 m), EM-Seq mode, through `fgx_process_batch_device`.  Prints one JSON line.

  --caller simplex (default; the streaming kernels of simplex_deep.inc): raw reads/s with the mode and with the mode off (the record / column split
      pipeline on the same batch).
  --caller duplex (k_family_wave<1, 1> + duplex_meth.inc; BASELINE configs[2] shape, 6 + 6 pairs per molecule): `em_seq`, `mode_off` on the same
      batch (the ceiling: the same kernels without the annotation), and `host_entry_opt_out`: the first --host-sample molecules of the batch through
      the host entry with FGX_METH_DEVICE=0 — the general path, which was the only way such a caller ran before —, --opt-out-runs times.  The simulated
      reads are unrelated to the random genome, so about one read base in sixteen is rewritten: the normalisation and the artifact rule are live.

  python tools/bench_methylation_device.py [--caller duplex] [--families 1000000] [--depth 8] [--steps 5]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--caller", choices=["simplex", "duplex"], default="simplex")
    ap.add_argument("--families", type=int, default=1000000)
    ap.add_argument("--depth", type=int, default=None, help="pairs per family (simplex: 8) / per molecule, both strands (duplex: 12 = 6 + 6)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=50000, help="duplex: molecules of the opt-out leg (the first ones of the batch)")
    ap.add_argument("--opt-out-runs", type=int, default=3)
    a = ap.parse_args()
    duplex = a.caller == "duplex"
    depth = a.depth if a.depth is not None else (12 if duplex else 8)
    import ctypes as C
    lib.fgx_debug_last_meth_device.restype = C.c_uint32
    lib.fgx_debug_last_meth_device.argtypes = [C.c_void_p]
    sim = dict(family_size=depth, duplex=1) if duplex else dict(family_size=depth)
    g = simulate_grouped_reads(a.families, **sim)
    dg = g.to_device()
    n_reads = int(g.n_rec)
    rng = np.random.default_rng(7)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=1000 + a.families * 1000 + 2000, dtype=np.uint8)].tobytes()
    what = f"{a.families} duplex molecules x {depth // 2} + {depth - depth // 2} pairs x 150 bp" if duplex else f"{a.families} families x {depth} pairs x 150 bp"
    line = {"workload": f"{what}, device-resident, EM-Seq mode, {len(genome) >> 20} MiB genome in HBM", "caller": a.caller, "raw_reads": n_reads}

    def make(mode):
        if duplex:
            return DuplexConsensusCaller("", "A", [1, 1, 1], cell_tag="CB", overlapping_consensus=True, methylation_mode=int(mode) if mode is not None else 0)
        kw = dict(min_reads=1, min_consensus_base_quality=2, cell_tag="CB")
        if mode is not None:
            kw["methylation_mode"] = mode
        return VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(**kw), overlapping_consensus=True)

    for name, mode in (("em_seq", MethylationMode.EmSeq), ("mode_off", None)):
        c = make(mode)
        if mode is not None:
            c.set_reference({"chr1": genome}, ["chr1"])
        dt, out = timed(c, dg, a.steps)
        line[name] = {"ms_per_step": round(dt * 1e3, 2), "raw_reads_per_s": round(n_reads / dt), "consensus_records": int(out.count), "output_bytes": int(out.data_len),
                      "deferred_families": int(out.n_deferred),
                      ("molecules_in_the_mode_on_the_device" if duplex else "families_on_the_streaming_kernels"): int(lib.fgx_debug_last_meth_device(c._h))}
        if duplex:
            line[name]["kernel_ms"] = round(float(c.last_timing["kernels"]), 2)
        c.close()
    if duplex:
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
