#!/usr/bin/env python3
"""--max-reads on deep simplex families in the device-resident pipeline: simulate-shaped families resident in HBM through `fgx_process_batch_device`, with the cap
and with the cap off on the same batch.  Prints one JSON line.

  deep:        200 000 families of 40 .. 150 pairs x 150 bp (80 .. 300 records: every family is the streaming kernels', simplex_deep.inc) at a cap of 50;
  methylation: 1 000 000 families of 8 pairs, EM-Seq mode (a random genome under their coordinates, as tools/bench_methylation_device.py), at a cap of 3.

Per leg: `cap_on` and `cap_off` (ms per step, raw reads/s, consensus records, families deferred, families the streaming kernels finished).  A library whose
streaming kernels refuse a biting cap hands the capped families on — above 128 records, and in the methylation-aware mode, to the deferred list —, and what its
users get is the host entry: when `cap_on` defers families the tool also times the first --host-sample families of the batch through `fgx_process_batch`
(`cap_on_host_entry`, --host-runs runs).  FGX_LIB selects the library, so the same tool measures the commit before the kernels took the cap.

  --parent-line FILE: the line this tool printed under the parent commit's library; with it the tool writes the three legs the profile file keeps
      (cap on at this commit, cap off at this commit, cap on at the parent) and their ratios per leg.

Timed region: device synchronize on both sides of the K steps, one warm-up pass ahead of them (allocations, table images), as bench.py does.

  python tools/bench_max_reads.py [--legs deep,methylation] [--families N] [--steps 5] [--parent-line parent.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fgumi_amd import MethylationMode, VanillaUmiConsensusCaller, VanillaUmiConsensusOptions, lib, simulate_grouped_reads  # noqa: E402

SHAPES = {"deep": dict(families=200000, cap=50, sim=dict(family_size=40, family_size_max=150), meth=False, what="families x 40 .. 150 pairs x 150 bp"),
          "methylation": dict(families=1000000, cap=3, sim=dict(family_size=8), meth=True, what="families x 8 pairs x 150 bp, EM-Seq mode")}


def make(S, cap, genome):
    kw = dict(min_reads=1, max_reads=cap, min_consensus_base_quality=2, cell_tag="CB")
    if S["meth"]:
        kw["methylation_mode"] = MethylationMode.EmSeq
    c = VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(**kw), overlapping_consensus=True)
    if S["meth"]:
        c.set_reference({"chr1": genome}, ["chr1"])
    return c


def timed(c, dg, steps, warmup):
    out = None
    for _ in range(warmup):
        out = c.process_batch_device(dg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = c.process_batch_device(dg)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="deep,methylation")
    ap.add_argument("--families", type=int, default=None, help="families of the batch (default: the shape's)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-sample", type=int, default=2000, help="families of the host-entry leg (the first ones of the batch)")
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--parent-line", default=None)
    a = ap.parse_args()
    for f in ("fgx_debug_last_deep_families", "fgx_debug_last_meth_device"):
        getattr(lib, f).restype = C.c_uint32
        getattr(lib, f).argtypes = [C.c_void_p]
    line = {"library": os.path.basename(os.environ.get("FGX_LIB") or "libfgumi_amd.so"), "steps": a.steps}
    for leg in a.legs.split(","):
        S = SHAPES[leg]
        n = a.families or S["families"]
        genome = None
        if S["meth"]:      # contig 0; the simulator places molecule m at 1000 + 1000 m
            genome = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(7).integers(0, 4, size=1000 + n * 1000 + 2000, dtype=np.uint8)].tobytes()
        c = make(S, None, genome)
        dg = c.simulate_on_device(n, **S["sim"])
        n_reads = int(dg.n_rec)
        res = {"workload": f"{n} {S['what']}, device-resident", "cap": S["cap"], "raw_reads": n_reads}
        for name, cap in (("cap_off", None), ("cap_on", S["cap"])):
            if cap is not None:
                c.close()
                c = make(S, cap, genome)
            dt, out = timed(c, dg, a.steps, a.warmup)
            res[name] = {"ms_per_step": round(dt * 1e3, 2), "raw_reads_per_s": round(n_reads / dt), "consensus_records": int(out.count), "output_bytes": int(out.data_len),
                         "deferred_families": int(out.n_deferred), "kernel_ms": round(float(c.last_timing["kernels"]), 2),
                         "families_on_the_streaming_kernels": int(lib.fgx_debug_last_meth_device(c._h) if S["meth"] else lib.fgx_debug_last_deep_families(c._h))}
        if res["cap_on"]["deferred_families"]:
            # the device pipeline left capped families to the general path: what a user of this library gets is the host entry
            gs = simulate_grouped_reads(min(a.host_sample, n), **S["sim"])
            c.process_batch(gs.subset(0, min(gs.n_grp, 100)))            # warm-up
            runs = []
            for _ in range(a.host_runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = c.process_batch(gs)
                torch.cuda.synchronize()
                runs.append(round(int(gs.n_rec) / (time.perf_counter() - t0)))
            res["cap_on_host_entry"] = {"families": int(gs.n_grp), "raw_reads": int(gs.n_rec), "raw_reads_per_s_runs": runs, "consensus_records": int(out.count)}
        c.close()
        del dg
        torch.cuda.empty_cache()
        line[leg] = res
    if a.parent_line:
        parent = json.loads(open(a.parent_line).read().strip().splitlines()[-1])
        legs = {"head": line, "parent": parent, "three_legs": {}}
        for leg in a.legs.split(","):
            h, p = line[leg], parent[leg]
            # the parent's cap-on figure: its device entry alone does not finish such a batch, so the host entry's best run stands for it
            p_on = max(p["cap_on_host_entry"]["raw_reads_per_s_runs"]) if "cap_on_host_entry" in p else p["cap_on"]["raw_reads_per_s"]
            legs["three_legs"][leg] = {"cap_on_raw_reads_per_s": h["cap_on"]["raw_reads_per_s"], "cap_off_raw_reads_per_s": h["cap_off"]["raw_reads_per_s"],
                                       "parent_cap_on_raw_reads_per_s": p_on, "cap_on_over_parent": round(h["cap_on"]["raw_reads_per_s"] / p_on, 1),
                                       "cap_on_over_cap_off": round(h["cap_on"]["raw_reads_per_s"] / h["cap_off"]["raw_reads_per_s"], 3),
                                       "deferred_families_cap_on": h["cap_on"]["deferred_families"], "parent_deferred_families_cap_on": p["cap_on"]["deferred_families"]}
        line = legs
    print(json.dumps(line))


if __name__ == "__main__":
    main()
