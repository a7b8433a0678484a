#!/usr/bin/env python3
"""--max-reads-per-strand in the device-resident pipeline: simulate-shaped molecules resident in HBM through `fgx_process_batch_device`, with the cap and
with the cap off on the same batch.  Prints one JSON line.

  duplex: 500 000 molecules of 6 + 6 pairs x 150 bp (BASELINE configs[2] shape) at a cap of 3 — every molecule has a read set above the cap;
  codec:  the CODEC benchmark shape (1 000 000 molecules of 4 pairs of 2 x 300 bp, insert N(350, 60)) at a cap of 2.

Per caller: `cap_on` and `cap_off` (ms per step, raw reads/s, consensus records, molecules deferred).  A library whose device pipeline does NOT decide
the cap defers the capped molecules — every one of them here —, and what its users get is the host entry: when `cap_on` defers molecules the tool also
times the first --host-sample molecules of the batch through `fgx_process_batch` (`cap_on_host_entry`, --host-runs runs).  FGX_LIB selects the library,
so the same tool measures the commit before this mode existed.

  --parent-line FILE: the line this tool printed under the parent commit's library; with it the tool writes the three legs the profile file keeps
      (cap on at this commit, cap off at this commit, cap on at the parent) and their ratios per caller.

Timed region: barrier + device synchronize on both sides of the K steps, one warm-up pass ahead of them (allocations, table images), as bench.py does.

  python tools/bench_strand_cap.py [--callers duplex,codec] [--steps 5] [--parent-line parent.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fgumi_amd import CodecConsensusCaller, CodecConsensusOptions, DuplexConsensusCaller, simulate_grouped_reads  # noqa: E402

SHAPES = {"duplex": dict(molecules=500000, cap=3, sim=dict(family_size=12, duplex=1), what="duplex molecules x 6 + 6 pairs x 150 bp"),
          "codec": dict(molecules=1000000, cap=2, sim=dict(family_size=4, read_length=300, insert_mean=350, insert_sd=60, codec=1), what="CODEC molecules x 4 pairs of 2 x 300 bp, insert N(350, 60)")}


def make(caller, cap):
    if caller == "duplex":
        return DuplexConsensusCaller("", "A", [1], cell_tag="CB", overlapping_consensus=True, max_reads_per_strand=cap)
    return CodecConsensusCaller("", "A", CodecConsensusOptions(produce_per_base_tags=True, cell_tag="CB", max_reads_per_strand=cap))


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
    ap.add_argument("--callers", default="duplex,codec")
    ap.add_argument("--molecules", type=int, default=None, help="molecules of the batch (default: the shape's)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-sample", type=int, default=50000, help="molecules of the host-entry leg (the first ones of the batch)")
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--parent-line", default=None)
    a = ap.parse_args()
    line = {"library": os.path.basename(os.environ.get("FGX_LIB") or "libfgumi_amd.so"), "steps": a.steps}
    for caller in a.callers.split(","):
        S = SHAPES[caller]
        n = a.molecules or S["molecules"]
        c = make(caller, None)
        dg = c.simulate_on_device(n, **S["sim"])
        n_reads = int(dg.n_rec)
        res = {"workload": f"{n} {S['what']}, device-resident", "cap": S["cap"], "raw_reads": n_reads}
        for name, cap in (("cap_off", None), ("cap_on", S["cap"])):
            if cap is not None:
                c.close()
                c = make(caller, cap)
            dt, out = timed(c, dg, a.steps, a.warmup)
            res[name] = {"ms_per_step": round(dt * 1e3, 2), "raw_reads_per_s": round(n_reads / dt), "consensus_records": int(out.count), "output_bytes": int(out.data_len),
                         "deferred_molecules": int(out.n_deferred), "kernel_ms": round(float(c.last_timing["kernels"]), 2)}
        if res["cap_on"]["deferred_molecules"]:
            # the device pipeline left capped molecules to the general path: what a user of this library gets is the host entry
            gs = simulate_grouped_reads(min(a.host_sample, n), **S["sim"])
            c.process_batch(gs.subset(0, min(gs.n_grp, 2000)))            # warm-up
            runs = []
            for _ in range(a.host_runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = c.process_batch(gs)
                torch.cuda.synchronize()
                runs.append(round(int(gs.n_rec) / (time.perf_counter() - t0)))
            res["cap_on_host_entry"] = {"molecules": int(gs.n_grp), "raw_reads": int(gs.n_rec), "raw_reads_per_s_runs": runs, "consensus_records": int(out.count)}
        c.close()
        del dg
        torch.cuda.empty_cache()
        line[caller] = res
    if a.parent_line:
        parent = json.loads(open(a.parent_line).read().strip().splitlines()[-1])
        legs = {"head": line, "parent": parent, "three_legs": {}}
        for caller in a.callers.split(","):
            h, p = line[caller], parent[caller]
            # the parent's cap-on figure: its device entry alone decides nothing of such a batch, so the host entry's best run stands for it
            p_on = max(p["cap_on_host_entry"]["raw_reads_per_s_runs"]) if "cap_on_host_entry" in p else p["cap_on"]["raw_reads_per_s"]
            legs["three_legs"][caller] = {"cap_on_raw_reads_per_s": h["cap_on"]["raw_reads_per_s"], "cap_off_raw_reads_per_s": h["cap_off"]["raw_reads_per_s"],
                                          "parent_cap_on_raw_reads_per_s": p_on, "cap_on_over_parent": round(h["cap_on"]["raw_reads_per_s"] / p_on, 1),
                                          "cap_on_over_cap_off": round(h["cap_on"]["raw_reads_per_s"] / h["cap_off"]["raw_reads_per_s"], 3),
                                          "deferred_molecules_cap_on": h["cap_on"]["deferred_molecules"], "parent_deferred_molecules_cap_on": p["cap_on"]["deferred_molecules"]}
        line = legs
    print(json.dumps(line))


if __name__ == "__main__":
    main()
