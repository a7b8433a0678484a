#!/usr/bin/env python3
"""Simplex consensus on unmapped reads in the device-resident pipeline (`fgumi group --allow-unmapped` | `fgumi simplex`): one simulate-shaped batch and its
wholly unmapped twin, both resident in HBM, through `fgx_process_batch_device`; and the host entry of the commit before — whose kernels refuse every family that
holds an unmapped record — on a prefix of the twin.  Writes one JSON document.

  batch:   --families (1 000 000) families x 8 pairs x 150 bp, generated on the device and copied to the host;
  twin:    every record of it unmapped on the host, in vectorised numpy: CIGAR stripped, 0x4 | 0x8 set, mapping quality 0, ref_id / pos -1 — the bytes of each
           record move up by 4 x (records before it);
  legs:    `mapped` and `unmapped`: --repeats (3) x --steps (40) steps each, alternating, in this one call (ms per step, raw reads/s, consensus records, families
           deferred, families the split pipeline finished); the twin does strictly less work per family (no clip, no overlap step), so a twin slower than its
           mapped batch by more than the spread of the mapped leg's own repeats is a finding;
           `parent_host_entry` (with --parent-lib): `fgx_process_batch` of THAT library (a child interpreter: FGX_LIB is read at import) on the first
           --host-sample (50 000) families of the twin, --host-runs (3) runs.
  --bench-ab FILE: lines of `python bench.py` / `python bench.py --depth 2 --depth-max 50` on the parent's library and on this one (each line a JSON object with
           "library" and "args" added by whoever ran them), kept in the same document with the means and the parent's spread.

Timed region: device synchronize on both sides of the K steps, one warm-up pass ahead of them, as bench.py does.

  python tools/bench_unmapped.py [--families N] [--steps 40] [--parent-lib fgumi_amd/parent.so] [--bench-ab lines.jsonl] [--out profiles/unmapped_device_bench.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fgumi_amd import GroupedReads, VanillaUmiConsensusCaller, VanillaUmiConsensusOptions, lib  # noqa: E402

SIM = dict(family_size=8)


def caller():
    return VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(min_reads=1, min_consensus_base_quality=2, cell_tag="CB"), overlapping_consensus=True)


def unmap_all(g):
    """Every record of a batch of one-CIGAR-op records unmapped; no loop over records."""
    off = np.asarray(g.rec_off, dtype=np.int64)
    ln = np.asarray(g.rec_len, dtype=np.int64)
    blob = np.array(g.blob, copy=True)
    assert (blob[off + 12] == 1).all() and (blob[off + 13] == 0).all() and (np.diff(off) > 0).all()
    l_name = blob[off + 8].astype(np.int64)
    blob[off + 14] |= 0x4 | 0x8
    for k in range(8):
        blob[off + k] = 0xFF                                  # ref_id -1, pos -1
    blob[off + 9] = 0
    blob[off + 12] = 0
    new_len = (ln - 4).astype(np.uint32)
    for k in range(4):
        blob[off - 4 + k] = ((new_len >> (8 * k)) & 0xFF).astype(np.uint8)      # the block_size prefix
    keep = np.ones(blob.size, dtype=bool)
    cig = off + 32 + l_name
    for k in range(4):
        keep[cig + k] = False
    new_off = (off - 4 * np.arange(len(off), dtype=np.int64)).astype(np.uint64)
    return GroupedReads(np.ascontiguousarray(blob[keep]), new_off, new_len, np.array(g.grp_first, copy=True))


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


def split_families(c):
    lib.fgx_debug_last_split_builds.restype = None
    lib.fgx_debug_last_split_builds.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    b = (C.c_uint64 * 4)()
    lib.fgx_debug_last_split_builds(c._h, b)
    return int(b[0]) + int(b[1])


def host_entry(a):
    """(child interpreter under the parent's library) the host entry on the prefix of the twin, read from --prefix-file."""
    z = np.load(a.prefix_file)
    g = GroupedReads(z["blob"], z["rec_off"], z["rec_len"], z["grp_first"])
    c = caller()
    c.process_batch(g.subset(0, min(g.n_grp, 100)))            # warm-up
    runs, out = [], None
    for _ in range(a.host_runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = c.process_batch(g)
        torch.cuda.synchronize()
        runs.append(round(int(g.n_rec) / (time.perf_counter() - t0)))
    dg = g.to_device()
    dev = c.process_batch_device(dg)
    print(json.dumps({"library": os.path.basename(os.environ.get("FGX_LIB") or "libfgumi_amd.so"), "families": int(g.n_grp), "raw_reads": int(g.n_rec),
                      "raw_reads_per_s_runs": runs, "consensus_records": int(out.count), "device_entry_deferred_families": int(dev.n_deferred)}))
    c.close()


def bench_ab(path):
    rows = [json.loads(ln) for ln in open(path).read().splitlines() if ln.strip().startswith("{")]
    out = {"lines": rows, "summary": {}}
    for args in sorted({r.get("args", "") for r in rows}):
        v = {lb: [float(r["value"]) for r in rows if r.get("args", "") == args and r.get("library") == lb] for lb in ("parent", "head")}
        if v["parent"] and v["head"]:
            pm, hm, spread = sum(v["parent"]) / len(v["parent"]), sum(v["head"]) / len(v["head"]), max(v["parent"]) - min(v["parent"])
            out["summary"][args or "(default)"] = {"parent_mean": pm, "head_mean": hm, "parent_spread_max_minus_min": spread, "head_mean_minus_parent_mean": hm - pm,
                                                    "head_not_below_parent_by_more_than_the_spread": bool(hm >= pm - spread)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=50000)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bench-ab", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unmapped_device_bench.json"))
    ap.add_argument("--prefix-file", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.prefix_file:
        return host_entry(a)
    c = caller()
    dg = c.simulate_on_device(a.families, **SIM)
    g = GroupedReads(dg.blob[:dg.blob_len].cpu().numpy(), dg.rec_off.cpu().numpy().astype(np.uint64), dg.rec_len.cpu().numpy().astype(np.uint32),
                     dg.grp_first.cpu().numpy().astype(np.uint32))
    t0 = time.perf_counter()
    u = unmap_all(g)
    t_convert = time.perf_counter() - t0
    du = u.to_device()
    n_reads = int(g.n_rec)
    doc = {"what": "simplex consensus on unmapped reads in the device-resident pipeline: a mapped batch, its wholly unmapped twin, the parent's host entry on a prefix of the twin",
           "library": os.path.basename(os.environ.get("FGX_LIB") or "libfgumi_amd.so"),
           "workload": f"{a.families} families x 8 pairs x 150 bp, device-resident", "raw_reads": n_reads, "steps": a.steps, "repeats": a.repeats,
           "host_conversion_s": round(t_convert, 2), "mapped": [], "unmapped": []}
    for _ in range(a.repeats):
        for name, d in (("mapped", dg), ("unmapped", du)):
            dt, out = timed(c, d, a.steps, a.warmup)
            doc[name].append({"ms_per_step": round(dt * 1e3, 3), "raw_reads_per_s": round(n_reads / dt), "consensus_records": int(out.count), "output_bytes": int(out.data_len),
                              "deferred_families": int(out.n_deferred), "families_finished_by_the_split_pipeline": split_families(c),
                              "kernel_ms": round(float(c.last_timing["kernels"]), 3)})
    m = [r["raw_reads_per_s"] for r in doc["mapped"]]
    w = [r["raw_reads_per_s"] for r in doc["unmapped"]]
    doc["summary"] = {"mapped_mean_raw_reads_per_s": round(sum(m) / len(m)), "unmapped_mean_raw_reads_per_s": round(sum(w) / len(w)),
                      "mapped_spread_max_minus_min": max(m) - min(m), "unmapped_over_mapped": round(sum(w) / sum(m), 4),
                      "twin_slower_than_mapped_by_more_than_the_spread": bool(sum(w) / len(w) < sum(m) / len(m) - (max(m) - min(m)))}
    c.close()
    if a.parent_lib:
        n = min(a.host_sample, u.n_grp)
        r1 = int(u.grp_first[n])
        end = int(u.rec_off[r1 - 1]) + int(u.rec_len[r1 - 1])
        pf = a.out + ".prefix.npz"
        np.savez(pf, blob=u.blob[:end], rec_off=u.rec_off[:r1], rec_len=u.rec_len[:r1], grp_first=u.grp_first[:n + 1])
        try:
            env = dict(os.environ, FGX_LIB=os.path.abspath(a.parent_lib))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--prefix-file", pf, "--host-runs", str(a.host_runs)], env=env, capture_output=True, text=True)
            assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
            doc["parent_host_entry"] = json.loads(p.stdout.strip().splitlines()[-1])
            best = max(doc["parent_host_entry"]["raw_reads_per_s_runs"])
            doc["summary"]["unmapped_over_parent_host_entry"] = round(doc["summary"]["unmapped_mean_raw_reads_per_s"] / best, 1)
        finally:
            os.remove(pf)
    else:
        doc["parent_host_entry"] = None
        doc["note_parent_host_entry"] = "not measured: no --parent-lib given"
    if a.bench_ab:
        doc["feature_unused_bench_ab"] = bench_ab(a.bench_ab)
    else:
        doc["feature_unused_bench_ab"] = None
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["summary"]))


if __name__ == "__main__":
    main()
