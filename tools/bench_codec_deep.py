#!/usr/bin/env python3
"""CODEC molecules of more than 64 records on the streaming CODEC kernels (fgumi_amd/csrc/codec_deep.inc; FGX_CODEC_DEEP=1, off by default) — measured against
the switch unset and against the parent commit's library, which decides such molecules on the general path of the host entry only.  Writes
profiles/codec_deep_bench.json.

The batch: --molecules (100 000) CODEC molecules of 2 .. 100 pairs x 150 bp (`family_size=2, family_size_max=100, codec=1`), resident in HBM; --steps (40) steps
per leg, --repeats (3) repeats.
  (a) device_entry: this library's device entry on the whole batch under FGX_CODEC_DEEP=1 — ms per step, raw reads/s, molecules deferred,
      fgx_debug_last_codec_deep / _capped — and the share of molecules and of reads above 64 records in the batch.  First a sample (--check-molecules, 300) of
      the batch's kind is compared byte for byte with the oracle (tests/orc.py), with nothing deferred.
  (b) switch_unset: the same batch, the same library, FGX_CODEC_DEEP unset: how many molecules the device entry defers (its rate is the rate of the DECIDED
      molecules only: no rate of the batch).
  (c) parent_host_entry: the PARENT library's host entry (fgx_process_batch) on the first --parent-molecules (20 000) molecules: the only route those molecules
      have without the new kernels.  The ratio (a) / (c) is written beside it.
  (d) nothing_deep: `python bench.py --caller codec` on the parent's library and on this one, alternating, three runs each: values, means, the parent's
      spread; this build's mean must not be below the parent's by more than that spread.
--max-reads-per-strand N gives every caller of every leg the cap (the CAP builds of the record kernel).

Every library runs in a child interpreter of its own (FGX_LIB selects it at import).  A leg that did not run — no --parent-lib, no GPU — is listed under
"missing".  --static FILE adds the kernels' static figures (a JSON object, see profiles/README.md) to the file; they are recorded even when no GPU leg ran.

  python tools/bench_codec_deep.py --parent-lib <parent commit's libfgumi_amd.so> [--legs a,b,c,d] [--max-reads-per-strand N] [--static FILE] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIM = dict(family_size=2, family_size_max=100, codec=1)


# ---- workers: one library each (the parent process set FGX_LIB / FGX_CODEC_DEEP) ------------------------------------------------------------------
def _caller(a):
    from fgumi_amd import CodecConsensusCaller, CodecConsensusOptions
    return CodecConsensusCaller("", "A", CodecConsensusOptions(produce_per_base_tags=True, max_reads_per_strand=a.max_reads_per_strand))


def _counter(c, name):
    from fgumi_amd import lib
    if not hasattr(lib, name):
        return None
    getattr(lib, name).restype = C.c_uint32
    getattr(lib, name).argtypes = [C.c_void_p]
    return int(getattr(lib, name)(c._h))


def _check_sample(a, c):
    """The device entry on a sample of the batch's kind against the oracle: nothing deferred, the bytes and the count equal."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fgx_opts
    import orc
    from fgumi_amd import simulate_grouped_reads
    g = simulate_grouped_reads(a.check_molecules, **SIM)
    o = fgx_opts.defaults(kind=2, overlapping_consensus=0, cell_tag=b"\0\0", produce_per_base_tags=1,
                          codec_max_reads_per_strand=-1 if a.max_reads_per_strand is None else a.max_reads_per_strand)
    want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=1000)
    out = c.process_batch_device(g.to_device())
    ok = out.n_deferred == 0 and out.count == want["count"] and out.to_host() == want["data"]
    return {"molecules": int(g.n_grp), "deferred_molecules": int(out.n_deferred), "consensus_records": int(out.count), "equal_to_the_oracle": bool(ok)}


def worker_device(a):
    """This library's device entry on the whole batch, the switch as the environment has it."""
    import numpy as np
    import torch
    c = _caller(a)
    check = _check_sample(a, c) if os.environ.get("FGX_CODEC_DEEP") == "1" and a.check_molecules > 0 else None
    dg = c.simulate_on_device(a.molecules, **SIM)
    n = np.diff(dg.grp_first.cpu().numpy().astype(np.int64))
    out = None
    for _ in range(a.warmup):
        out = c.process_batch_device(dg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = c.process_batch_device(dg)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    print(json.dumps({"molecules": int(dg.n_grp), "raw_reads": int(dg.n_rec), "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt * 1e3, 3),
                      "raw_reads_per_s": round(int(dg.n_rec) / dt), "consensus_records": int(out.count), "deferred_molecules": int(out.n_deferred),
                      "codec_deep_molecules": _counter(c, "fgx_debug_last_codec_deep"), "codec_deep_capped_molecules": _counter(c, "fgx_debug_last_codec_deep_capped"),
                      "max_reads_per_strand": a.max_reads_per_strand, "check_sample": check, "kernel_ms": round(float(c.last_timing["kernels"]), 3),
                      "molecules_above_64_records": int((n > 64).sum()), "molecules_above_254_records": int((n > 254).sum()),
                      "share_of_molecules_above_64_records": round(float((n > 64).mean()), 4), "share_of_reads_above_64_records": round(float(n[n > 64].sum() / n.sum()), 4)}))
    c.close()


def worker_host_entry(a):
    """The host entry (fgx_process_batch) on the first molecules of the same batch: how a library without the new kernels decides its deep molecules."""
    import torch
    from fgumi_amd import simulate_grouped_reads
    gs = simulate_grouped_reads(a.parent_molecules, **SIM)
    c = _caller(a)
    c.process_batch(gs.subset(0, 1))                          # warm-up: allocations, table images
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = c.process_batch(gs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"molecules": int(gs.n_grp), "raw_reads": int(gs.n_rec), "ms": round(dt * 1e3, 2), "raw_reads_per_s": round(int(gs.n_rec) / dt), "consensus_records": int(out.count)}))
    c.close()


# ---- the driver -----------------------------------------------------------------------------------------------------------------------------------
def _last_json(text):
    for ln in reversed(text.strip().splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    raise ValueError("no JSON line in the child's output:\n" + text[-2000:])


def _child(cmd, lib=None, switch=None, timeout=1200):
    e = dict(os.environ)
    e.pop("FGX_LIB", None)
    e.pop("FGX_CODEC_DEEP", None)
    if lib:
        e["FGX_LIB"] = lib
    if switch is not None:
        e["FGX_CODEC_DEEP"] = switch
    p = subprocess.run(cmd, env=e, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} exited with {p.returncode}:\n{p.stderr[-3000:]}")
    return p.stdout


def _me(a, worker):
    return [sys.executable, os.path.abspath(__file__), "--worker", worker, "--molecules", str(a.molecules), "--parent-molecules", str(a.parent_molecules),
            "--steps", str(a.steps), "--warmup", str(a.warmup), "--check-molecules", str(a.check_molecules)] + \
           (["--max-reads-per-strand", str(a.max_reads_per_strand)] if a.max_reads_per_strand is not None else [])


def leg_device(a, switch):
    runs = [_last_json(_child(_me(a, "device"), switch=switch)) for _ in range(a.repeats)]
    rates = [r["raw_reads_per_s"] for r in runs]
    what = f"; --max-reads-per-strand {a.max_reads_per_strand}" if a.max_reads_per_strand is not None else ""
    return {"workload": f"{a.molecules} CODEC molecules x 2 .. 100 pairs x 150 bp, device-resident; FGX_CODEC_DEEP {'unset' if switch is None else switch}{what}",
            "repeats": runs, "raw_reads_per_s": rates, "mean_raw_reads_per_s": round(sum(rates) / len(rates)),
            "deferred_molecules": [r["deferred_molecules"] for r in runs], "codec_deep_molecules": [r["codec_deep_molecules"] for r in runs],
            "codec_deep_capped_molecules": [r["codec_deep_capped_molecules"] for r in runs]}


def leg_a(a):
    out = leg_device(a, "1")
    out["defers_nothing"] = all(d == 0 for d in out["deferred_molecules"])
    out["sample_equal_to_the_oracle"] = all(r["check_sample"] and r["check_sample"]["equal_to_the_oracle"] for r in out["repeats"]) if a.check_molecules > 0 else None
    return out


def leg_b(a):
    out = leg_device(a, None)
    out["note"] = "the rate is that of the molecules the device entry decided; the deferred ones are still to be decided by the general path"
    return out


def leg_c(a):
    runs = [_last_json(_child(_me(a, "host_entry"), lib=a.parent_lib)) for _ in range(a.repeats)]
    rates = [r["raw_reads_per_s"] for r in runs]
    return {"workload": f"the parent library's host entry on the first {a.parent_molecules} molecules of the batch", "repeats": runs, "raw_reads_per_s": rates,
            "mean_raw_reads_per_s": round(sum(rates) / len(rates))}


def leg_d(a):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--caller", "codec", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup), "--no-cpu-baseline"]
    vals = {"parent": [], "this": []}
    for _ in range(3):
        for who, lib in (("parent", a.parent_lib), ("this", None)):
            vals[who].append(_last_json(_child(cmd, lib=lib, timeout=1800))["value"])
    mp, mt = sum(vals["parent"]) / 3, sum(vals["this"]) / 3
    spread = max(vals["parent"]) - min(vals["parent"])
    return {"command": "bench.py " + " ".join(cmd[2:]), "parent_values": vals["parent"], "this_values": vals["this"], "parent_mean": mp, "this_mean": mt, "parent_spread": spread,
            "this_not_below_parent_by_more_than_its_spread": mt >= mp - spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libfgumi_amd.so")
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--molecules", type=int, default=100000)
    ap.add_argument("--parent-molecules", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=2)
    ap.add_argument("--static", default=None, help="JSON file with the kernels' static figures, copied into the result")
    ap.add_argument("--max-reads-per-strand", type=int, default=None, help="the cap of every leg's caller")
    ap.add_argument("--check-molecules", type=int, default=300, help="molecules of the sample leg (a) checks against the oracle first (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_deep_bench.json"))
    ap.add_argument("--worker", choices=["device", "host_entry"], default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return {"device": worker_device, "host_entry": worker_host_entry}[a.worker](a)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.setdefault("missing", [])
    if a.static:
        res["static"] = json.load(open(a.static))

    def save():                                             # (after every leg: a later one that is cut short loses nothing)
        if "device_entry" in res and "parent_host_entry" in res:
            res["device_entry_over_parent_host_entry"] = round(res["device_entry"]["mean_raw_reads_per_s"] / res["parent_host_entry"]["mean_raw_reads_per_s"], 1)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    stopped = False
    for leg, key, fn, needs_parent in (("a", "device_entry", leg_a, False), ("b", "switch_unset", leg_b, False), ("c", "parent_host_entry", leg_c, True), ("d", "nothing_deep", leg_d, True)):
        if leg not in a.legs.split(","):
            if key not in res and not any(m.startswith(key) for m in res["missing"]):
                res["missing"].append(f"{key}: not measured yet (leg {leg} was not asked for)")
            continue
        if stopped:                                         # an earlier leg's child failed or hung: nothing more is started on the device in this call
            if key not in res:
                res["missing"] = [m for m in res["missing"] if not m.startswith(key)] + [f"{key}: not measured yet (not started: an earlier leg failed)"]
            continue
        try:
            if needs_parent and not a.parent_lib:
                raise RuntimeError("no --parent-lib")
            res[key] = fn(a)
            res["missing"] = [m for m in res["missing"] if not m.startswith(key)]
            save()
        except Exception as ex:
            print(f"{key}: {ex}", file=sys.stderr)
            why = "no --parent-lib" if needs_parent and not a.parent_lib else "its child process failed: no MI355X run has filled it in"
            res["missing"] = [m for m in res["missing"] if not m.startswith(key)] + [f"{key}: not measured yet ({why})"]
            stopped = bool(a.parent_lib) or not needs_parent
    save()
    print(json.dumps({"written": os.path.relpath(a.out, ROOT), "missing": res["missing"]}))


if __name__ == "__main__":
    main()
