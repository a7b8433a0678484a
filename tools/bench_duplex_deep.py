#!/usr/bin/env python3
"""Duplex molecules of more than 64 records on the streaming duplex kernels (fgumi_amd/csrc/duplex_deep.inc; FGX_DUPLEX_DEEP, on by default) — measured against
the switch at 0 and against the parent commit's library, which decides such molecules on the general path of the host entry only.  Writes
profiles/duplex_deep_bench.json.

The batch: --molecules (200 000) duplex molecules of 2 .. 100 pairs x 150 bp (`family_size=2, family_size_max=100`), resident in HBM; --steps (40) steps per leg,
--repeats (3) repeats.
  (a) device_entry: this library's device entry on the whole batch — ms per step, raw reads/s, molecules deferred, fgx_debug_last_duplex_deep — and the share
      of molecules and of reads above 64 records in the batch.
  (b) switch_0: the same batch, the same library, FGX_DUPLEX_DEEP=0: how many molecules the device entry defers (its rate is the rate of the DECIDED molecules
      only: no rate of the batch).
  (c) parent_host_entry: the PARENT library's host entry (fgx_process_batch) on the first --parent-molecules (50 000) molecules: the rate those molecules get
      without the new kernels.
  (d) nothing_deep: `python bench.py --caller duplex` on the parent's library and on this one, alternating, three runs each: values, means, the parent's
      spread; this build's mean must not be below the parent's by more than that spread.

Every library runs in a child interpreter of its own (FGX_LIB selects it at import).  A leg that did not run — no --parent-lib, no GPU — is listed under
"missing".  --static FILE adds the kernels' static figures (a JSON object, see profiles/README.md) to the file.

--max-reads-per-strand N: every caller of every leg gets the cap, the device legs of THIS library run under FGX_DUPLEX_DEEP_CAP=1 (the CAP builds of the two
kernels; off by default), their lines carry fgx_debug_last_duplex_deep_capped, and the result goes to profiles/duplex_deep_cap_bench.json.  Leg (a) then
first checks a sample (--check-molecules, 300) of the batch's kind byte for byte against the oracle (tests/orc.py), with nothing deferred.  The parent has
one way only for a capped deep molecule — its device entry defers it, its host entry decides it: leg (c) is that way, leg (e) the parent's device entry alone
on the whole batch (how many molecules it defers).

  python tools/bench_duplex_deep.py --parent-lib <parent commit's libfgumi_amd.so> [--legs a,b,c,d,e] [--max-reads-per-strand N] [--out profiles/duplex_deep_bench.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIM = dict(family_size=2, family_size_max=100, duplex=1)


# ---- workers: one library each (the parent process set FGX_LIB / FGX_DUPLEX_DEEP) ----------------------------------------------------------------
def _caller(a):
    from fgumi_amd import DuplexConsensusCaller
    return DuplexConsensusCaller("", "A", [1, 1, 0], cell_tag="CB", overlapping_consensus=True, max_reads_per_strand=a.max_reads_per_strand)


def _last_duplex_deep(c, name="fgx_debug_last_duplex_deep"):
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
    o = fgx_opts.defaults(kind=1, duplex_min_reads=(1, 1, 0), duplex_max_reads_per_strand=a.max_reads_per_strand)
    want = orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=100)
    out = c.process_batch_device(g.to_device())
    ok = out.n_deferred == 0 and out.count == want["count"] and out.to_host() == want["data"]
    return {"molecules": int(g.n_grp), "deferred_molecules": int(out.n_deferred), "consensus_records": int(out.count), "equal_to_the_oracle": bool(ok)}


def worker_device(a):
    """This library's device entry on the whole batch, the switch as the environment has it."""
    import numpy as np
    import torch
    c = _caller(a)
    check = _check_sample(a, c) if a.max_reads_per_strand is not None and a.check_molecules > 0 else None
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
                      "duplex_deep_molecules": _last_duplex_deep(c), "duplex_deep_capped_molecules": _last_duplex_deep(c, "fgx_debug_last_duplex_deep_capped"),
                      "max_reads_per_strand": a.max_reads_per_strand, "check_sample": check, "kernel_ms": round(float(c.last_timing["kernels"]), 3),
                      "molecules_above_64_records": int((n > 64).sum()), "share_of_molecules_above_64_records": round(float((n > 64).mean()), 4),
                      "share_of_reads_above_64_records": round(float(n[n > 64].sum() / n.sum()), 4)}))
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


def _child(cmd, lib=None, switch=None, timeout=1200, cap_switch=False):
    e = dict(os.environ)
    e.pop("FGX_LIB", None)
    e.pop("FGX_DUPLEX_DEEP", None)
    e.pop("FGX_DUPLEX_DEEP_CAP", None)
    if cap_switch:
        e["FGX_DUPLEX_DEEP_CAP"] = "1"
    if lib:
        e["FGX_LIB"] = lib
    if switch is not None:
        e["FGX_DUPLEX_DEEP"] = switch
    p = subprocess.run(cmd, env=e, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} exited with {p.returncode}:\n{p.stderr[-3000:]}")
    return p.stdout


def _me(a, worker):
    return [sys.executable, os.path.abspath(__file__), "--worker", worker, "--molecules", str(a.molecules), "--parent-molecules", str(a.parent_molecules),
            "--steps", str(a.steps), "--warmup", str(a.warmup), "--check-molecules", str(a.check_molecules)] + \
           (["--max-reads-per-strand", str(a.max_reads_per_strand)] if a.max_reads_per_strand is not None else [])


def leg_device(a, switch, lib=None):
    capped = a.max_reads_per_strand is not None
    cmd = _me(a, "device") + (["--check-molecules", "0"] if lib else [])           # (the oracle check is of this library's legs)
    runs = [_last_json(_child(cmd, lib=lib, switch=switch, cap_switch=capped and lib is None)) for _ in range(a.repeats)]
    rates = [r["raw_reads_per_s"] for r in runs]
    what = f"; --max-reads-per-strand {a.max_reads_per_strand}, FGX_DUPLEX_DEEP_CAP {'1' if lib is None else 'unset'}" if capped else ""
    return {"workload": f"{a.molecules} duplex molecules x 2 .. 100 pairs x 150 bp, device-resident; FGX_DUPLEX_DEEP {'unset' if switch is None else switch}{what}",
            "repeats": runs, "raw_reads_per_s": rates, "mean_raw_reads_per_s": round(sum(rates) / len(rates)),
            "deferred_molecules": [r["deferred_molecules"] for r in runs], "duplex_deep_molecules": [r["duplex_deep_molecules"] for r in runs],
            "duplex_deep_capped_molecules": [r["duplex_deep_capped_molecules"] for r in runs]}


def leg_a(a):
    return leg_device(a, None)


def leg_b(a):
    out = leg_device(a, "0")
    out["note"] = "the rate is that of the molecules the device entry decided; the deferred ones are still to be decided by the general path"
    return out


def leg_c(a):
    runs = [_last_json(_child(_me(a, "host_entry"), lib=a.parent_lib)) for _ in range(a.repeats)]
    rates = [r["raw_reads_per_s"] for r in runs]
    return {"workload": f"the parent library's host entry on the first {a.parent_molecules} molecules of the batch", "repeats": runs, "raw_reads_per_s": rates,
            "mean_raw_reads_per_s": round(sum(rates) / len(rates))}


def leg_e(a):
    out = leg_device(a, None, lib=a.parent_lib)
    out["note"] = "the parent library's device entry: the rate is that of the molecules it decided; the deferred ones are still to be decided by its host entry (leg c)"
    return out


def leg_d(a):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--caller", "duplex", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup), "--no-cpu-baseline"]
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
    ap.add_argument("--molecules", type=int, default=200000)
    ap.add_argument("--parent-molecules", type=int, default=50000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=2)
    ap.add_argument("--static", default=None, help="JSON file with the kernels' static figures, copied into the result")
    ap.add_argument("--max-reads-per-strand", type=int, default=None, help="the callers' cap; this library's device legs then run under FGX_DUPLEX_DEEP_CAP=1")
    ap.add_argument("--check-molecules", type=int, default=300, help="under a cap: molecules of the sample leg (a) checks against the oracle first (0: none)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", choices=["device", "host_entry"], default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "duplex_deep_bench.json" if a.max_reads_per_strand is None else "duplex_deep_cap_bench.json")
    if a.worker:
        return {"device": worker_device, "host_entry": worker_host_entry}[a.worker](a)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.setdefault("missing", [])
    if a.static:
        res["static"] = json.load(open(a.static))

    def save():                                             # (after every leg: a later one that is cut short loses nothing)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    stopped = False
    for leg, key, fn, needs_parent in (("a", "device_entry", leg_a, False), ("b", "switch_0", leg_b, False), ("c", "parent_host_entry", leg_c, True), ("d", "nothing_deep", leg_d, True),
                                      ("e", "parent_device_entry", leg_e, True)):
        if leg not in a.legs.split(","):
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
