#!/usr/bin/env python3
"""FGX_DEEP_WIDE=1 — simplex families of more than 512 records / more than 255 reads per end on the wide kernels (fgumi_amd/csrc/simplex_wide.inc) — measured
against the parent commit's library, which decides such families on the general path of the host entry only.  Writes profiles/deep_wide_bench.json.

  (a) resident: --families (2 000) families of 300 .. 1 000 pairs x 150 bp resident in HBM, without a cap and at --max-reads 100: this library's device entry with
      the switch on (ms per step, raw reads/s, families on the wide kernels, families deferred) against the PARENT library's host entry on the first
      --parent-families (20) families of the same batch (the only way the parent decides them); three alternating repeats, both rates and their ratio.
  (b) bound: one family of WIDE_MAX = 16 384 records through the device entry: ms per step, and — under `rocprofv3 --kernel-trace`, when it is installed — the
      mean time of k_wide_parse, k_wide_cols and k_wide_finish (what the O(n^2) phases of k_wide_parse cost at the bound).
  (c) unset: `python bench.py` and `python bench.py --depth 2 --depth-max 50` on the parent's library and on this one, alternating, three runs each, the switch
      unset: values, means, the parent's spread; and tools/chain_counts.py on both (kernel launches, host synchronisations, diagnostics and counters of
      three seeded batches must be equal).

Every library runs in a child interpreter of its own (FGX_LIB selects it at import).  A leg that did not run — no --parent-lib, no GPU — is listed under
"missing".  --static FILE adds the kernels' static figures (a JSON object, see profiles/README.md) to the file.

  python tools/bench_deep_wide.py --parent-lib <parent commit's libfgumi_amd.so> [--legs a,b,c] [--out profiles/deep_wide_bench.json]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIM = dict(family_size=300, family_size_max=1000)
WIDE_MAX = 16384
KERNELS = ("k_wide_parse", "k_wide_cols", "k_wide_finish")


# ---- workers: one library each (the parent process set FGX_LIB / FGX_DEEP_WIDE) ------------------------------------------------------------------
def _caller(cap):
    from fgumi_amd import VanillaUmiConsensusCaller, VanillaUmiConsensusOptions
    return VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(min_reads=1, max_reads=cap, min_consensus_base_quality=2, cell_tag="CB"), overlapping_consensus=True)


def _device_steps(c, dg, steps, warmup):
    import torch
    out = None
    for _ in range(warmup):
        out = c.process_batch_device(dg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = c.process_batch_device(dg)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, out


def worker_resident(a):
    """This library's device entry, the switch as the environment has it."""
    import torch  # noqa: F401
    res = {}
    for name, cap in (("no_cap", None), ("max_reads_100", 100)):
        c = _caller(cap)
        dg = c.simulate_on_device(a.families, **SIM)
        dt, out = _device_steps(c, dg, a.steps, a.warmup)
        res[name] = {"families": int(dg.n_grp), "raw_reads": int(dg.n_rec), "ms_per_step": round(dt * 1e3, 3), "raw_reads_per_s": round(int(dg.n_rec) / dt),
                     "consensus_records": int(out.count), "deferred_families": int(out.n_deferred), "families_on_the_wide_kernels": c.last_wide_families,
                     "kernel_ms": round(float(c.last_timing["kernels"]), 3)}
        c.close()
        del dg
        torch.cuda.empty_cache()
    print(json.dumps(res))


def worker_host_entry(a):
    """The host entry (fgx_process_batch) on the first families of the same batch: how a library without the wide kernels decides them."""
    import torch
    from fgumi_amd import simulate_grouped_reads
    gs = simulate_grouped_reads(a.parent_families, **SIM)
    res = {}
    for name, cap in (("no_cap", None), ("max_reads_100", 100)):
        c = _caller(cap)
        c.process_batch(gs.subset(0, 1))                      # warm-up: allocations, table images
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = c.process_batch(gs)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[name] = {"families": int(gs.n_grp), "raw_reads": int(gs.n_rec), "ms": round(dt * 1e3, 2), "raw_reads_per_s": round(int(gs.n_rec) / dt), "consensus_records": int(out.count)}
        c.close()
    print(json.dumps(res))


def worker_bound(a):
    import torch  # noqa: F401
    c = _caller(None)
    dg = c.simulate_on_device(1, family_size=WIDE_MAX // 2)
    assert int(dg.n_rec) == WIDE_MAX
    dt, out = _device_steps(c, dg, a.steps, a.warmup)
    print(json.dumps({"records": int(dg.n_rec), "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt * 1e3, 3), "kernel_ms": round(float(c.last_timing["kernels"]), 3),
                      "consensus_records": int(out.count), "deferred_families": int(out.n_deferred), "families_on_the_wide_kernels": c.last_wide_families}))
    c.close()


# ---- the driver -----------------------------------------------------------------------------------------------------------------------------------
def _last_json(text):
    for ln in reversed(text.strip().splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    raise ValueError("no JSON line in the child's output:\n" + text[-2000:])


def _child(cmd, lib=None, wide=None, timeout=1200):
    e = dict(os.environ)
    e.pop("FGX_LIB", None)
    e.pop("FGX_DEEP_WIDE", None)
    if lib:
        e["FGX_LIB"] = lib
    if wide is not None:
        e["FGX_DEEP_WIDE"] = wide
    p = subprocess.run(cmd, env=e, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} exited with {p.returncode}:\n{p.stderr[-3000:]}")
    return p.stdout


def leg_a(a):
    me = [sys.executable, os.path.abspath(__file__)]
    common = ["--families", str(a.families), "--parent-families", str(a.parent_families), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    runs = []
    for _ in range(a.repeats):
        head = _last_json(_child(me + ["--worker", "resident"] + common, wide="1"))
        parent = _last_json(_child(me + ["--worker", "host_entry"] + common, lib=a.parent_lib))
        runs.append({"this_device_entry": head, "parent_host_entry": parent})
    out = {"workload": f"{a.families} families x 300 .. 1000 pairs x 150 bp, device-resident; parent: host entry on the first {a.parent_families}", "repeats": runs}
    for name in ("no_cap", "max_reads_100"):
        h = [r["this_device_entry"][name]["raw_reads_per_s"] for r in runs]
        p = [r["parent_host_entry"][name]["raw_reads_per_s"] for r in runs]
        out[name] = {"this_raw_reads_per_s": h, "parent_raw_reads_per_s": p, "ratio_of_means": round((sum(h) / len(h)) / (sum(p) / len(p)), 1),
                     "deferred_families": [r["this_device_entry"][name]["deferred_families"] for r in runs]}
    return out


def leg_b(a):
    me = [sys.executable, os.path.abspath(__file__), "--worker", "bound", "--steps", str(a.steps), "--warmup", str(a.warmup)]
    out = _last_json(_child(me, wide="1"))
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if not prof:
        out["per_kernel_ms"] = "missing: rocprofv3 is not installed"
        return out
    d = tempfile.mkdtemp(prefix="deep_wide_trace_")
    try:
        _child([prof, "--kernel-trace", "--output-format", "csv", "-d", d, "--"] + me, wide="1")
        per = {}
        for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            for r in csv.DictReader(open(f)):
                for k in KERNELS:
                    if k in r["Kernel_Name"]:
                        per.setdefault(k, []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
        out["per_kernel_ms"] = {k: round(sum(t for _, t in sorted(v)[-a.steps:]) / min(a.steps, len(v)), 4) for k, v in per.items()} or "missing: no wide kernel in the trace"
    except Exception as ex:
        print(f"bound under rocprofv3: {ex}", file=sys.stderr)
        out["per_kernel_ms"] = "missing: the run under rocprofv3 failed"
        out["stop"] = True                                  # (a child failed or hung: main() starts nothing after this leg)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return out


def leg_c(a):
    out = {}
    # the launch chain of three seeded batches (tools/chain_counts.py: launches, host synchronisations, every diagnostic, the 28 counters), both libraries
    docs = {}
    cases = "depth8_packed,long_tail_2_50,deep_35_120"
    for who, lib in (("parent", a.parent_lib), ("this", None)):
        f = tempfile.NamedTemporaryFile(suffix=".json", delete=False).name
        try:
            _child([sys.executable, os.path.join(ROOT, "tools", "chain_counts.py"), "--cases", cases, "--out", f], lib=lib, timeout=600)
            docs[who] = json.load(open(f))
        finally:
            os.remove(f)
    out["launch_chain"] = {"cases": cases, "documents_equal": docs["parent"] == docs["this"],
                           "per_case": {k: {who: docs[who][k]["second_batch"]["last_chain"] for who in docs} for k in docs["this"]}}
    for name, extra in (("default", []), ("long_tail", ["--depth", "2", "--depth-max", "50"])):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup), "--no-cpu-baseline"] + extra
        vals = {"parent": [], "this": []}
        for _ in range(3):
            for who, lib in (("parent", a.parent_lib), ("this", None)):
                line = _last_json(_child(cmd, lib=lib, timeout=1800))
                vals[who].append(line["value"])
        mp, mt = sum(vals["parent"]) / 3, sum(vals["this"]) / 3
        spread = max(vals["parent"]) - min(vals["parent"])
        out[name] = {"command": " ".join(cmd[1:]), "parent_values": vals["parent"], "this_values": vals["this"], "parent_mean": mp, "this_mean": mt, "parent_spread": spread,
                     "this_not_below_parent_by_more_than_its_spread": mt >= mp - spread}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libfgumi_amd.so")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--families", type=int, default=2000)
    ap.add_argument("--parent-families", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=2)
    ap.add_argument("--static", default=None, help="JSON file with the kernels' static figures, copied into the result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_wide_bench.json"))
    ap.add_argument("--worker", choices=["resident", "host_entry", "bound"], default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return {"resident": worker_resident, "host_entry": worker_host_entry, "bound": worker_bound}[a.worker](a)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.setdefault("missing", [])
    names = {"a": "resident", "b": "bound", "c": "switch_unset"}
    if a.static:
        res["static"] = json.load(open(a.static))

    def save():                                             # (after every leg: a later one that is cut short loses nothing)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    stopped = False
    for leg, fn, needs_parent in (("a", leg_a, True), ("b", leg_b, False), ("c", leg_c, True)):
        key = names[leg]
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
            save()
            stopped = res[key].pop("stop", False)
            res["missing"] = [m for m in res["missing"] if not m.startswith(key)]
        except Exception as ex:
            print(f"{key}: {ex}", file=sys.stderr)
            why = "no --parent-lib" if needs_parent and not a.parent_lib else "its child process failed: no MI355X run has filled it in"
            res["missing"] = [m for m in res["missing"] if not m.startswith(key)] + [f"{key}: not measured yet ({why})"]
            stopped = bool(a.parent_lib) or not needs_parent
    save()
    print(json.dumps({"written": os.path.relpath(a.out, ROOT), "missing": res["missing"]}))


if __name__ == "__main__":
    main()
