#!/usr/bin/env python3
"""Deep duplex molecules with indel reads through the workgroup-per-molecule canonicaliser and the deep duplex kernels in the canonical second pass
(FGX_DEEP_INDELS=1, off by default) — measured against the switch unset, which is the parent commit's only route.  Writes profiles/deep_indels_bench.json.

The simulator draws no indels, so the tool rewrites, on the host, one read of about half (--indel-share, 0.5) of the molecules above 64 records of a simulated batch
(the `tools/bench_duplex_deep.py` shape: --molecules (200 000) molecules of 2 .. 100 pairs): the one-op CIGAR `<l>M` becomes `<a>M2D<l-a>M` (a in 30 .. l - 30; a
deletion leaves SEQ and QUAL as they are) and the MC of the record's mate is rewritten to match.  The share of deep molecules that then hold an indel read is recorded.
  (a) on:        the switch on: ms per step, raw reads/s, deferred molecules, fgx_debug_last_duplex_deep (first pass), fgx_debug_last_deep_indels (second pass);
                 first a sample (--check-groups, 200) of the batch's kind compared byte for byte with the oracle (tests/orc.py), both entries.
  (b) unset:     the switch unset on a prefix (--prefix-molecules, 50 000) — the device entry (its rate is that of the molecules it decided) and the host entry
                 (fgx_process_batch) on the first --host-groups (300) of the molecules it deferred: the route those molecules have in the parent.
  (c) no_indels: the batch without an indel read, the switch on against unset, alternating, three runs each: the switch costs such a batch nothing.
Every run is a child interpreter of its own.  A leg that did not run is listed under "missing".  --static FILE adds the kernels' static figures.

  python tools/bench_deep_indels.py [--legs a,b,c] [--static FILE] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIM = dict(family_size=2, family_size_max=100, duplex=1)


def with_indels(g, share, seed=20241021):
    """`g` (GroupedReads of the simulator: records back to back, each behind its 4-byte size, mates adjacent, one `<l>M` op each) with one read of `share` of the
    molecules above 64 records given a 2-base deletion, and that read's mate's MC rewritten.  Returns (GroupedReads, has_indel[n_grp])."""
    from fgumi_amd import GroupedReads
    off, ln = g.rec_off.astype(np.int64), g.rec_len.astype(np.int64)
    assert off[0] == 4 and np.array_equal(off[1:], off[:-1] + ln[:-1] + 4), "records back to back"
    first = np.asarray(g.grp_first, dtype=np.int64)
    n = np.diff(first)
    assert (n % 2 == 0).all(), "mates adjacent: an even number of records per group"
    rng = np.random.default_rng(seed)
    has_indel = (n > 64) & (rng.random(g.n_grp) < share)
    picks = {}                                                    # record -> bases ahead of the deletion
    for gi in np.flatnonzero(has_indel).tolist():
        picks[int(first[gi] + rng.integers(0, n[gi]))] = int(rng.integers(30, 60))
    touched = sorted(set(picks) | {r ^ 1 for r in picks})
    blob = memoryview(g.blob)
    pieces, new_len, at = [], ln.copy(), 0
    for r in touched:
        o, k = int(off[r]), int(ln[r])
        rec = bytes(blob[o:o + k])
        l_name, n_cig, l_seq = rec[8], rec[12] | (rec[13] << 8), int.from_bytes(rec[16:20], "little")
        assert n_cig == 1 and l_seq > 90
        c0 = 32 + l_name
        head, ops, tail = bytearray(rec[:c0]), rec[c0:c0 + 4], rec[c0 + 4:]
        if r in picks:
            a = picks[r]
            ops = b"".join(int(v).to_bytes(4, "little") for v in ((a << 4), (2 << 4) | 2, ((l_seq - a) << 4)))
            head[12], head[13] = 3, 0
        m = r ^ 1
        if m in picks:
            i = tail.find(b"MCZ", (l_seq + 1) // 2 + l_seq)
            assert i >= 0, "the simulator's paired records carry MC"
            e = tail.index(b"\0", i + 3)
            ml = int.from_bytes(bytes(blob[int(off[m]) + 16:int(off[m]) + 20]), "little")
            tail = tail[:i + 3] + f"{picks[m]}M2D{ml - picks[m]}M".encode() + tail[e:]
        body = bytes(head) + ops + tail
        pieces += [blob[at:o - 4], len(body).to_bytes(4, "little"), body]
        at = o + k
        new_len[r] = len(body)
    pieces.append(blob[at:])
    new_blob = np.frombuffer(b"".join(pieces), dtype=np.uint8)
    new_off = np.cumsum(new_len + 4) - new_len
    return GroupedReads(new_blob, new_off.astype(np.uint64), new_len.astype(np.uint32), g.grp_first.copy()), has_indel


def _batch(n, share):
    from fgumi_amd import simulate_grouped_reads
    g = simulate_grouped_reads(n, **SIM)
    if share <= 0:
        return g, np.zeros(g.n_grp, dtype=bool)
    return with_indels(g, share)


def _caller():
    from fgumi_amd import DuplexConsensusCaller
    return DuplexConsensusCaller("", "A", [1, 1, 0], cell_tag="CB", overlapping_consensus=True)


def _counter(c, name):
    from fgumi_amd import lib
    if not hasattr(lib, name):
        return None
    getattr(lib, name).restype = C.c_uint32
    getattr(lib, name).argtypes = [C.c_void_p]
    return int(getattr(lib, name)(c._h))


def _check_sample(a):
    """Both entries on a sample of the batch's kind against the oracle (bytes, count, the 28 counters)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import deep_indel_cases as D
    import fgx_opts
    g, has_indel = _batch(a.check_groups, a.indel_share)
    o = fgx_opts.defaults(kind=1)
    want = D.want_of(o, g)
    c = D.Caller(o)
    try:
        got = c.device(g)
        ok_dev = got["deferred"] == 0 and got["data"] == want["data"] and got["count"] == want["count"] and np.array_equal(got["stats"], want["stats"])
        host = c.host(g)
        ok_host = host["data"] == want["data"] and host["count"] == want["count"] and np.array_equal(host["stats"], want["stats"])
    finally:
        c.close()
    return {"groups": int(g.n_grp), "molecules_with_an_indel_read": int(has_indel.sum()), "deferred": got["deferred"], "deep_indels": got["deep_indels"],
            "device_entry_equal_to_the_oracle": bool(ok_dev), "host_entry_equal_to_the_oracle": bool(ok_host)}


def worker_device(a):
    """The device entry on the whole batch, the switch as the environment has it; with --host-groups the host entry on the first deferred deep molecules as well."""
    import torch
    check = _check_sample(a) if a.check_groups > 0 else None
    t0 = time.perf_counter()
    g, has_indel = _batch(a.groups, a.indel_share)
    t_build = time.perf_counter() - t0
    n = np.diff(np.asarray(g.grp_first, dtype=np.int64))
    c = _caller()
    dg = g.to_device()
    out = None
    for _ in range(a.warmup):
        out = c.process_batch_device(dg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = c.process_batch_device(dg)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    deep = n > 64
    res = {"switch": os.environ.get("FGX_DEEP_INDELS"), "groups": int(g.n_grp), "raw_reads": int(g.n_rec), "indel_share": a.indel_share, "steps": a.steps, "warmup": a.warmup,
           "ms_per_step": round(dt * 1e3, 3), "raw_reads_per_s": round(int(g.n_rec) / dt), "consensus_records": int(out.count), "deferred_groups": int(out.n_deferred),
           "duplex_deep": _counter(c, "fgx_debug_last_duplex_deep"), "deep_indels": _counter(c, "fgx_debug_last_deep_indels"),
           "kernel_ms": round(float(c.last_timing["kernels"]), 3), "host_seconds_to_build_the_batch": round(t_build, 1),
           "molecules_above_64_records": int(deep.sum()), "share_of_reads_above_64_records": round(float(n[deep].sum() / n.sum()), 4),
           "deep_molecules_with_an_indel_read": int(has_indel.sum()), "share_of_deep_molecules_with_an_indel_read": round(float(has_indel[deep].mean()), 4) if deep.any() else None,
           "share_of_reads_in_molecules_with_an_indel_read": round(float(n[has_indel].sum() / n.sum()), 4), "check_sample": check}
    if a.host_groups > 0:
        from fgumi_amd import GroupedReads
        ids = np.flatnonzero(has_indel)[:a.host_groups]           # what the device entry defers with the switch unset
        if len(ids):
            gs = GroupedReads.from_groups([g.records(int(i)) for i in ids])
            c.process_batch(gs.subset(0, 1))                      # warm-up: allocations, table images
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ho = c.process_batch(gs)
            torch.cuda.synchronize()
            dh = time.perf_counter() - t0
            res["host_entry_on_deferred_groups"] = {"groups": int(gs.n_grp), "raw_reads": int(gs.n_rec), "ms": round(dh * 1e3, 2), "raw_reads_per_s": round(int(gs.n_rec) / dh),
                                                    "consensus_records": int(ho.count)}
    print(json.dumps(res))
    c.close()


def _last_json(text):
    for ln in reversed(text.strip().splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    raise ValueError("no JSON line in the child's output:\n" + text[-2000:])


def _run(a, groups, share, switch, check=0, host_groups=0, timeout=1500):
    e = dict(os.environ)
    e.pop("FGX_DEEP_INDELS", None)
    if switch:
        e["FGX_DEEP_INDELS"] = "1"
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--groups", str(groups), "--indel-share", str(share), "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--check-groups", str(check), "--host-groups", str(host_groups)]
    p = subprocess.run(cmd, env=e, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} exited with {p.returncode}:\n{p.stderr[-3000:]}")
    r = _last_json(p.stdout)
    print(f"{groups} molecules, indel share {share}, switch {'on' if switch else 'unset'}: {r['raw_reads_per_s']} raw reads/s, deferred {r['deferred_groups']}", file=sys.stderr, flush=True)
    return r


def leg_a(a):
    r = _run(a, a.molecules, a.indel_share, True, check=a.check_groups)
    r["sample_equal_to_the_oracle"] = bool(r["check_sample"] and r["check_sample"]["device_entry_equal_to_the_oracle"] and r["check_sample"]["host_entry_equal_to_the_oracle"])
    return r


def leg_b(a):
    r = _run(a, a.prefix_molecules, a.indel_share, False, host_groups=a.host_groups)
    r["note"] = "the device entry's rate is that of the molecules it decided; the deferred ones are still to be decided by the host entry, at the rate of host_entry_on_deferred_groups"
    return r


def leg_c(a):
    vals = {"on": [], "unset": []}
    for _ in range(3):
        for who in ("unset", "on"):
            vals[who].append(_run(a, a.molecules, 0.0, who == "on")["raw_reads_per_s"])
    mo, mu = sum(vals["on"]) / 3, sum(vals["unset"]) / 3
    return {"on_raw_reads_per_s": vals["on"], "unset_raw_reads_per_s": vals["unset"], "on_mean": round(mo), "unset_mean": round(mu), "unset_spread": max(vals["unset"]) - min(vals["unset"]),
            "price_of_the_switch_percent": round(100.0 * (mu - mo) / mu, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--molecules", type=int, default=200000)
    ap.add_argument("--prefix-molecules", type=int, default=50000)
    ap.add_argument("--indel-share", type=float, default=0.5, help="share of the molecules above 64 records that get an indel read")
    ap.add_argument("--host-groups", type=int, default=300, help="deferred molecules the host entry decides in leg (b)")
    ap.add_argument("--check-groups", type=int, default=200, help="molecules of the sample leg (a) checks against the oracle first (0: none)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--static", default=None, help="JSON file with the kernels' static figures, copied into the result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_indels_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--groups", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker_device(a)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.setdefault("missing", [])
    if a.static:
        res["static"] = json.load(open(a.static))

    def save():                                             # (after every leg: a later one that is cut short loses nothing)
        if "on" in res and "unset" in res and "host_entry_on_deferred_groups" in res["unset"]:
            res["on_over_host_entry_on_deferred_groups"] = round(res["on"]["raw_reads_per_s"] / res["unset"]["host_entry_on_deferred_groups"]["raw_reads_per_s"], 1)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    stopped = False
    for leg, key, fn in (("a", "on", leg_a), ("b", "unset", leg_b), ("c", "no_indels", leg_c)):
        if leg not in a.legs.split(","):
            if key not in res and not any(m.startswith(key + ":") for m in res["missing"]):
                res["missing"].append(f"{key}: not measured yet (leg {leg} was not asked for)")
            continue
        if stopped:                                         # an earlier leg's child failed or hung: nothing more is started on the device in this call
            if key not in res:
                res["missing"] = [m for m in res["missing"] if not m.startswith(key + ":")] + [f"{key}: not measured yet (not started: an earlier leg failed)"]
            continue
        try:
            res[key] = fn(a)
            res["missing"] = [m for m in res["missing"] if not m.startswith(key + ":")]
            save()
        except Exception as ex:
            print(f"{key}: {ex}", file=sys.stderr)
            res["missing"] = [m for m in res["missing"] if not m.startswith(key + ":")] + [f"{key}: not measured yet (its child process failed: no MI355X run has filled it in)"]
            stopped = True
    save()
    print(json.dumps({"written": os.path.relpath(a.out, ROOT), "missing": res["missing"]}))


if __name__ == "__main__":
    main()
