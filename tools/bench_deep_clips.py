#!/usr/bin/env python3
"""Deep simplex families and deep duplex molecules with soft-clipped reads on the clip-taking builds of the streaming record kernels (FGX_DEEP_CLIPS=1, off by
default) — measured against the switch unset, which is the parent commit's only route.  Writes profiles/deep_clips_bench.json.

The simulator draws no clips, so the tool rewrites a seeded share (--clip-share, 2 %) of the records of a simulated long-tail batch on the host: the one-op
CIGAR `<l>M` becomes `<k>S<l-k>M` or `<l-k>M<k>S` (k in 1 .. 20) and the MC of the record's mate is rewritten to match.  The rewritten batch goes to HBM once.
  (a) duplex_on:    --molecules (200 000) duplex molecules of 2 .. 100 pairs, the switch on: ms per step, raw reads/s, deferred molecules,
                    fgx_debug_last_duplex_deep, fgx_debug_last_deep_clipped, the share of molecules and of reads in molecules that hold a clipped read; first a
                    sample (--check-groups, 200) of the batch's kind compared byte for byte with the oracle (tests/orc.py), both entries.
  (b) duplex_unset: the same batch, the switch unset — the device entry (its rate is that of the molecules it decided) and the host entry (fgx_process_batch)
                    on the first --host-groups (300) of the molecules it deferred: the route those molecules have without the clip builds.
  (c) simplex_on / simplex_unset: --families (400 000) simplex families of 2 .. 50 pairs (the `bench.py --depth 2 --depth-max 50` shape), clipped alike.
  (d) no_clips:     batches (a) and (c) without a clipped read, the switch on against unset, alternating, three runs each: the price of the larger record kernel.
Every run is a child interpreter of its own.  A leg that did not run is listed under "missing".  --static FILE adds the kernels' static figures.

  python tools/bench_deep_clips.py [--legs a,b,c,d] [--static FILE] [--out FILE]"""
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
SIMS = {"duplex": dict(family_size=2, family_size_max=100, duplex=1), "simplex": dict(family_size=2, family_size_max=50)}


# ---- clips on the host ----------------------------------------------------------------------------------------------------------------------------------
def with_clips(g, share, seed=20240917):
    """`g` (GroupedReads of the simulator: records back to back, each behind its 4-byte size, mates adjacent, one `<l>M` op each) with `share` of its records
    soft-clipped at one end and the mates' MC rewritten.  Returns (GroupedReads, clipped[n_rec])."""
    from fgumi_amd import GroupedReads
    off, ln = g.rec_off.astype(np.int64), g.rec_len.astype(np.int64)
    assert off[0] == 4 and np.array_equal(off[1:], off[:-1] + ln[:-1] + 4), "records back to back"
    first = np.asarray(g.grp_first, dtype=np.int64)
    assert (np.diff(first) % 2 == 0).all(), "mates adjacent: an even number of records per group"
    rng = np.random.default_rng(seed)
    clipped = rng.random(g.n_rec) < share
    ks, lead = rng.integers(1, 21, g.n_rec), rng.random(g.n_rec) < 0.5
    touched = np.flatnonzero(clipped | clipped[np.arange(g.n_rec) ^ 1])      # (group starts are even: record r's mate is r ^ 1)
    blob = memoryview(g.blob)
    pieces, new_len, at = [], ln.copy(), 0

    def cigar_text(r, l_seq):
        k = int(ks[r])
        return (f"{k}S{l_seq - k}M" if lead[r] else f"{l_seq - k}M{k}S"), ([(k << 4) | 4, ((l_seq - k) << 4)] if lead[r] else [((l_seq - k) << 4), (k << 4) | 4])

    for r in touched.tolist():
        o, n = int(off[r]), int(ln[r])
        rec = bytes(blob[o:o + n])
        l_name, n_cig, l_seq = rec[8], rec[12] | (rec[13] << 8), int.from_bytes(rec[16:20], "little")
        assert n_cig == 1 and l_seq > 40
        c0 = 32 + l_name
        head, ops, tail = bytearray(rec[:c0]), rec[c0:c0 + 4], rec[c0 + 4:]
        if clipped[r]:
            _, new_ops = cigar_text(r, l_seq)
            ops = b"".join(int(v).to_bytes(4, "little") for v in new_ops)
            head[12], head[13] = 2, 0
        m = r ^ 1
        if clipped[m]:
            a0 = (l_seq + 1) // 2 + l_seq
            i = tail.find(b"MCZ", a0)
            assert i >= 0, "the simulator's paired records carry MC"
            e = tail.index(b"\0", i + 3)
            ml = int.from_bytes(bytes(blob[int(off[m]) + 16:int(off[m]) + 20]), "little")
            tail = tail[:i + 3] + cigar_text(m, ml)[0].encode() + tail[e:]
        body = bytes(head) + ops + tail
        pieces.append(blob[at:o - 4])
        pieces.append(len(body).to_bytes(4, "little"))
        pieces.append(body)
        at = o + n
        new_len[r] = len(body)
    pieces.append(blob[at:])
    new_blob = np.frombuffer(b"".join(pieces), dtype=np.uint8)
    new_off = np.cumsum(new_len + 4) - new_len
    return GroupedReads(new_blob, new_off.astype(np.uint64), new_len.astype(np.uint32), g.grp_first.copy()), clipped


def _batch(a, kind, n, share):
    from fgumi_amd import simulate_grouped_reads
    g = simulate_grouped_reads(n, **SIMS[kind])
    if share <= 0:
        return g, np.zeros(g.n_rec, dtype=bool)
    return with_clips(g, share)


def _caller(kind):
    from fgumi_amd import DuplexConsensusCaller, VanillaUmiConsensusCaller
    if kind == "duplex":
        return DuplexConsensusCaller("", "A", [1, 1, 0], cell_tag="CB", overlapping_consensus=True)
    from fgumi_amd.caller import VanillaUmiConsensusOptions
    return VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(min_reads=1, min_consensus_base_quality=2, cell_tag="CB"), overlapping_consensus=True)


def _counter(c, name):
    from fgumi_amd import lib
    if not hasattr(lib, name):
        return None
    getattr(lib, name).restype = C.c_uint32
    getattr(lib, name).argtypes = [C.c_void_p]
    return int(getattr(lib, name)(c._h))


def _check_sample(a, kind):
    """Both entries on a sample of the batch's kind against the oracle (bytes, count, the 28 counters), through the tests' runner."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import deep_clip_cases as K
    g, clipped = _batch(a, kind, a.check_groups, a.clip_share)
    n = np.diff(np.asarray(g.grp_first, dtype=np.int64))
    case = K.Case(g, kind=1 if kind == "duplex" else 0)
    want = K.want_of(case)
    c = K.Caller(case.kind)
    try:
        got = c.device(g)
        ok_dev = got["deferred"] == 0 and got["data"] == want["data"] and got["count"] == want["count"] and np.array_equal(got["stats"], want["stats"])
        host = c.host(g)
        ok_host = host["data"] == want["data"] and host["count"] == want["count"] and np.array_equal(host["stats"], want["stats"])
    finally:
        c.close()
    return {"groups": int(g.n_grp), "groups_above_64_records": int((n > 64).sum()), "clipped_reads": int(clipped.sum()), "deferred": got["deferred"], "deep_clipped": got["clipped"],
            "device_entry_equal_to_the_oracle": bool(ok_dev), "host_entry_equal_to_the_oracle": bool(ok_host)}


def worker_device(a):
    """The device entry on the whole batch, the switch as the environment has it; with --host-groups the host entry on the first deferred deep groups as well."""
    import torch
    kind = a.kind
    check = _check_sample(a, kind) if a.check_groups > 0 else None
    t0 = time.perf_counter()
    g, clipped = _batch(a, kind, a.groups, a.clip_share)
    t_build = time.perf_counter() - t0
    first = np.asarray(g.grp_first, dtype=np.int64)
    n = np.diff(first)
    has_clip = np.add.reduceat(clipped.astype(np.int64), first[:-1]) > 0
    c = _caller(kind)
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
    res = {"kind": kind, "switch": os.environ.get("FGX_DEEP_CLIPS"), "groups": int(g.n_grp), "raw_reads": int(g.n_rec), "clip_share": a.clip_share, "steps": a.steps, "warmup": a.warmup,
           "ms_per_step": round(dt * 1e3, 3), "raw_reads_per_s": round(int(g.n_rec) / dt), "consensus_records": int(out.count), "deferred_groups": int(out.n_deferred),
           "duplex_deep": _counter(c, "fgx_debug_last_duplex_deep"), "deep_families": _counter(c, "fgx_debug_last_deep_families"), "deep_clipped": _counter(c, "fgx_debug_last_deep_clipped"),
           "kernel_ms": round(float(c.last_timing["kernels"]), 3), "host_seconds_to_build_the_batch": round(t_build, 1),
           "clipped_reads": int(clipped.sum()), "groups_above_64_records": int((n > 64).sum()), "share_of_reads_above_64_records": round(float(n[n > 64].sum() / n.sum()), 4),
           "groups_with_a_clipped_read": int(has_clip.sum()), "share_of_groups_with_a_clipped_read": round(float(has_clip.mean()), 4),
           "share_of_reads_in_groups_with_a_clipped_read": round(float(n[has_clip].sum() / n.sum()), 4),
           "deep_groups_with_a_clipped_read": int((has_clip & (n > 64)).sum()), "share_of_deep_groups_with_a_clipped_read": round(float(has_clip[n > 64].mean()), 4) if (n > 64).any() else None,
           "share_of_reads_in_deep_groups_with_a_clipped_read": round(float(n[has_clip & (n > 64)].sum() / n.sum()), 4), "check_sample": check}
    if a.host_groups > 0:
        from fgumi_amd import GroupedReads
        ids = np.flatnonzero(has_clip & (n > (64 if kind == "duplex" else 128)))[:a.host_groups]      # what the device entry defers with the switch unset
        gs = GroupedReads.from_groups([g.records(int(i)) for i in ids]) if len(ids) else None
        if gs is None:                                          # (families of at most 128 records with a clipped read are k_family's: nothing is deferred)
            res["host_entry_on_deferred_groups"] = None
            print(json.dumps(res))
            c.close()
            return
        c.process_batch(gs.subset(0, 1))                        # warm-up: allocations, table images
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ho = c.process_batch(gs)
        torch.cuda.synchronize()
        dh = time.perf_counter() - t0
        res["host_entry_on_deferred_groups"] = {"groups": int(gs.n_grp), "raw_reads": int(gs.n_rec), "ms": round(dh * 1e3, 2), "raw_reads_per_s": round(int(gs.n_rec) / dh),
                                                "consensus_records": int(ho.count)}
    print(json.dumps(res))
    c.close()


# ---- the driver -----------------------------------------------------------------------------------------------------------------------------------------
def _last_json(text):
    for ln in reversed(text.strip().splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    raise ValueError("no JSON line in the child's output:\n" + text[-2000:])


def _run(a, kind, groups, share, switch, check=0, host_groups=0, timeout=1500):
    e = dict(os.environ)
    e.pop("FGX_DEEP_CLIPS", None)
    if switch:
        e["FGX_DEEP_CLIPS"] = "1"
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--kind", kind, "--groups", str(groups), "--clip-share", str(share), "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--check-groups", str(check), "--host-groups", str(host_groups)]
    p = subprocess.run(cmd, env=e, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} exited with {p.returncode}:\n{p.stderr[-3000:]}")
    r = _last_json(p.stdout)
    print(f"{kind}, {groups} groups, clip share {share}, switch {'on' if switch else 'unset'}: {r['raw_reads_per_s']} raw reads/s, deferred {r['deferred_groups']}", file=sys.stderr, flush=True)
    return r


def leg_a(a):
    r = _run(a, "duplex", a.molecules, a.clip_share, True, check=a.check_groups)
    r["sample_equal_to_the_oracle"] = bool(r["check_sample"] and r["check_sample"]["device_entry_equal_to_the_oracle"] and r["check_sample"]["host_entry_equal_to_the_oracle"])
    return r


def leg_b(a):
    r = _run(a, "duplex", a.molecules, a.clip_share, False, host_groups=a.host_groups)
    r["note"] = "the device entry's rate is that of the molecules it decided; the deferred ones are still to be decided by the host entry, at the rate of host_entry_on_deferred_groups"
    return r


def leg_c(a):
    on = _run(a, "simplex", a.families, a.clip_share, True, check=a.check_groups)
    off = _run(a, "simplex", a.families, a.clip_share, False, host_groups=a.host_groups)
    return {"on": on, "unset": off, "on_over_unset_device_entry": round(on["raw_reads_per_s"] / off["raw_reads_per_s"], 3),
            "note": "unset, a family of 65 .. 128 records with a clipped read is k_family's and one above 128 is deferred; families of 2 .. 50 pairs hold at most 100 records, so nothing is deferred here"}


def leg_d(a):
    out = {}
    for kind, n in (("duplex", a.molecules), ("simplex", a.families)):
        vals = {"on": [], "unset": []}
        for _ in range(3):
            for who in ("unset", "on"):
                vals[who].append(_run(a, kind, n, 0.0, who == "on")["raw_reads_per_s"])
        mo, mu = sum(vals["on"]) / 3, sum(vals["unset"]) / 3
        out[kind] = {"on_raw_reads_per_s": vals["on"], "unset_raw_reads_per_s": vals["unset"], "on_mean": round(mo), "unset_mean": round(mu), "unset_spread": max(vals["unset"]) - min(vals["unset"]),
                     "price_of_the_clip_builds_percent": round(100.0 * (mu - mo) / mu, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--molecules", type=int, default=200000)
    ap.add_argument("--families", type=int, default=400000)
    ap.add_argument("--clip-share", type=float, default=0.02)
    ap.add_argument("--host-groups", type=int, default=300, help="deferred groups the host entry decides in legs (b) and (c)")
    ap.add_argument("--check-groups", type=int, default=200, help="groups of the sample legs (a) and (c) check against the oracle first (0: none)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--static", default=None, help="JSON file with the kernels' static figures, copied into the result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_clips_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--kind", choices=["duplex", "simplex"], default="duplex", help=argparse.SUPPRESS)
    ap.add_argument("--groups", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker_device(a)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.setdefault("missing", [])
    if a.static:
        res["static"] = json.load(open(a.static))

    def save():                                             # (after every leg: a later one that is cut short loses nothing)
        if "duplex_on" in res and "duplex_unset" in res and "host_entry_on_deferred_groups" in res["duplex_unset"]:
            res["duplex_on_over_host_entry_on_deferred_groups"] = round(res["duplex_on"]["raw_reads_per_s"] / res["duplex_unset"]["host_entry_on_deferred_groups"]["raw_reads_per_s"], 1)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    stopped = False
    for leg, key, fn in (("a", "duplex_on", leg_a), ("b", "duplex_unset", leg_b), ("c", "simplex", leg_c), ("d", "no_clips", leg_d)):
        if leg not in a.legs.split(","):
            if key not in res and not any(m.startswith(key) for m in res["missing"]):
                res["missing"].append(f"{key}: not measured yet (leg {leg} was not asked for)")
            continue
        if stopped:                                         # an earlier leg's child failed or hung: nothing more is started on the device in this call
            if key not in res:
                res["missing"] = [m for m in res["missing"] if not m.startswith(key)] + [f"{key}: not measured yet (not started: an earlier leg failed)"]
            continue
        try:
            res[key] = fn(a)
            res["missing"] = [m for m in res["missing"] if not m.startswith(key)]
            save()
        except Exception as ex:
            print(f"{key}: {ex}", file=sys.stderr)
            res["missing"] = [m for m in res["missing"] if not m.startswith(key)] + [f"{key}: not measured yet (its child process failed: no MI355X run has filled it in)"]
            stopped = True
    save()
    print(json.dumps({"written": os.path.relpath(a.out, ROOT), "missing": res["missing"]}))


if __name__ == "__main__":
    main()
