#!/usr/bin/env python3
"""What the host driver of the device-resident pipeline (fastpath.hip) DID for a fixed list of seeded batches, one per route of the launch chain:
kernel launches, host synchronisations and every `fgx_debug_last_*` diagnostic, plus the deferred count and the 28 counters — for the first batch
of a caller (it carries the table-image uploads and their synchronisations) and for a second batch through the same caller.  One JSON document.

  python tools/chain_counts.py [--out FILE] [--scale 1.0] [--cases a,b]

A host-side change of the driver must leave the document EQUAL: run it with the library before and after (`FGX_LIB=<library>`; each case is a child
interpreter with its own environment switches) and compare the files.  With the CPU emulator (`FGX_LIB=tests/hostemu/_build/libwavemu.so`, see
tests/wavemu.py) the batches are host arrays; with the product library they are copied to the GPU first.  TEST TOOLING: it uses tests/methsim.py."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

# name: (caller kind, families, simulate_grouped_reads arguments | "meth", option overrides, environment)
CASES = {
    "depth3_seg4": (0, 600, dict(family_size=3), {}, {}),
    "depth8_packed": (0, 600, dict(family_size=8), {}, {}),
    "long_tail_2_50": (0, 500, dict(family_size=2, family_size_max=50), {}, {}),
    "deep_35_120": (0, 40, dict(family_size=35, family_size_max=120), {}, {}),
    "depth8_classic_build": (0, 600, dict(family_size=8), {}, {"FGX_S2_PACKED": "0"}),
    "depth8_no_split": (0, 600, dict(family_size=8), {}, {"FGX_SPLIT": "0"}),
    "depth8_4_chunks": (0, 600, dict(family_size=8), {}, {"FGX_SPLIT_CHUNKS": "4"}),
    "depth8_direct": (0, 600, dict(family_size=8), {}, {"FGX_DIRECT": "1"}),
    "long_tail_direct_merge": (0, 300, dict(family_size=2, family_size_max=50), {}, {"FGX_DIRECT": "1"}),
    "noisy_depth8_pool_rerun": (0, 600, dict(family_size=8, error_rate_ppm=20000), {}, {"FGX_POOL_DIV": "4096", "FGX_POOL_SLACK": "1"}),
    "duplex": (1, 300, dict(family_size=12, duplex=1), {}, {}),
    "duplex_em_seq": (1, 300, "meth", dict(methylation_mode=1), {}),
    "codec": (2, 300, dict(family_size=4, read_length=300, insert_mean=350, insert_sd=60, codec=1), dict(overlapping_consensus=0), {}),
    "codec_per_field_writer": (2, 100, dict(family_size=3, read_length=150, insert_mean=200, insert_sd=30, codec=1), dict(overlapping_consensus=0, read_name_prefix=b"n" * 70), {}),
    "simplex_em_seq": (0, 300, "meth", dict(methylation_mode=1), {}),
}


def one_case(name, scale):
    import numpy as np

    import fgx_opts
    from fgumi_amd import GroupedReads, simulate_grouped_reads
    from fgumi_amd._lib import SO, Options, Output, lib
    kind, n, sim, opts, _ = CASES[name]
    n = max(8, int(n * scale))
    contigs = None
    if sim == "meth":
        import bamutil
        import methsim
        rng = methsim.seeded(71 if kind == 1 else 40)
        contigs = methsim.genome(rng)
        groups = methsim.duplex_groups(rng, contigs, n) if kind == 1 else methsim.simplex_groups(rng, contigs, n)
        g = GroupedReads.from_groups([x for x in groups if all(bamutil.parse(r)["n_cigar"] == 1 for r in x)])
    else:
        g = simulate_grouped_reads(n, **sim)
    o = fgx_opts.defaults(kind=kind, **opts)
    po = Options.from_buffer_copy(bytes(o))
    h = lib.fgx_create(C.byref(po))
    assert h, lib.fgx_global_error().decode()
    for f, t in (("last_split_chunks", C.c_uint32), ("last_routed", C.c_uint32), ("last_big_families", C.c_uint32), ("last_deep_families", C.c_uint32),
                 ("last_meth_device", C.c_uint32), ("last_direct", C.c_int)):
        getattr(lib, "fgx_debug_" + f).restype = t
        getattr(lib, "fgx_debug_" + f).argtypes = [C.c_void_p]
    lib.fgx_debug_last_chain.restype = None
    lib.fgx_debug_last_chain.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    lib.fgx_debug_last_split_builds.restype = None
    lib.fgx_debug_last_split_builds.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    if contigs is not None:
        bufs = [C.create_string_buffer(bytes(s), max(1, len(s))) for s in contigs]
        ptrs = (C.c_void_p * len(bufs))(*[C.cast(b, C.c_void_p).value for b in bufs])
        lens = (C.c_uint64 * len(bufs))(*[len(s) for s in contigs])
        assert lib.fgx_set_reference(h, len(bufs), ptrs, lens) == 0, lib.fgx_last_error(h).decode()
    arrays = [np.concatenate([g.blob, np.zeros(64, dtype=np.uint8)]), g.rec_off, g.rec_len, g.grp_first]
    if "emu" in os.path.basename(SO):     # the CPU emulation libraries take host arrays for the tensors in HBM
        ptr = [a.ctypes.data for a in arrays]
    else:
        import torch
        dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
        ptr = [t.data_ptr() for t in dev]
    batches = []
    try:
        for _ in range(2):
            out, nd, dp = Output(), C.c_uint32(), C.c_void_p()
            rc = lib.fgx_process_batch_device(h, ptr[0], g.blob.size, ptr[1], ptr[2], g.n_rec, ptr[3], g.n_grp, C.byref(out), C.byref(nd), C.byref(dp))
            assert rc == 0, lib.fgx_last_error(h).decode()
            chain, builds = (C.c_uint32 * 2)(), (C.c_uint64 * 4)()
            lib.fgx_debug_last_chain(h, chain)
            lib.fgx_debug_last_split_builds(h, builds)
            d = {"last_chain": {"launches": int(chain[0]), "host_syncs": int(chain[1])},
                 "last_split_builds": {"packed_families": int(builds[0]), "classic_families": int(builds[1]), "build": int(builds[2]), "first_stage_retries": int(builds[3])}}
            for f in ("last_split_chunks", "last_routed", "last_big_families", "last_deep_families", "last_meth_device", "last_direct"):
                d[f] = int(getattr(lib, "fgx_debug_" + f)(h))
            d.update(n_deferred=int(nd.value), count=int(out.count), out_len=int(out.data_len), stats=[int(v) for v in out.stats])
            batches.append(d)
    finally:
        lib.fgx_destroy(h)
    print(json.dumps({"families": int(g.n_grp), "records": int(g.n_rec), "first_batch": batches[0], "second_batch": batches[1]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--scale", type=float, default=1.0, help="families of every case x this")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--one", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one_case(a.one, a.scale)
    doc = {}
    for name in a.cases.split(","):
        e = dict(os.environ, FGX_ALLOW_LIBM_MISMATCH="1")
        e.update(CASES[name][4])
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--scale", str(a.scale)], env=e, capture_output=True, text=True, timeout=1500)
        if p.returncode != 0:
            sys.exit(f"{name}: child exited with {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        doc[name] = {"env": CASES[name][4], **json.loads(p.stdout.strip().splitlines()[-1])}
        print(name, json.dumps(doc[name]["first_batch"]["last_chain"]), file=sys.stderr, flush=True)
    text = json.dumps(doc, indent=1, sort_keys=True) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
