"""Batches in the record layouts of tests/layouts.py, with hostile groups of the general-path fuzz spliced in, through BOTH entries of the
product library against the oracle (TEST INFRASTRUCTURE).  Shared by the wave-level emulator tests (host arrays, tests/wavemu) and the GPU
tests (tensors in HBM).

Per batch: `fgx_process_batch` must equal the oracle over the whole batch; `fgx_process_batch_device` must equal the oracle over the groups
it did not defer, the deferred groups resubmitted through the host entry must equal the oracle over them, and the two entries' counters
must add up to the whole batch's.  Where the oracle raises, the product must refuse the batch.  Returns what ran (head, deferred groups,
hostile groups decided on the device) so that the tests can assert the route."""
import ctypes as C
import json
import os
import random

import numpy as np

import fgx_opts
import layouts
import orc
import test_general_path_fuzz as fuzz
from fgumi_amd import GroupedReads, simulate_grouped_reads

KINDS = {"simplex": 0, "duplex": 1, "codec": 2}
BATCH = {0: 50, 1: 100, 2: 1000}

# the heads of the launch chain and the simulated backgrounds that pick them (kind, simulate_grouped_reads arguments, options, environment)
HEADS = {
    "seg4": ("simplex", dict(family_size=3), dict(min_reads=1), {}),
    "packed": ("simplex", dict(family_size=8), dict(min_reads=1), {}),
    "pair": ("simplex", dict(family_size=2, family_size_max=50), dict(min_reads=1), {}),
    "deep": ("simplex", dict(family_size=35, family_size_max=60), dict(min_reads=1), {}),
    "trim": ("simplex", dict(family_size=4), dict(min_reads=1, trim=1), {}),
    "wave2": ("simplex", dict(family_size=4), dict(min_reads=1), {"FGX_SPLIT": "0"}),
    "meth": ("simplex", None, dict(min_reads=1, methylation_mode=1), {}),
    "duplex": ("duplex", dict(family_size=6, duplex=1), dict(min_reads=1), {}),
    "codec": ("codec", dict(family_size=3, read_length=150, insert_mean=200, insert_sd=30, codec=1), dict(overlapping_consensus=0), {}),
}


def _debug(lib):
    for f in ("fgx_debug_last_big_families", "fgx_debug_last_deep_families", "fgx_debug_last_routed", "fgx_debug_last_split_chunks", "fgx_debug_last_meth_device"):
        getattr(lib, f).restype = C.c_uint32
        getattr(lib, f).argtypes = [C.c_void_p]
    lib.fgx_debug_last_split_builds.restype = None
    lib.fgx_debug_last_split_builds.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.fgx_debug_last_deferral.restype = None
    lib.fgx_debug_last_deferral.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]


def background(head, n, seed=42):
    """The head's simulated batch (and, for the methylation-aware mode, its reference contigs)."""
    kind, sim, okw, _ = HEADS[head]
    if sim is None:
        import methsim
        rng = methsim.seeded(seed)
        contigs = methsim.genome(rng)
        return GroupedReads.from_groups(methsim.simplex_groups(rng, contigs, n, depth=(2, 8), read_len=(40, 120))), contigs
    return simulate_grouped_reads(n, seed=seed, **sim), None


def chunk_starts(n_grp, n_rec, n_chunks):
    """First group of each chunk after the first, as Batch::set_up cuts the batch for the split pipeline (fastpath.hip): families per wavefront
    of the record kernel from the mean family size, chunks rounded up to whole workgroups (4 wavefronts) of it."""
    mean_recs = n_rec / n_grp
    fpw = min(16, max(1, int(64.0 / mean_recs))) if mean_recs >= 1.0 else 16
    raw = (n_grp + n_chunks - 1) // n_chunks
    chunk_fam = (raw + 4 * fpw - 1) // (4 * fpw) * (4 * fpw)
    return [k * chunk_fam for k in range(1, n_chunks) if k * chunk_fam < n_grp]


def splice(g, kind, hostile_seed, n_hostile, n_chunks=None):
    """Hostile groups of the general-path fuzz (random_group, `exotic`) spliced into batch g.  Positions in the SPLICED batch: the first and the
    last group, three inside the first 64 (the build-choice sample), with `n_chunks` the groups on both sides of every chunk boundary, the rest
    at random.  Returns (batch, indices of the hostile groups)."""
    rng = random.Random(hostile_seed)
    hostile = [x for x in (fuzz.random_group(rng, 100000 + i, kind, True) for i in range(n_hostile * 2)) if x][:n_hostile]
    groups = [g.records(i) for i in range(g.n_grp)]
    total = len(groups) + len(hostile)
    want = [0, total - 1] + [rng.randrange(1, min(64, total - 1)) for _ in range(3)]
    if n_chunks:
        for b in chunk_starts(total, g.n_rec + sum(len(x) for x in hostile), n_chunks):
            want += [b - 1, b]
    where = []
    for p in want + [rng.randrange(total) for _ in range(len(hostile))]:
        if p not in where and len(where) < len(hostile):
            where.append(p)
    assert len(where) == len(hostile) and set(want) <= set(where), (want, where)
    where = set(where)
    out, hi, bi = [], iter(hostile), iter(groups)
    for i in range(total):
        out.append(next(hi) if i in where else next(bi))
    return GroupedReads.from_groups(out), sorted(where)


def hostile_deep(g, seed, every=2):
    """Hostile records inside the background's families of more than 64 records (the streaming kernels' families): in every `every`-th such
    family one of record 0 made secondary, record 0 made unmapped, a record dropped (its mate is left alone), one read's qualities all 2, a
    foreign MC (clipped CIGAR of another shape).  Returns (batch, indices of the changed families)."""
    rng = random.Random(seed)
    groups, changed = [], []
    for gi in range(g.n_grp):
        recs = [layouts.Rec(r) for r in g.records(gi)]
        if len(recs) > 64 and gi % every == 0:
            what = rng.choice(["secondary0", "unmapped0", "drop", "q2", "mc"])
            if what == "secondary0":
                recs[0].flag |= 0x100
            elif what == "unmapped0":
                recs[0].flag |= 0x4
            elif what == "drop":
                recs.pop(rng.randrange(len(recs)))
            elif what == "q2":
                r = recs[rng.randrange(len(recs))]
                r.qual = bytes([2] * r.l_seq)
            else:
                r = recs[rng.randrange(len(recs))]
                r.tags = [layouts.z("MC", "7S100M3I33M") if k == b"MC" else (k, t, v) for k, t, v in r.tags]
            changed.append(gi)
        groups.append([r.encode() for r in recs])
    return GroupedReads.from_groups(groups), changed


def hostile_options(kind, head, seed):
    """random_options of the fuzz, restricted to what the head needs: no --trim on the split / seg heads, --trim on the trim head, no
    downsampling (families above --max-reads go to the host whole, background ones included), no CODEC disagreement thresholds (the
    device entry refuses those as a whole)."""
    rng = random.Random(seed)
    o = fuzz.random_options(rng, kind)
    if kind == "simplex":
        o.trim = 1 if head == "trim" else 0
        o.max_reads = -1                   # (--max-reads downsampling: the device pipeline hands every family above it to the host)
    if kind == "duplex":
        o.duplex_max_reads_per_strand = -1
    if kind == "codec":
        o.codec_max_reads_per_strand = -1
        o.codec_max_duplex_disagreements = 0xFFFFFFFF
        o.codec_max_duplex_disagreement_rate = 1.0
    return o


def _subset(g, idx):
    return GroupedReads.from_groups([g.records(i) for i in idx])


def _oracle(o, g, contigs):
    orc.set_reference(contigs)
    try:
        return orc.process(o, g.blob, g.rec_off, g.rec_len, g.grp_first, batch_groups=max(BATCH[int(o.caller_kind)], g.n_grp))
    finally:
        orc.set_reference(None)


def _set_reference(lib, h, contigs):
    if not contigs:
        return
    bufs = [C.create_string_buffer(bytes(s), max(1, len(s))) for s in contigs]
    ptrs = (C.c_void_p * len(bufs))(*[C.cast(b, C.c_void_p).value for b in bufs])
    lens = (C.c_uint64 * len(bufs))(*[len(s) for s in contigs])
    assert lib.fgx_set_reference(h, len(bufs), ptrs, lens) == 0, lib.fgx_last_error(h).decode()


def _same(what, got, want, rejects):
    if got["data"] != want["data"]:
        import bamutil
        from fgumi_amd.caller import split_records
        a, b = split_records(got["data"]), split_records(want["data"])
        for i, (x, y) in enumerate(zip(a, b)):
            if x != y:
                raise AssertionError(f"{what}: record {i} differs:\n got {bamutil.parse(x)}\nwant {bamutil.parse(y)}")
        raise AssertionError(f"{what}: {len(a)} records, the oracle {len(b)}")
    assert got["count"] == want["count"], (what, got["count"], want["count"])
    assert np.array_equal(got["stats"], want["stats"]), (what, got["stats"].tolist(), want["stats"].tolist())
    if rejects:
        assert got["n_rejects"] == want["n_rejects"] and got["rejects"] == want["rejects"], (what, got["n_rejects"], want["n_rejects"])


def _host_entry(lib, o, g, contigs):
    from fgumi_amd._lib import Options, Output
    h = lib.fgx_create(C.byref(Options.from_buffer_copy(bytes(o))))
    assert h, lib.fgx_global_error().decode()
    try:
        _set_reference(lib, h, contigs)
        out = Output()
        rc = lib.fgx_process_batch(h, g.blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, g.grp_first.ctypes.data, g.n_grp, C.byref(out))
        if rc != 0:
            return None, lib.fgx_last_error(h).decode()
        return dict(data=C.string_at(out.data, out.data_len) if out.data_len else b"", count=int(out.count), stats=np.array(list(out.stats), dtype=np.uint64),
                    rejects=C.string_at(out.rejects, out.rejects_len) if out.rejects_len else b"", n_rejects=int(out.n_rejects)), ""
    finally:
        lib.fgx_destroy(h)


def _device_entry(lib, h, g, mem):
    """fgx_process_batch_device: host arrays (the emulator) or tensors in HBM (mem == "device").  Returns (rc, result, deferred group indices)."""
    from fgumi_amd._lib import Output
    out, nd, dp = Output(), C.c_uint32(), C.c_void_p()
    keep = None
    if mem == "device":
        import torch
        from fgumi_amd._lib import hip_memcpy_d2h
        dg = g.to_device()
        keep = dg
        torch.cuda.synchronize()
        args = (dg.blob.data_ptr(), dg.blob_len, dg.rec_off.data_ptr(), dg.rec_len.data_ptr(), dg.n_rec, dg.grp_first.data_ptr(), dg.n_grp)
        fetch = hip_memcpy_d2h
    else:
        blob = np.concatenate([g.blob, np.zeros(64, dtype=np.uint8)])
        keep = blob
        args = (blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, g.grp_first.ctypes.data, g.n_grp)

        def fetch(p, n):
            return C.string_at(p, n) if n else b""
    rc = lib.fgx_process_batch_device(h, *args, C.byref(out), C.byref(nd), C.byref(dp))
    del keep
    if rc != 0:
        return rc, lib.fgx_last_error(h).decode(), []
    deferred = sorted(np.frombuffer(fetch(dp.value, 4 * nd.value), dtype=np.uint32).tolist()) if nd.value else []
    res = dict(data=fetch(out.data, out.data_len) if out.data_len else b"", count=int(out.count), stats=np.array(list(out.stats), dtype=np.uint64),
               rejects=fetch(out.rejects, out.rejects_len) if out.rejects_len else b"", n_rejects=int(out.n_rejects))
    return 0, res, deferred


def check(head, n, layout=None, hostile_seed=None, n_hostile=12, mem="host", seed=42, layout_seed=7, n_chunks=None, opts=None, guard=False, deep_hostile=None):
    """One batch through both entries against the oracle; returns the route it took."""
    from fgumi_amd._lib import Options, lib
    _debug(lib)
    kind, _, okw, _ = HEADS[head]
    g, contigs = background(head, n, seed)
    if layout:
        g = layouts.apply(layout, g, layout_seed)
    hostile = []
    if deep_hostile is not None:
        g, hostile = hostile_deep(g, deep_hostile)
        assert hostile, "no family of more than 64 records in the background"
    if hostile_seed is not None:
        g, hostile = splice(g, kind, hostile_seed, n_hostile, n_chunks)
        o = hostile_options(kind, head, hostile_seed)
        if head == "meth":
            o.methylation_mode = 1
    elif deep_hostile is not None:
        o = fgx_opts.defaults(kind=KINDS[kind], **okw)
    else:
        o = fgx_opts.defaults(kind=KINDS[kind], **okw)
    for k, v in (opts or {}).items():
        setattr(o, k, v)
    rejects = bool(o.track_rejects)
    try:
        want = _oracle(o, g, contigs)
    except RuntimeError:
        want = None
    # the host entry
    got, err = _host_entry(lib, o, g, contigs)
    if want is None:
        assert got is None, f"{head}/{layout}: the oracle refuses the batch, the host entry does not"
    else:
        assert got is not None, f"{head}/{layout}: host entry: {err}"
        _same(f"{head}/{layout} host entry", got, want, rejects)
    # the device entry
    h = lib.fgx_create(C.byref(Options.from_buffer_copy(bytes(o))))
    assert h, lib.fgx_global_error().decode()
    try:
        _set_reference(lib, h, contigs)
        rc, res, deferred = _device_entry(lib, h, g, mem)
        b = (C.c_uint64 * 4)()
        lib.fgx_debug_last_split_builds(h, b)
        route = dict(head=head, layout=layout, groups=g.n_grp, hostile=len(hostile), rc=rc, builds=list(b), routed=int(lib.fgx_debug_last_routed(h)),
                     big=int(lib.fgx_debug_last_big_families(h)), deep=int(lib.fgx_debug_last_deep_families(h)), chunks=int(lib.fgx_debug_last_split_chunks(h)),
                     meth=int(lib.fgx_debug_last_meth_device(h)), deferred=len(deferred))
        if n_chunks:
            assert route["chunks"] == n_chunks, route
            starts = chunk_starts(g.n_grp, g.n_rec, n_chunks)
            assert starts and all(b - 1 in hostile and b in hostile for b in starts), (starts, hostile)
        if guard:
            bad = lib.fgx_debug_check_guard_bands(f"{head}/{layout}".encode(), 600)
            assert bad == 0, f"{head}/{layout}: guard bands overwritten"
    finally:
        lib.fgx_destroy(h)
    if rc != 0 and rejects and "--rejects" in res and (hostile or layout):
        # documented: --rejects of duplex / CODEC on a batch with molecules the device defers, of simplex with a group out of the side
        # kernels' scope; the same batch without it still runs here
        if kind == "simplex":   # the side kernels' scope: the host twin of their source must find a group outside it
            n_out, n_rej = C.c_uint64(), C.c_uint64()
            po = Options.from_buffer_copy(bytes(o))
            scope = lib.fgx_simplex_rejects_host(C.byref(po), g.blob.ctypes.data, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.grp_first.ctypes.data, g.n_grp,
                                                 None, 0, C.byref(n_out), C.byref(n_rej))
            assert scope == 1, f"{head}/{layout}: --rejects refused, yet every group is in the side kernels' scope ({res})"
        route = check(head, n, layout, hostile_seed, n_hostile, mem, seed, layout_seed, n_chunks, dict(opts or {}, track_rejects=0), guard, deep_hostile)
        if kind != "simplex":   # duplex / CODEC refuse --rejects only when molecules are deferred
            assert route["deferred"] > 0, f"{head}/{layout}: --rejects refused with nothing deferred ({res})"
        route["refused_rejects"] = 1
        return route
    if rc != 0:
        # refusals the entry documents: --rejects of duplex / CODEC with molecules it defers; otherwise only where the oracle raises
        documented = rejects and kind != "simplex" and "--rejects" in res
        assert want is None or documented, f"{head}/{layout}: device entry refused ({res})"
        route["refused"] = res[:80]
        return route
    d = set(deferred)
    sizes = np.diff(np.asarray(g.grp_first, dtype=np.int64))
    route["deferred_upto_64"] = int(sum(1 for i in deferred if sizes[i] <= 64))   # deferred families the split pipeline's shape covers
    assert not (d - set(hostile)) or not hostile, f"{head}/{layout}: background groups deferred: {sorted(d - set(hostile))[:10]}"
    route["hostile_on_device"] = len(set(hostile) - d)
    kept = [i for i in range(g.n_grp) if i not in d]
    if want is None:
        # the oracle refuses the batch: what the device decided may stand, the deferred rest must be refused by the host entry
        got_d, err = _host_entry(lib, o, _subset(g, deferred), contigs)
        assert got_d is None, f"{head}/{layout}: the oracle refuses the batch, nothing of the product does"
        route["refused"] = err[:80]
        return route
    want_k = _oracle(o, _subset(g, kept), contigs) if d else want
    _same(f"{head}/{layout} device entry", res, want_k, False)
    stats = res["stats"].copy()
    if deferred:
        got_d, err = _host_entry(lib, o, _subset(g, deferred), contigs)
        assert got_d is not None, f"{head}/{layout}: deferred groups: {err}"
        _same(f"{head}/{layout} deferred groups", got_d, _oracle(o, _subset(g, deferred), contigs), rejects and kind != "simplex")
        stats += got_d["stats"]
    assert np.array_equal(stats, want["stats"]), (f"{head}/{layout}: counters do not add up", stats.tolist(), want["stats"].tolist())
    if rejects:   # the simplex side kernels cover every group, the deferred ones included; duplex / CODEC ran with nothing deferred
        assert res["n_rejects"] == want["n_rejects"] and res["rejects"] == want["rejects"], (f"{head}/{layout}: rejects", res["n_rejects"], want["n_rejects"])
    return route


SPLIT_HEADS = ("seg4", "packed", "pair")
PLAIN = (None, "illumina", "all_types", "duplicates")


def assert_route(r):
    """The routes the code documents, per head and layout (a route that does not hold is a finding, not a case to loosen)."""
    head, layout, n = r["head"], r["layout"], r["groups"]
    if layout == "huge_record":              # a record beyond 65 535 bytes: every kernel's `len > 0xFFFF` guard hands its family to the host
        assert r["deferred"] == n, r
        return
    if head == "seg4" and layout is None:
        assert r["chunks"] == 0 and r["routed"] == 0 and r["deferred"] == 0, r          # k_simplex_seg<4>
    if head == "seg4" and layout in ("illumina", "all_types"):
        assert r["chunks"] >= 1, r             # longer records: the mean span no longer fits seg4's quarter slice, the split pipeline takes the batch
    if head in SPLIT_HEADS and layout in PLAIN and (head != "seg4" or r["chunks"]):
        # one M op, l_name + 4 <= 48, len <= 0xFFFF: the split pipeline keeps the record whatever its aux length
        assert r["chunks"] >= 1 and r["routed"] == 0 and r["deferred"] == 0, r
    if head in ("packed", "pair") and layout == "window_edges":
        # names past the head window leave to k_simplex_wave2, nothing of up to 64 records deferred (families above 64 records with such names
        # are not all taken by the streaming kernels: some go to the host)
        assert r["chunks"] >= 1 and r["routed"] > 0 and r["deferred_upto_64"] == 0, r
    if head == "packed" and layout in PLAIN:
        assert r["builds"][2] in (1, 2) and r["builds"][0] > 0, r
    if head == "pair" and layout in PLAIN:
        assert r["builds"][2] == 2 and r["big"] == r["deep"] > 0, r
    if head == "deep" and layout in PLAIN:
        assert r["big"] == r["deep"] == n and r["deferred"] == 0, r
    if head == "wave2" and layout in PLAIN + ("window_edges",):
        assert r["chunks"] == 0 and r["deferred"] == 0, r
    if head == "seg4" and layout in ("window_edges", "duplicates"):
        assert r["chunks"] == 0 and r["deferred"] == 0, r                               # still k_simplex_seg<4>: the mean span did not grow past it
    if head == "trim" and layout in PLAIN + ("window_edges", "clipped"):
        # --trim: neither seg4 nor the split pipeline (the k_simplex_wave2 / k_family_wave<0> chain); families of up to 64 records
        assert r["chunks"] == 0 and r["builds"] == [0, 0, 0, 0] and r["big"] == 0 and r["deferred"] == 0, r
    if head == "seg4" and layout in ("window_edges", "duplicates"):
        assert r["chunks"] == 0 and r["deferred"] == 0, r                               # still k_simplex_seg<4>: the mean span did not grow past it
    if head == "trim" and layout in PLAIN + ("window_edges", "clipped"):
        # --trim: neither seg4 nor the split pipeline (the k_simplex_wave2 / k_family_wave<0> chain); families of up to 64 records
        assert r["chunks"] == 0 and r["builds"] == [0, 0, 0, 0] and r["big"] == 0 and r["deferred"] == 0, r
    if head == "meth":
        assert r["meth"] == n, r
    if head in ("duplex", "codec"):         # k_family_wave<1> / <2>: no simplex head ran
        assert r["chunks"] == 0 and r["builds"] == [0, 0, 0, 0] and r["big"] == r["deep"] == r["meth"] == 0, r
    if head in ("duplex", "codec") and layout in (None, "illumina", "window_edges", "duplicates"):
        assert r["deferred"] == 0, r


def _log(tag, r):
    print(tag, r)
    if os.environ.get("FGX_ROUTE_LOG"):           # (a JSON line per batch for the record: which head ran, what was deferred)
        with open(os.environ["FGX_ROUTE_LOG"], "a") as f:
            f.write(json.dumps(dict(r, kind=tag)) + "\n")


def check_layouts(head, n, names, mem="host"):
    """Every layout in `names` over the head's background; the routes asserted; one line per layout printed for the record."""
    for name in names:
        r = check(head, n, None if name == "plain" else name, mem=mem)
        _log("ROUTE", r)
        assert_route(r)


def check_hostile(head, n, seeds, n_hostile=10, mem="host", n_chunks=None, min_share=0.25):
    """Hostile groups spliced into the head's background, seed by seed: no background group deferred (asserted in check) and at least
    `min_share` of the hostile groups decided on the device over the seeds (the test cannot pass by deferring everything)."""
    spliced = on_device = 0
    for s in seeds:
        r = check(head, n, hostile_seed=s, n_hostile=n_hostile, mem=mem, n_chunks=n_chunks)
        _log("HOSTILE", r)
        if "refused" not in r:
            spliced += r["hostile"]
            on_device += r["hostile_on_device"]
    assert spliced > 0 and on_device >= min_share * spliced, (head, on_device, spliced)


def check_hostile_deep(n, seeds, mem="host", min_share=0.25):
    """Hostile records inside families of more than 64 records (hostile_deep), with and without --rejects: nothing but the changed families
    deferred, and at least `min_share` of them decided by the streaming kernels."""
    changed = on_device = 0
    for s in seeds:
        for opts in (None, dict(track_rejects=1)):
            r = check("deep", n, mem=mem, deep_hostile=s, opts=opts)
            _log("HOSTILE_DEEP", r)
            assert "refused" not in r, r
            assert r["big"] + r["deferred"] >= r["groups"] and r["deep"] > 0, r
            changed += r["hostile"]
            on_device += r["hostile_on_device"]
    assert changed > 0 and on_device >= min_share * changed, (on_device, changed)


def check_sample_build(n=200, mem="host"):
    """(run with FGX_SPLIT_CHUNKS=8) The build of k_split_cols chosen from the sample of the first chunk (here 32 families, fewer than the
    64 rows sampled) must not depend on what an earlier batch left in the rows past that chunk."""
    from fgumi_amd._lib import Options, lib
    _debug(lib)
    o = fgx_opts.defaults(kind=0, min_reads=1)
    g = simulate_grouped_reads(n, family_size=8, seed=5)
    tail = simulate_grouped_reads(3000, family_size=2, family_size_max=50, seed=6)
    want = _oracle(o, g, None)
    builds = []
    for warm in (None, tail):
        h = lib.fgx_create(C.byref(Options.from_buffer_copy(bytes(o))))
        assert h, lib.fgx_global_error().decode()
        try:
            if warm is not None:
                assert _device_entry(lib, h, warm, mem)[0] == 0
            rc, res, deferred = _device_entry(lib, h, g, mem)
            assert rc == 0 and not deferred, res
            _same("sample build", res, want, False)
            assert lib.fgx_debug_last_split_chunks(h) == 8
            b = (C.c_uint64 * 4)()
            lib.fgx_debug_last_split_builds(h, b)
            builds.append(list(b))
        finally:
            lib.fgx_destroy(h)
    assert builds[0][2] == builds[1][2] == 1, builds     # depth 8, every family in the packed build's shape: the packed build alone


def check_long_mi_refused(mem="host"):
    from fgumi_amd._lib import Options, lib
    g = layouts.long_values(simulate_grouped_reads(50, family_size=3), 1, mi_totals=(255,))
    o = fgx_opts.defaults(kind=0, min_reads=1)
    try:
        _oracle(o, g, None)
        raise AssertionError("the oracle accepts a 255-byte consensus name")
    except RuntimeError:
        pass
    assert _host_entry(lib, o, g, None)[0] is None
    h = lib.fgx_create(C.byref(Options.from_buffer_copy(bytes(o))))
    try:
        rc, res, deferred = _device_entry(lib, h, g, mem)
        if rc == 0:      # what the device defers must then be refused by the host entry
            assert deferred and _host_entry(lib, o, _subset(g, deferred), None)[0] is None, (res["count"], len(deferred))
    finally:
        lib.fgx_destroy(h)


def check_guarded(mem="device"):
    """(run with FGX_GUARD_BAND set) one batch each of huge_record, all_types and hostile records inside deep families (with and without
    --rejects); the bands checked after each."""
    from fgumi_amd._lib import lib
    lib.fgx_debug_check_guard_bands.restype = C.c_int
    lib.fgx_debug_check_guard_bands.argtypes = [C.c_char_p, C.c_int]
    for kw in (dict(head="packed", n=300, layout="huge_record"), dict(head="packed", n=2000, layout="all_types"), dict(head="deep", n=300, deep_hostile=8801),
               dict(head="deep", n=300, deep_hostile=8802, opts=dict(track_rejects=1))):
        r = check(kw["head"], kw["n"], kw.get("layout"), mem=mem, guard=True, deep_hostile=kw.get("deep_hostile"), opts=kw.get("opts"))
        _log("GUARDED", r)


def check_file_path(tmp_dir, n=3000):
    """An illumina-layout batch written as a BGZF BAM at level 6 and at level 0 (stored blocks, as `samtools view -u` writes them), through
    run_bam (device inflate, record boundaries, grouping by MI on the rich aux blocks, the consensus batch) against the oracle."""
    from fgumi_amd import VanillaUmiConsensusCaller, VanillaUmiConsensusOptions, bgzf
    g = layouts.illumina(simulate_grouped_reads(n, family_size=3, family_size_max=10, seed=9), 3)
    want = _oracle(fgx_opts.defaults(min_reads=1), g, None)
    refs = [("chr%d" % (i + 1), 2147483647) for i in range(24)]
    for level in (6, 0):
        src, dst = os.path.join(tmp_dir, f"grouped{level}.bam"), os.path.join(tmp_dir, f"consensus{level}.bam")
        bgzf.write_bam(src, bgzf.grouped_input_header(refs), refs, g.blob, level=level)
        raw = open(src, "rb").read()
        stored = [(raw[o + 18] >> 1) & 3 == 0 for o, _ in bgzf.bgzf_block_table(raw)[:-1]]
        assert all(stored) if level == 0 else not all(stored), level
        c = VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(min_reads=1, min_consensus_base_quality=2, cell_tag="CB"), overlapping_consensus=True)
        try:
            st = c.run_bam(src, dst, threads=8)
        finally:
            c.close()
        text, orefs, stream, off, ln = bgzf.read_bam(dst)
        got = b"".join(bytes(stream[int(o) - 4:int(o) + int(l)]) for o, l in zip(off, ln))
        assert st["device_inflate"] == 1 and st["groups"] == g.n_grp and st["kept_records"] == g.n_rec, (level, st)
        assert st["consensus_records"] == want["count"] == len(off), level
        assert got == want["data"], f"level {level}: the consensus BAM's records differ from the oracle's"
        assert st["stats"][:len(want["stats"])] == [int(v) for v in want["stats"]], level
