"""Inputs and the runner of the FGX_DEEP_WIDE=1 tests (tests/test_wavemu_deep_wide.py on the CPU, tests/test_gpu_deep_wide.py on the GPU): simplex families the
streaming kernels of deep families (simplex_deep.inc) refuse for size alone — more than 512 records (1 024 under --max-reads) or an end that keeps more than
255 reads — which the wide kernels (simplex_wide.inc) decide up to 16 384 records.  Every batch is built from the simulator's families (cut to size with
GroupedReads.from_groups, bytes changed in place) and says how many of its families need the wide kernels and how many the existing builds take."""
import ctypes as C
import dataclasses
import os

import numpy as np

import fgx_opts
import orc
from max_reads_cases import READ_THROUGH, REJ_DOWNSAMPLED, families_with_a_tie_cut_in_the_middle, with_tied_names

WIDE_MAX = 16384
REJ_INSUFFICIENT_READS, REJ_ORPHAN_CONSENSUS = 1, 13            # FGX_REJ_* (include/fgumi_amd.h)
EMULATED = "FGX_LIB" in os.environ                               # the wave emulator: host arrays stand in for the tensors in HBM


@dataclasses.dataclass
class Case:
    g: object                  # GroupedReads
    wide: int                  # families that need the wide kernels
    deep: int                  # families the existing builds of the streaming kernels take
    opts: dict = dataclasses.field(default_factory=dict)
    deferred: int = 0          # families not even the wide kernels take


def _sim(n, **kw):
    from fgumi_amd import simulate_grouped_reads
    return simulate_grouped_reads(n, **kw)


def _cut(g, sizes, keep=None):
    """Family i of `g` cut to its first sizes[i] records (mates are adjacent in the simulator's families); `keep(record bytes)` filters them first."""
    from fgumi_amd import GroupedReads
    groups = []
    for gi, n in enumerate(sizes):
        recs = g.records(gi)
        if keep is not None:
            recs = [r for r in recs if keep(r)]
        assert len(recs) >= n, (gi, len(recs), n)
        groups.append(recs[:n])
    return GroupedReads.from_groups(groups)


def records_per_family(g):
    return np.diff(np.asarray(g.grp_first, dtype=np.int64))


# ---- 1. the byte edge: 255 pairs stay with k_deep_parse<256, 512>, 256 pairs are wide ---------------------------------------------------------
def byte_edge(err):
    g = _cut(_sim(2, family_size=256, error_rate_ppm=err), [510, 512])
    return Case(g, wide=1, deep=1)


# ---- 2. the record-count edges, without a cap ------------------------------------------------------------------------------------------------
def up_to_1024_records(n_families=6):
    g = _sim(n_families, family_size=270, family_size_max=500, error_rate_ppm=5000)
    n = records_per_family(g)
    assert n.min() >= 540 and n.max() <= 1024
    return Case(g, wide=n_families, deep=0)


def above_1024_records():
    g = _sim(3, family_size=600, family_size_max=700)
    n = records_per_family(g)
    assert n.min() >= 1025
    return Case(g, wide=3, deep=0)


# ---- 3. under a cap: more than DEEP_CAP_MAX records ------------------------------------------------------------------------------------------
def capped(cap, n_families=3, size=(550, 700), ties=False):
    g = _sim(n_families, family_size=size[0], family_size_max=size[1], error_rate_ppm=5000)
    n = records_per_family(g)
    assert n.min() >= 1100 and n.max() <= 1400
    if ties:
        g = with_tied_names(g)
        assert families_with_a_tie_cut_in_the_middle(g, cap) >= 1
    return Case(g, wide=n_families, deep=0, opts=dict(max_reads=cap))


# ---- 4. --min-reads 3 on read-through inserts: the min_reads-th longest read sets the length --------------------------------------------------
def read_through(n_families=3):
    g = _sim(n_families, family_size=300, family_size_max=350, **READ_THROUGH)
    n = records_per_family(g)
    assert n.min() >= 600 and n.max() <= 700
    return Case(g, wide=n_families, deep=0, opts=dict(min_reads=3))


# ---- 5. masked input ----------------------------------------------------------------------------------------------------------------------------
def with_low_qualities(g, every=37, values=(0, 1, 2, 0, 5)):
    """The batch with every `every`-th quality byte of every record replaced by one of `values` (tests/test_gpu_deep_families.py's construction)."""
    blob = np.array(g.blob, copy=True)
    k = 0
    for o in np.asarray(g.rec_off, dtype=np.int64):
        l_name, n_cig, l_seq = int(blob[o + 8]), int(blob[o + 12]) | (int(blob[o + 13]) << 8), int(blob[o + 16:o + 20].view(np.uint32)[0])
        q0 = o + 32 + l_name + 4 * n_cig + (l_seq + 1) // 2
        for i in range(every - 1 - (k % 7), l_seq, every):      # (never the first byte: 0xFF there would mean "no qualities")
            blob[q0 + i] = values[k % len(values)]
            k += 1
    assert k > 0
    return dataclasses.replace(g, blob=blob)


def masked():
    c = up_to_1024_records()
    return Case(with_low_qualities(c.g), wide=c.wide, deep=0, opts=dict(min_input_base_quality=10))


# ---- 6. UMIs --------------------------------------------------------------------------------------------------------------------------------------
def _rx_value(rec):
    """(offset, length) of the RX:Z value in a record body."""
    l_name, n_cig, l_seq = rec[8], rec[12] | (rec[13] << 8), int.from_bytes(rec[16:20], "little")
    p = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    sizes = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while p + 3 <= len(rec):
        tag, ty = rec[p:p + 2], chr(rec[p + 2])
        p += 3
        if ty == "Z":
            e = rec.index(0, p)
            if tag == b"RX":
                return p, e - p
            p = e + 1
        elif ty in sizes:
            p += sizes[ty]
        else:
            raise ValueError(f"aux type {ty} in a simulated record")
    raise ValueError("no RX tag")


def umi_disagreement():
    """Two 300-pair families: in the first every third read's RX has its first character changed in place (more than 255 observations of a UMI character,
    with disagreement); in the second every read carries the first read's RX."""
    from fgumi_amd import GroupedReads
    g = _cut(_sim(2, family_size=300, error_rate_ppm=2000), [600, 600])
    fam0 = [bytearray(r) for r in g.records(0)]
    for t in range(0, 300, 3):
        for r in fam0[2 * t:2 * t + 2]:
            o, ln = _rx_value(r)
            assert ln >= 1
            r[o] = ord("C") if r[o] == ord("A") else ord("A")
    fam1 = [bytearray(r) for r in g.records(1)]
    o0, l0 = _rx_value(fam1[0])
    value = bytes(fam1[0][o0:o0 + l0])
    for r in fam1:
        o, ln = _rx_value(r)
        assert ln == l0
        r[o:o + ln] = value
    return Case(GroupedReads.from_groups([[bytes(r) for r in fam0], [bytes(r) for r in fam1]]), wide=2, deep=0)


def umi_of_unequal_length():
    """A 300-pair family one of whose reads carries an RX one character shorter (not this path's: the general path decides) beside a family as it came."""
    from fgumi_amd import GroupedReads
    g = _cut(_sim(2, family_size=300, error_rate_ppm=2000), [600, 600])
    fam0 = [bytearray(r) for r in g.records(0)]
    o, ln = _rx_value(fam0[100])
    assert ln >= 2
    del fam0[100][o + ln - 1]
    return Case(GroupedReads.from_groups([[bytes(r) for r in fam0], g.records(1)]), wide=1, deep=0, deferred=1)


# ---- 7. an orphan end -----------------------------------------------------------------------------------------------------------------------------
def orphan_end():
    g = _cut(_sim(1, family_size=300, error_rate_ppm=2000), [300], keep=lambda r: not ((r[14] | (r[15] << 8)) & 0x80))
    return Case(g, wide=1, deep=0)


# ---- 8. the bound ---------------------------------------------------------------------------------------------------------------------------------
def the_bound():
    g = _cut(_sim(2, family_size=WIDE_MAX // 2 + 1, error_rate_ppm=2000), [WIDE_MAX, WIDE_MAX + 2])
    return Case(g, wide=1, deep=0, deferred=1)


# ---- 9. a mixed stream ----------------------------------------------------------------------------------------------------------------------------
def mixed_stream():
    from fgumi_amd import GroupedReads
    small = _sim(2000, family_size=1, family_size_max=5, error_rate_ppm=5000)
    big = _cut(_sim(3, family_size=1500, seed=7, error_rate_ppm=5000), [600, 1300, 3000])
    groups = [small.records(i) for i in range(1000)] + [big.records(i) for i in range(3)] + [small.records(i) for i in range(1000, 2000)]
    return Case(GroupedReads.from_groups(groups), wide=3, deep=0)


# ---- the runner -----------------------------------------------------------------------------------------------------------------------------------
def want_of(case, **more):
    return orc.process(fgx_opts.defaults(**dict(dict(min_reads=1), **case.opts, **more)), case.g.blob, case.g.rec_off, case.g.rec_len, case.g.grp_first)


class Caller:
    """A simplex caller of the library under test (the product's on the GPU, the wave emulator's when FGX_LIB names it) with the options of
    fgx_opts.defaults: the device entry and the host (hybrid) entry over one batch, and the path the last device batch took."""

    def __init__(self, **opts):
        from fgumi_amd._lib import Options, lib
        self.lib = lib
        self._o = fgx_opts.defaults(**dict(dict(min_reads=1), **opts))
        po = Options.from_buffer_copy(bytes(self._o))
        self.h = lib.fgx_create(C.byref(po))
        assert self.h, lib.fgx_global_error().decode()
        for f in ("fgx_debug_last_big_families", "fgx_debug_last_deep_families", "fgx_debug_last_wide_families"):
            getattr(lib, f).restype = C.c_uint32
            getattr(lib, f).argtypes = [C.c_void_p]

    def close(self):
        if self.h:
            self.lib.fgx_destroy(self.h)
            self.h = None

    def path(self):
        lib = self.lib
        return dict(big=int(lib.fgx_debug_last_big_families(self.h)), deep=int(lib.fgx_debug_last_deep_families(self.h)), wide=int(lib.fgx_debug_last_wide_families(self.h)))

    def device(self, g):
        """fgx_process_batch_device: dict(data, count, stats, deferred) + the path."""
        from fgumi_amd._lib import Output
        lib = self.lib
        out, nd, dp = Output(), C.c_uint32(), C.c_void_p()
        if EMULATED:
            blob = np.concatenate([g.blob, np.zeros(64, dtype=np.uint8)])
            keep = (blob, g.rec_off, g.rec_len, g.grp_first)
            ptrs = (blob.ctypes.data, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.grp_first.ctypes.data)
        else:
            import torch
            dg = g.to_device()
            torch.cuda.synchronize(dg.blob.device)
            keep = dg
            ptrs = (dg.blob.data_ptr(), dg.rec_off.data_ptr(), dg.rec_len.data_ptr(), dg.grp_first.data_ptr())
        rc = lib.fgx_process_batch_device(self.h, ptrs[0], g.blob.size, ptrs[1], ptrs[2], g.n_rec, ptrs[3], g.n_grp, C.byref(out), C.byref(nd), C.byref(dp))
        assert rc == 0, lib.fgx_last_error(self.h).decode()
        if not out.data_len:
            data = b""
        elif EMULATED:
            data = C.string_at(out.data, out.data_len)
        else:
            from fgumi_amd._lib import hip_memcpy_d2h
            data = hip_memcpy_d2h(out.data, out.data_len)
        del keep
        return dict(data=data, count=int(out.count), stats=np.array([int(v) for v in out.stats], dtype=np.uint64), deferred=int(nd.value), **self.path())

    def host(self, g):
        """fgx_process_batch (the hybrid entry: what the device defers, the general path decides)."""
        from fgumi_amd._lib import Output
        lib = self.lib
        out = Output()
        rc = lib.fgx_process_batch(self.h, g.blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, g.n_rec, g.grp_first.ctypes.data, g.n_grp, C.byref(out))
        assert rc == 0, lib.fgx_last_error(self.h).decode()
        data = C.string_at(out.data, out.data_len) if out.data_len else b""
        return dict(data=data, count=int(out.count), stats=np.array([int(v) for v in out.stats], dtype=np.uint64), **self.path())


def assert_equal(got, want, what=""):
    """Bytes, count and all 28 counters."""
    if got["data"] != want["data"]:
        import bamutil
        from fgumi_amd import split_records
        a, b = split_records(got["data"]), split_records(want["data"])
        for i, (x, y) in enumerate(zip(a, b)):
            assert x == y, f"{what}: record {i} differs:\n got {bamutil.parse(x)}\nwant {bamutil.parse(y)}"
        assert len(a) == len(b), f"{what}: {len(a)} records, the oracle has {len(b)}"
    assert got["count"] == want["count"] and got["data"] == want["data"], what
    assert np.array_equal(got["stats"], want["stats"]), (what, got["stats"].tolist(), want["stats"].tolist())


def check_on(case, want=None):
    """The switch is on (the environment of this process): the device entry decides the batch as the oracle does, every family on the path it was built for."""
    assert os.environ.get("FGX_DEEP_WIDE", "")[:1] not in ("", "0")
    want = want or want_of(case)
    c = Caller(**case.opts)
    try:
        got = c.device(case.g)
        path = {k: got[k] for k in ("big", "deep", "wide", "deferred")}
        print(f"path {path}", flush=True)
        assert got["deferred"] == case.deferred, path
        assert got["wide"] == case.wide and got["deep"] == case.deep, (path, case.wide, case.deep)
        if case.deferred == 0:
            assert_equal(got, want, "device entry")
        else:
            assert_equal(c.host(case.g), want, "host entry")
    finally:
        c.close()
    return want


def check_off(case, want=None):
    """The switch is off (unset, "0" or ""): every family of `case` is deferred by the device entry and the host entry returns the oracle's bytes."""
    want = want or want_of(case)
    c = Caller(**case.opts)
    try:
        got = c.device(case.g)
        assert got["wide"] == 0 and got["deferred"] == case.g.n_grp and got["deep"] == 0, got
        got = c.host(case.g)
        assert got["wide"] == 0
        assert_equal(got, want, "host entry")
    finally:
        c.close()
    return want
