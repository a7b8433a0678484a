"""Inputs and the runner of the deep duplex tests (tests/test_wavemu_duplex_deep.py on the CPU, tests/test_gpu_duplex_deep.py on the GPU): duplex molecules of
more than 64 records, which k_family_wave<1> used to defer and the streaming kernels of fgumi_amd/csrc/duplex_deep.inc decide up to 512 records with at
most 255 retained reads per record side.  Every batch is built once from the simulator's duplex molecules (`family_size=N` gives a molecule of 2 N records —
the /A pairs first, then the /B pairs, mates adjacent — whose two record sides hold N reads each), cut to size with GroupedReads.from_groups or changed in
place, and says how many of its molecules the new kernels decide and how many the device entry defers."""
import ctypes as C
import dataclasses
import os

import numpy as np

import fgx_opts
import orc
from max_reads_cases import READ_THROUGH
from wide_cases import _rx_value, assert_equal, records_per_family, with_low_qualities

EMULATED = "FGX_LIB" in os.environ                               # the wave emulator: host arrays stand in for the tensors in HBM
REJ_FRAGMENT_READ, REJ_INSUFFICIENT_READS, REJ_ZERO_LENGTH, REJ_POTENTIAL_COLLISION = 0, 1, 11, 17       # FGX_REJ_* (include/fgumi_amd.h)
PAIRED, REVERSE, FIRST, LAST, SECONDARY = 0x1, 0x10, 0x40, 0x80, 0x100


@dataclasses.dataclass
class Case:
    g: object                  # GroupedReads
    opts: dict = dataclasses.field(default_factory=dict)
    deferred: int = 0          # molecules the device entry defers
    deep: int = -1             # molecules the new kernels decide; -1: every molecule of more than 64 records that is not deferred

    def __post_init__(self):
        if self.deep < 0:
            self.deep = int((records_per_family(self.g) > 64).sum()) - self.deferred


def _sim(n, **kw):
    from fgumi_amd import simulate_grouped_reads
    return simulate_grouped_reads(n, duplex=1, **kw)


def _groups(groups):
    from fgumi_amd import GroupedReads
    return GroupedReads.from_groups([[bytes(r) for r in recs] for recs in groups])


def _flag(rec):
    return rec[14] | (rec[15] << 8)


def _set_flag(rec, f):
    rec[14], rec[15] = f & 0xFF, f >> 8


def _tag_value(rec, want):
    """(offset, length) of the Z value of tag `want` in a record body."""
    l_name, n_cig, l_seq = rec[8], rec[12] | (rec[13] << 8), int.from_bytes(rec[16:20], "little")
    p = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    sizes = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while p + 3 <= len(rec):
        tag, ty = bytes(rec[p:p + 2]), chr(rec[p + 2])
        p += 3
        if ty == "Z":
            e = rec.index(0, p)
            if tag == want:
                return p, e - p
            p = e + 1
        else:
            p += sizes[ty]
    raise ValueError(f"no {want} tag")


def _strand(rec):
    o, ln = _tag_value(rec, b"MI")
    return chr(rec[o + ln - 1])


def _with_cigar(rec, ops):
    """The record with its CIGAR replaced by `ops` (op length << 4 | kind)."""
    l_name, n_cig = rec[8], rec[12] | (rec[13] << 8)
    p = 32 + l_name
    out = bytearray(rec[:p]) + b"".join(int(o).to_bytes(4, "little") for o in ops) + bytearray(rec[p + 4 * n_cig:])
    out[12], out[13] = len(ops) & 0xFF, len(ops) >> 8
    return out


# ---- 1. the lower edge: 32 pairs are k_family_wave's, 33 pairs the new kernels' ---------------------------------------------------------------------
def lower_edge():
    g = _sim(2, family_size=33)
    return Case(_groups([g.records(0)[:64], g.records(1)]))


# ---- 2. integer tag types: cD is type c up to 127 and type C above --------------------------------------------------------------------------------------
def pairs(n_pairs, n_molecules=1, err=1000):
    return Case(_sim(n_molecules, family_size=n_pairs, error_rate_ppm=err))


def cd_types(data):
    """(type, value) of the cD tag of every record of a consensus stream."""
    import bamutil
    from fgumi_amd import split_records
    return [bamutil.parse(r)["tags"]["cD"] for r in split_records(data)]


# ---- 3. the bound: 255 pairs are decided, 256 pairs are deferred -------------------------------------------------------------------------------------
def the_bound():
    g = _sim(2, family_size=256)
    c = Case(_groups([g.records(0)[2:], g.records(1)]), deferred=1)      # the first molecule without its first /A template
    assert records_per_family(c.g).tolist() == [510, 512]
    return c


# ---- 4 / 5. error rates; the long tail and its option matrix ---------------------------------------------------------------------------------------------
def long_tail(n=3, **sim):
    g = _sim(n, **dict(dict(family_size=40, family_size_max=250), **sim))
    assert records_per_family(g).min() >= 80
    return g


OPTION_MATRIX = {
    "min_reads_3_2_1": dict(duplex_min_reads=(3, 2, 1)),
    "min_reads_2_1_0": dict(duplex_min_reads=(2, 1, 0)),
    "min_reads_6_3_3": dict(duplex_min_reads=(6, 3, 3)),
    "overlapping_off": dict(overlapping_consensus=0),
    "per_base_tags_off": dict(produce_per_base_tags=0),
    "min_input_base_quality_30": dict(min_input_base_quality=30),
    "error_rates_30_25": dict(error_rate_pre_umi=30, error_rate_post_umi=25),
    "tie_rule_1": dict(tie_rule=1),
    "long_prefix": dict(read_name_prefix=b"p" * 60),                # the per-field record writer
    "reads_of_300_bases": dict(),                                   # records above 256 positions
}


def option_case(name):
    sim = dict(read_length=300, insert_mean=500) if name == "reads_of_300_bases" else {}
    return Case(long_tail(**sim), opts=OPTION_MATRIX[name])


# ---- 6. read-through inserts with masked input ---------------------------------------------------------------------------------------------------------
def read_through():
    g = with_low_qualities(_sim(3, family_size=40, family_size_max=120, **READ_THROUGH))
    blob = np.array(g.blob, copy=True)
    for gi in range(g.n_grp):                                      # one template per molecule with every quality at 2 (both mates: agreeing mates ADD their qualities)
        for k in (4, 5):
            o = int(g.rec_off[int(g.grp_first[gi]) + k])
            l_name, n_cig, l_seq = int(blob[o + 8]), int(blob[o + 12]) | (int(blob[o + 13]) << 8), int(blob[o + 16:o + 20].view(np.uint32)[0])
            q0 = o + 32 + l_name + 4 * n_cig + (l_seq + 1) // 2
            blob[q0:q0 + l_seq] = 2
    return Case(dataclasses.replace(g, blob=blob))


# ---- 7. strand shapes, built by filtering a simulated molecule's records ----------------------------------------------------------------------------
def only_a_strand(min_reads):
    recs = [r for r in _sim(1, family_size=80).records(0) if _strand(r) == "A"][:80]
    assert len(recs) == 80
    return Case(_groups([recs]), opts=dict(duplex_min_reads=min_reads))


def single_read_sets():
    recs = _sim(1, family_size=90).records(0)      # (the simulator draws a molecule's strand split: this one has 73 /A and 17 /B templates)
    a, b = [r for r in recs if _strand(r) == "A"], [r for r in recs if _strand(r) == "B"]
    assert len(a) >= 120 and len(b) >= 2
    return Case(_groups([a[:120] + b[:2]]))


def stray_fragments():
    recs = [bytearray(r) for r in _sim(1, family_size=50).records(0)]
    for r in recs[6:8] + recs[70:72]:                             # both mates of two templates become fragment records
        _set_flag(r, _flag(r) & ~(PAIRED | 0x2 | 0x8 | 0x20 | FIRST | LAST))
    return Case(_groups([recs]))


def strand_collision():
    recs = [bytearray(r) for r in _sim(1, family_size=50).records(0)]
    for r in recs[0:2]:                                            # one /A template relabelled /B: its R2 lies on the other strand than the /A R1s
        o, ln = _tag_value(r, b"MI")
        assert r[o + ln - 1] == ord("A")
        r[o + ln - 1] = ord("B")
    return Case(_groups([recs]))


def r1_only():
    recs = [r for r in _sim(1, family_size=90).records(0) if _flag(r) & FIRST]
    assert len(recs) == 90
    return Case(_groups([recs]))


# ---- 8. UMIs ----------------------------------------------------------------------------------------------------------------------------------------------
def umi_disagreement():
    recs = [bytearray(r) for r in _sim(1, family_size=100, error_rate_ppm=2000).records(0)]
    for t in range(0, 100, 3):
        for r in recs[2 * t:2 * t + 2]:
            o, ln = _rx_value(r)
            r[o] = ord("C") if r[o] == ord("A") else ord("A")
    return Case(_groups([recs]))


def paired_umi():
    """RX becomes `<3 bases>-<4 bases>` in place; the reads of the /B strand carry the halves swapped."""
    recs = [bytearray(r) for r in _sim(1, family_size=60).records(0)]
    for r in recs:
        o, ln = _rx_value(r)
        assert ln == 8
        left, right = bytes(r[o:o + 3]), bytes(r[o + 4:o + 8])
        r[o:o + ln] = (left + b"-" + right) if _strand(r) == "A" else (right + b"-" + left)
    return Case(_groups([recs]))


def no_rx():
    recs = []
    for r in _sim(1, family_size=50).records(0):
        o, ln = _rx_value(r)
        recs.append(r[:o - 3] + r[o + ln + 1:])
    return Case(_groups([recs]))


def umi_of_unequal_length():
    """A molecule one of whose reads carries an RX one character shorter (the general path's: the reference refuses it) beside a molecule as it came."""
    g = _sim(2, family_size=50)
    m0 = [bytearray(r) for r in g.records(0)]
    o, ln = _rx_value(m0[20])
    del m0[20][o + ln - 1]
    return Case(_groups([m0, g.records(1)]), deferred=1)


# ---- 9. not this path's ---------------------------------------------------------------------------------------------------------------------------------
def not_this_path(what):
    recs = [bytearray(r) for r in _sim(1, family_size=40).records(0)]
    r = recs[10]
    l_seq = int.from_bytes(r[16:20], "little")
    if what == "deletion":
        recs[10] = _with_cigar(r, [(40 << 4) | 0, (2 << 4) | 2, ((l_seq - 40) << 4) | 0])
    elif what == "soft_clip":
        recs[10] = _with_cigar(r, [(5 << 4) | 4, ((l_seq - 5) << 4) | 0])
    else:
        _set_flag(r, _flag(r) | SECONDARY)
    return Case(_groups([recs]), deferred=1)


# ---- 10. options that keep the path off -----------------------------------------------------------------------------------------------------------------
def path_off_case(what):
    g = _sim(3, family_size=40)
    opts = dict(trim=dict(trim=1), rejects=dict(track_rejects=1), cap=dict(duplex_max_reads_per_strand=20), methylation=dict(methylation_mode=1))[what]
    return Case(g, opts=opts, deferred=3)


def methylation_contigs():
    import methsim
    return methsim.genome(methsim.seeded(71))


# ---- 12 / 13. a shallow batch; a mixed stream -------------------------------------------------------------------------------------------------------------
def shallow():
    return Case(_sim(500, family_size=12))


def mixed_stream():
    small = _sim(2000, family_size=1, family_size_max=5, error_rate_ppm=5000)
    big = _sim(3, family_size=255, seed=7, error_rate_ppm=5000)
    deep = [big.records(0)[:40] + big.records(0)[306:332], big.records(1)[:180] + big.records(1)[306:426], big.records(2)]       # 66, 300 and 510 records
    groups = [small.records(i) for i in range(1000)] + deep + [small.records(i) for i in range(1000, 2000)]
    c = Case(_groups(groups))
    assert sorted(records_per_family(c.g).tolist())[-3:] == [66, 300, 510] and c.deep == 3
    return c


# ---- the runner -----------------------------------------------------------------------------------------------------------------------------------------
def options_of(case, **more):
    return fgx_opts.defaults(kind=1, **dict(case.opts, **more))


def want_of(case, contigs=None, **more):
    orc.set_reference(contigs)
    try:
        return orc.process(options_of(case, **more), case.g.blob, case.g.rec_off, case.g.rec_len, case.g.grp_first, batch_groups=100)
    finally:
        orc.set_reference(None)


class Caller:
    """A duplex caller of the library under test (the product's on the GPU, the wave emulator's when FGX_LIB names it): the device entry and the host (hybrid)
    entry over one batch, and the path the last device batch took."""

    def __init__(self, contigs=None, **opts):
        from fgumi_amd._lib import Options, lib
        self.lib = lib
        self._o = fgx_opts.defaults(kind=1, **opts)
        po = Options.from_buffer_copy(bytes(self._o))
        self.h = lib.fgx_create(C.byref(po))
        assert self.h, lib.fgx_global_error().decode()
        for f in ("fgx_debug_last_big_families", "fgx_debug_last_deep_families", "fgx_debug_last_duplex_deep"):
            getattr(lib, f).restype = C.c_uint32
            getattr(lib, f).argtypes = [C.c_void_p]
        lib.fgx_debug_last_chain.restype = None
        lib.fgx_debug_last_chain.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        if contigs:
            bufs = [C.create_string_buffer(bytes(s), max(1, len(s))) for s in contigs]
            ptrs = (C.c_void_p * len(bufs))(*[C.cast(b, C.c_void_p).value for b in bufs])
            lens = (C.c_uint64 * len(bufs))(*[len(s) for s in contigs])
            assert lib.fgx_set_reference(self.h, len(bufs), ptrs, lens) == 0, lib.fgx_last_error(self.h).decode()

    def close(self):
        if self.h:
            self.lib.fgx_destroy(self.h)
            self.h = None

    def path(self):
        lib = self.lib
        return dict(big=int(lib.fgx_debug_last_big_families(self.h)), deep=int(lib.fgx_debug_last_deep_families(self.h)), duplex_deep=int(lib.fgx_debug_last_duplex_deep(self.h)))

    def chain(self):
        """(kernel launches, host synchronisations) of the last device batch, as tests/record_rule_cases.py reads them."""
        ch = (C.c_uint32 * 2)()
        self.lib.fgx_debug_last_chain(self.h, ch)
        return int(ch[0]), int(ch[1])

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


PATH_KEYS = ("deferred", "duplex_deep", "big", "deep")


def check(case, want=None, contigs=None):
    """Both entries against the oracle, and the path of the device batch: `case.deferred` molecules deferred, `case.deep` decided by the new kernels, nothing
    counted as a simplex big / deep family.  With nothing deferred the device entry's bytes, count and 28 counters are the oracle's; the host entry's always are."""
    want = want or want_of(case, contigs)
    c = Caller(contigs, **case.opts)
    try:
        got = c.device(case.g)
        path = {k: got[k] for k in PATH_KEYS}
        print(f"path {path}", flush=True)
        assert got["deferred"] == case.deferred and got["duplex_deep"] == case.deep and got["big"] == 0 and got["deep"] == 0, (path, case.deferred, case.deep)
        if case.deferred == 0:
            assert_equal(got, want, "device entry")
        assert_equal(c.host(case.g), want, "host entry")
    finally:
        c.close()
    return want


def check_deferred_beside_decided(case, want_first):
    """`case`: two molecules, the second deferred — the device entry's bytes are the oracle's for the first molecule alone (`want_first`)."""
    c = Caller(**case.opts)
    try:
        got = c.device(case.g)
        assert got["deferred"] == 1 and got["duplex_deep"] == 1 and got["big"] == 0 and got["deep"] == 0, {k: got[k] for k in PATH_KEYS}
        assert got["data"] == want_first["data"] and got["count"] == want_first["count"]
    finally:
        c.close()
