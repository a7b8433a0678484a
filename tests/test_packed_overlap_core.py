"""The overlap correction of the packed column kernel on packed words, on the HOST (fgumi_amd/csrc/packed_core.h compiled by
tests/devemu/packed_overlap.cpp: the very functions k_split_cols<.., 1> inlines in its phase 2), against the rule stated position by position:

  * ov_step at each of the eight positions of a group: all 16 x 16 code pairs x all quality pairs 0 .. 127 x floors 0, 2, 10, 11, 30, 94, 128, the
    seven other positions filled from a fixed seed — both mates' bytes and nibbles and the three counts;
  * a whole pair walked the way the kernel walks it (aligned words of the mate whose offset is 0, funnel-shifted words and XOR deltas of the other):
    every misalignment 0 .. 7 (and beyond: whole words), every overlap length 1 .. 24 and 63, 64, 65, 149, 150, the groups in any order, what lies
    outside the overlap — bytes of 128 and more included — unchanged;
  * the guard: a byte of 128 or more at a shared position is reported and nothing is written; outside the overlap it is not reported."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "devemu", "packed_overlap.cpp")
OUT = os.path.join(ROOT, "tests", "hostemu", "_build", "libpackedoverlap.so")
FLOORS = (0, 2, 10, 11, 30, 94, 128)
LENGTHS = tuple(range(1, 25)) + (63, 64, 65, 149, 150)


@pytest.fixture(scope="module")
def L():
    deps = [SRC] + [os.path.join(ROOT, "fgumi_amd", "csrc", f) for f in ("packed_core.h", "consensus_math.h", "glibc_libm.h", "glibc_tables.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        tmp = f"{OUT}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-w", SRC, "-o", tmp])
        os.replace(tmp, OUT)
    lib = C.CDLL(OUT)
    VP, U32 = C.c_void_p, C.c_uint32
    lib.pov_exhaustive.argtypes = [U32, U32, C.c_uint64, VP]
    lib.pov_exhaustive.restype = C.c_uint64
    lib.pov_pair.argtypes = [VP, VP, VP, VP, U32, U32, U32, U32, U32, VP, VP]
    lib.pov_pair.restype = C.c_int
    lib.pov_pair_rule.argtypes = [VP, VP, VP, VP, U32, U32, U32, VP]
    lib.pov_pair_rule.restype = None
    for f in (lib.pov_alignbyte, lib.pov_alignbit):
        f.argtypes = [U32, U32, U32]
        f.restype = U32
    lib.pov_popc.argtypes = [U32]
    lib.pov_popc.restype = U32
    return lib


def test_host_twins_of_the_builtins(L):
    rng = np.random.default_rng(81)
    for _ in range(300):
        hi, lo = (int(x) for x in rng.integers(0, 2 ** 32, size=2))
        w = (hi << 32) | lo
        for n in range(4):
            assert L.pov_alignbyte(hi, lo, n) == (w >> (8 * n)) & 0xFFFFFFFF
        for n in range(32):
            assert L.pov_alignbit(hi, lo, n) == (w >> n) & 0xFFFFFFFF
        assert L.pov_popc(lo) == bin(lo).count("1")
    assert L.pov_popc(0) == 0 and L.pov_popc(0xFFFFFFFF) == 32


def test_every_code_pair_and_quality_pair_at_every_position(L):
    """16 x 16 x 128 x 128 inputs per (floor, position): 56 runs of 4.2 M, spread over the cores (ctypes releases the interpreter's lock)."""
    def run(fp):
        floor, pos = fp
        first = (C.c_uint32 * 8)()
        bad = L.pov_exhaustive(floor, pos, 0x5EED0000 + 16 * floor + pos, first)
        return floor, pos, int(bad), list(first)
    jobs = [(f, p) for f in FLOORS for p in range(8)]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        res = list(ex.map(run, jobs))
    assert len(res) == 7 * 8
    wrong = [r for r in res if r[2]]
    assert not wrong, wrong[:3]


def _pack(codes):
    return ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8)


def _pair(rng, read_len, off, cn, high_outside):
    """Two reads of read_len bases in rows of whole 16-byte chunks: A shares its bases [0, cn), B its bases [off, off + cn)."""
    qs, ss = ((read_len + 15) // 16) * 16, (((read_len + 1) // 2 + 15) // 16) * 16
    def read():
        q = np.zeros(qs, dtype=np.uint8)
        q[:read_len] = rng.integers(0, 128, size=read_len)
        q[read_len:] = rng.choice([0, 65, 200, 255], size=qs - read_len)            # tag text behind the read
        c = np.zeros(2 * ss, dtype=np.uint8)
        c[:read_len] = rng.choice([1, 2, 4, 8, 15, 0, 5], size=read_len, p=[.22, .22, .22, .22, .05, .04, .03])
        return q, c
    qa, ca = read()
    qb, cb = read()
    same = rng.random(cn) < 0.5                                                     # half of the shared bases agree
    cb[off:off + cn][same] = ca[:cn][same]
    ties = rng.random(cn) < 0.1
    qb[off:off + cn][ties] = qa[:cn][ties]
    big = rng.random(cn) < 0.1                                                      # sums past the cap
    qa[:cn][big] = rng.integers(47, 128, size=int(big.sum()))
    if high_outside:                                                                # 128 and more right beside the overlap: no carry, no report
        qa[cn:read_len] = rng.integers(128, 256, size=read_len - cn)
        qb[:off] = rng.integers(128, 256, size=off)
        qb[off + cn:read_len] = rng.integers(128, 256, size=read_len - off - cn)
    return qs, ss, qa, _pack(ca), qb, _pack(cb)


def _run(L, qs, ss, qa, sa, qb, sb, off, cn, floor, order):
    got = [np.ascontiguousarray(x.copy()) for x in (qa, sa, qb, sb)]
    want = [np.ascontiguousarray(x.copy()) for x in (qa, sa, qb, sb)]
    gc, wc = np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.uint32)
    o = np.ascontiguousarray(order, dtype=np.uint32)
    guard = L.pov_pair(*(x.ctypes.data for x in got), qs, ss, off, cn, floor, o.ctypes.data, gc.ctypes.data)
    L.pov_pair_rule(*(x.ctypes.data for x in want), off, cn, floor, wc.ctypes.data)
    return guard, got, want, gc, wc


@pytest.mark.parametrize("floor", FLOORS)
def test_pairs_at_every_misalignment_and_overlap_length(L, floor):
    rng = np.random.default_rng(8000 + floor)
    seen_counts = np.zeros(3, dtype=np.int64)
    for cn in LENGTHS:
        for off in list(range(8)) + [9, 12, 16, 21]:
            for high_outside in (False, True):
                read_len = off + cn + int(rng.choice([0, 0, 1, 5, 17]))             # (0: the overlap ends with the read, in its last chunk)
                qs, ss, qa, sa, qb, sb = _pair(rng, read_len, off, cn, high_outside)
                ng = (cn + 7) // 8
                order = rng.permutation(ng) if high_outside else np.arange(ng)
                guard, got, want, gc, wc = _run(L, qs, ss, qa, sa, qb, sb, off, cn, floor, order)
                assert guard == 0, (cn, off, high_outside)
                for name, g, w in zip(("qual A", "seq A", "qual B", "seq B"), got, want):
                    assert np.array_equal(g, w), (name, cn, off, high_outside, read_len, np.flatnonzero(g != w)[:6])
                assert np.array_equal(gc, wc), (cn, off, gc, wc)
                # outside the overlap nothing moved (the rule's side says the same, by construction: checked against the inputs)
                assert np.array_equal(got[0][cn:], qa[cn:]) and np.array_equal(got[2][:off], qb[:off]) and np.array_equal(got[2][off + cn:], qb[off + cn:])
                seen_counts += wc
    assert (seen_counts > 500).all(), seen_counts


def test_the_guard_reports_a_high_byte_inside_the_overlap_only(L):
    rng = np.random.default_rng(77)
    fired = 0
    for cn in LENGTHS:
        for off in (0, 3, 5, 8):
            read_len = off + cn + 6
            qs, ss, qa, sa, qb, sb = _pair(rng, read_len, off, cn, True)
            order = np.arange((cn + 7) // 8)
            assert _run(L, qs, ss, qa, sa, qb, sb, off, cn, 10, order)[0] == 0
            for value in (128, 200, 255):
                for in_b in (False, True):
                    w = int(rng.choice([0, cn - 1, rng.integers(0, cn)]))
                    q1, q2 = qa.copy(), qb.copy()
                    (q2 if in_b else q1)[(off if in_b else 0) + w] = value
                    guard, got, _, gc, _ = _run(L, qs, ss, q1, sa, q2, sb, off, cn, 10, order)
                    assert guard == 1, (cn, off, value, in_b, w)
                    assert np.array_equal(got[0], q1) and np.array_equal(got[2], q2) and np.array_equal(got[1], sa) and np.array_equal(got[3], sb)   # reported, never added
                    assert not gc.any()
                    fired += 1
    assert fired == len(LENGTHS) * 4 * 6
