"""The row-loop arithmetic of the packed column pass on the HOST (fgumi_amd/csrc/packed_core.h compiled by tests/devemu/packed_rows.cpp: the very
functions k_split_cols<.., 1> inlines):

  * keep_mask without a branch (two byte permutes, one subtraction) against the bit-by-bit formulation the pass ran before, and against the plain
    statement "nibble of position p = 0xF where its quality is at or above the floor" — every quality byte, every floor 0 .. 128, every position;
  * acc_row_seq (a clean family's row: the codes alone) == acc_row on tiles that obey the invariant "code 0 under every sub-floor quality";
  * the clean test: "not clean" exactly when a byte below the floor lies at a position below its read's length — lengths 1 .. 40, floors 0, 2,
    10, 11, 128, whatever the bytes at and past the length are (tag text, NULs)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "devemu", "packed_rows.cpp")
OUT = os.path.join(ROOT, "tests", "hostemu", "_build", "libpackedrows.so")


@pytest.fixture(scope="module")
def L():
    deps = [SRC] + [os.path.join(ROOT, "fgumi_amd", "csrc", f) for f in ("packed_core.h", "consensus_math.h", "glibc_libm.h", "glibc_tables.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        tmp = f"{OUT}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-w", SRC, "-o", tmp])
        os.replace(tmp, OUT)
    lib = C.CDLL(OUT)
    VP, U32 = C.c_void_p, C.c_uint32
    lib.prow_keep_masks.argtypes = [U32, U32, U32, VP, VP]
    lib.prow_keep_masks.restype = None
    lib.prow_acc.argtypes = [VP, VP, U32, U32, U32, U32, U32, C.c_int, VP]
    lib.prow_acc.restype = None
    lib.prow_dirty.argtypes = [VP, U32, U32, VP, U32, C.c_int]
    lib.prow_dirty.restype = C.c_int
    return lib


def test_branch_free_keep_mask_equals_the_bitwise_one(L):
    new, old = np.zeros(256, dtype=np.uint32), np.zeros(256, dtype=np.uint32)
    q = np.arange(256, dtype=np.int64)
    checked = 0
    for floor in range(0, 129):
        for pos in range(8):
            for bg in (0, 9, 40, 127, 128, 255):      # the other seven qualities: below every floor, around the usual ones, at the borrow's edges
                L.prow_keep_masks(floor, pos, bg, new.ctypes.data, old.ctypes.data)
                assert np.array_equal(new, old), (floor, pos, bg, np.flatnonzero(new != old)[:4])
                # position p = nibble p ^ 1 of the sequence word (BAM packs the even position into the high nibble)
                nib = (new.astype(np.int64) >> (4 * (pos ^ 1))) & 15
                assert np.array_equal(nib, np.where(q >= floor, 15, 0)), (floor, pos, bg)
                for other in range(8):
                    if other != pos:
                        assert (((new.astype(np.int64) >> (4 * (other ^ 1))) & 15) == (15 if bg >= floor else 0)).all(), (floor, pos, bg, other)
                checked += 256
    assert checked == 129 * 8 * 6 * 256


def _pack(codes):
    return ((codes[:, 0::2] << 4) | codes[:, 1::2]).astype(np.uint8)


@pytest.mark.parametrize("floor", [0, 2, 10, 11, 30, 128])
def test_acc_row_seq_equals_acc_row_on_tiles_that_obey_the_invariant(L, floor):
    rng = np.random.default_rng(700 + floor)
    differs_without = 0
    for t in range(200):
        m, groups = int(rng.integers(1, 32)), int(rng.integers(1, 33))
        n = 8 * groups
        qual = rng.integers(0, 256, size=(m, n)).astype(np.uint8)
        qual[rng.random((m, n)) < 0.7] = rng.integers(floor, 94) if floor < 94 else 128
        codes = rng.choice([0, 1, 2, 4, 8, 15, 3], size=(m, n), p=[.1, .2, .2, .2, .2, .05, .05]).astype(np.uint8)
        raw = _pack(codes)
        codes[qual < floor] = 0                                   # the invariant: what the overlap step's `drop` leaves
        seq = _pack(codes)
        a, b, c = (np.zeros(3 * groups, dtype=np.uint32) for _ in range(3))
        q = np.ascontiguousarray(qual)
        L.prow_acc(seq.ctypes.data, q.ctypes.data, n, n // 2, m, groups, floor, 1, a.ctypes.data)
        L.prow_acc(seq.ctypes.data, q.ctypes.data, n, n // 2, m, groups, floor, 0, b.ctypes.data)
        assert np.array_equal(a, b), (t, m, groups)
        # (and acc_row of the RAW codes gives the same: clearing is what the invariant anticipates — the test is not vacuous)
        L.prow_acc(raw.ctypes.data, q.ctypes.data, n, n // 2, m, groups, floor, 1, c.ctypes.data)
        assert np.array_equal(a, c), (t, m, groups)
        L.prow_acc(raw.ctypes.data, q.ctypes.data, n, n // 2, m, groups, floor, 0, c.ctypes.data)
        differs_without += int(not np.array_equal(a, c))
    assert floor == 0 or differs_without > 150


@pytest.mark.parametrize("floor", [0, 2, 10, 11, 128])
def test_clean_test_finds_exactly_the_bytes_below_the_floor_in_front_of_l_seq(L, floor):
    rng = np.random.default_rng(900 + floor)
    seen = {0: 0, 1: 0}
    for length in range(1, 41):
        qs = ((length + 15) // 16) * 16
        for t in range(60):
            m = int(rng.integers(1, 9))
            lens = np.full(m, length, dtype=np.uint32)
            if t % 3 == 2 and length > 1:                          # reads shorter than their end's rows (one keeps the full length)
                lens[1:] = rng.integers(1, length + 1, size=m - 1)
            hi = max(floor, 1)
            qual = rng.integers(hi, max(hi + 1, 94), size=(m, qs)).astype(np.uint8) if floor < 94 else np.full((m, qs), 200, dtype=np.uint8)
            if floor == 128:
                qual[rng.random((m, qs)) < 0.5] = 128
            for j in range(m):                                     # behind the read: tag text, NULs, anything
                qual[j, lens[j]:] = rng.choice([0, 0, 1, 9, 65, 90, 255], size=qs - int(lens[j]))
            want = 0
            if floor > 0 and t % 2:
                for _ in range(int(rng.integers(1, 4))):
                    j = int(rng.integers(0, m)); p = int(rng.choice([0, lens[j] - 1, rng.integers(0, lens[j])]))
                    qual[j, p] = rng.choice([0, floor - 1, rng.integers(0, floor)])
                want = 1
            assert want == int(any((qual[j, :lens[j]] < floor).any() for j in range(m)))
            q = np.ascontiguousarray(qual)
            for per_row in (0, 1):
                got = L.prow_dirty(q.ctypes.data, qs, m, lens.ctypes.data, floor, per_row)
                assert got == want, (length, t, m, lens.tolist(), floor, per_row, got, want)
            seen[want] += 1
    assert seen[0] > 500 and (floor == 0 or seen[1] > 500)


def test_a_floor_above_128_is_never_clean(L):
    q = np.full((2, 16), 255, dtype=np.uint8)
    lens = np.array([16, 16], dtype=np.uint32)
    assert L.prow_dirty(q.ctypes.data, 16, 2, lens.ctypes.data, 129, 0) == 1
    assert L.prow_dirty(q.ctypes.data, 16, 2, lens.ctypes.data, 128, 0) == 0
