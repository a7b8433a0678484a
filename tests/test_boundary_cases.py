"""The case set of tests/boundary_cases.py on the CPU: the constructed answers against the sequential walk (and the conditions each case states about its own
decoys), then the two sequential host walkers — fgx_record_boundaries and the pure-Python fallback of bgzf.record_boundaries — on every stream.  Both treat a
stream that does not end on a whole record as an error (a file, not a chunk); neither looks at block_size < 32."""
import ctypes as C

import numpy as np
import pytest

import boundary_cases as bc
from fgumi_amd import _lib, bgzf, lib

CASES = bc.all_cases()


def test_constructed_answers_equal_the_sequential_walk():
    bc.check_case_set(CASES)
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for g in ("A1", "A2", "A3", "A4", "A5", "B1", "B2", "B3", "B4", "B5", "B6", "B7", "B8"):
        assert any(n.startswith(g + "/") for n in names), g


def _whole(c):
    """does the stream, read from `start`, end on a whole record (or hold nothing at all)?"""
    return c.start >= len(c.stream) or bc.chain(c.stream, c.start)[2] == len(c.stream)


def test_fgx_record_boundaries_on_every_case():
    seen = [0, 0]
    for c in CASES:
        off, ln, _, _ = bc.chain(c.stream, c.start)
        buf = np.frombuffer(c.stream + b"\0", dtype=np.uint8)          # (never NULL, also for the empty stream; the walker is told len(stream))
        n = C.c_uint64(77)
        rc = lib.fgx_record_boundaries(buf.ctypes.data, len(c.stream), c.start, None, None, 0, C.byref(n))
        assert rc == (0 if _whole(c) else 1), c.name
        seen[rc] += 1
        if rc == 0:
            assert n.value == len(off), c.name
            goff, gln = np.full(n.value + 4, 7, dtype=np.uint64), np.full(n.value + 4, 7, dtype=np.uint32)
            assert lib.fgx_record_boundaries(buf.ctypes.data, len(c.stream), c.start, goff.ctypes.data, gln.ctypes.data, n.value, C.byref(n)) == 0
            assert np.array_equal(goff[:n.value], off) and np.array_equal(gln[:n.value], ln) and (goff[n.value:] == 7).all() and (gln[n.value:] == 7).all(), c.name
    assert min(seen) >= 10, seen


def test_python_fallback_of_record_boundaries_on_every_case(monkeypatch):
    def no_library():
        raise _lib.LibraryMissing("no library")
    monkeypatch.setattr(_lib, "load", no_library)
    for c in CASES:
        if _whole(c):
            off, ln, _, _ = bc.chain(c.stream, c.start)
            goff, gln = bgzf.record_boundaries(c.stream, c.start)
            assert np.array_equal(goff, off) and np.array_equal(gln, ln), c.name
        else:
            with pytest.raises(ValueError):
                bgzf.record_boundaries(c.stream, c.start)
