"""The case set of tests/inflate_cases.py through the decoder's three host forms (csrc/inflate_core.h compiled for the host: one-phase with the
64-lane CRC-32 fold; two-phase played in order; two-phase in k_bgzf_resolve's schedule emulated lane by lane) against zlib — so that a case
that fails on the device (tests/test_gpu_bgzf_device.py) points at the device-only code, not at the shared core — and the refusal set against
the reference's verdict, case by case, and under the guard page before any of it reaches a GPU."""
import ctypes as C
import zlib

import pytest

import inflate_cases as ic
from fgumi_amd import bgzf, lib


def one_phase(payload, n):
    """(status, bytes, CRC-32 by the device's 64-slice fold)"""
    out = C.create_string_buffer(n + 16)
    crc = C.c_uint32()
    lib.fgx_inflate_block_host.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    st = lib.fgx_inflate_block_host(payload + bytes(16), len(payload), out, n, C.byref(crc))
    return st, out.raw[:n], crc.value


def two_phase(payload, n, mode):
    """(status, bytes, entries, rounds)"""
    out = C.create_string_buffer(n + 16)
    ne, rounds = C.c_uint32(), C.c_uint32()
    lib.fgx_inflate_block_two_phase_host.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    st = lib.fgx_inflate_block_two_phase_host(payload + bytes(16), len(payload), out, n, mode, C.byref(ne), C.byref(rounds))
    return st, out.raw[:n], ne.value, rounds.value


def host_forms_accept(payload, isize, crc):
    """the verdict of each of the three host forms on a block: status 0 and the CRC-32 of what it produced equals the field"""
    st, _, c = one_phase(payload, isize)
    verdicts = [st == 0 and c == crc]
    for mode in (0, 1):
        st, out, _, _ = two_phase(payload, isize, mode)
        verdicts.append(st == 0 and (zlib.crc32(out) & 0xFFFFFFFF) == crc)
    return verdicts


def _valid_cases(group):
    if group == "E":
        out = []
        for name, blk, d in ic.group_e():
            (off, in_len, isize, crc), = ic.block_table(blk)
            assert isize == len(d)
            out.append((name, blk[off:off + in_len], d))
        return out
    return getattr(ic, "group_" + group.lower())()


@pytest.mark.parametrize("group", ["A", "B", "C", "D", "E"])
def test_host_forms_equal_zlib(group):
    for name, payload, want in _valid_cases(group):
        n = len(want)
        bound = n // 3 + n // 255 + 2
        st, out, crc = one_phase(payload, n)
        assert st == 0 and out == want, (name, st)
        assert crc == (zlib.crc32(want) & 0xFFFFFFFF), name
        for mode in (0, 1):
            st, out, ne, rounds = two_phase(payload, n, mode)
            assert st == 0 and out == want, (name, mode, st)
            assert ne <= bound, (name, ne, bound)
            if mode == 1 and name.startswith("C1/"):
                assert rounds >= ic.C1_MIN_ROUNDS, rounds         # the chain really serialises: the case is the worst one for the schedule


def test_case_set_holds_what_it_names():
    """the module's own conditions, stated once more from outside: sizes, in_len coverage, C1's shape, the entry bound of C3"""
    assert sorted(len(d) for _, _, d in ic.group_a() if d) == ic.A_SIZES
    assert sum(1 for _, _, d in ic.group_a() if not d) == len(ic.A_SIZES) // 10 + 1
    assert ic.D_IN_LENS <= {len(p) for _, p, _ in ic.group_d()}
    c = {name.split("/")[0]: (p, d) for name, p, d in ic.group_c()}
    assert len(c["C1"][1]) == 37601 and len(c["C2"][1]) == 65536 and len(c["C3"][1]) == 65536
    assert two_phase(c["C1"][0], 37601, 0)[2] == 397
    assert two_phase(c["C3"][0], 65536, 0)[2] == 21845


def test_refusals_match_the_reference():
    payload_cases, header_cases = ic.group_f(ic.f_block())
    assert sum(1 for _, _, ok in payload_cases if not ok) >= ic.F_MIN_REFUSED
    for name, blk, ref_ok in payload_cases:
        (off, in_len, isize, crc), = ic.block_table(blk)
        assert host_forms_accept(blk[off:off + in_len], isize, crc) == [ref_ok] * 3, (name, ref_ok)
    for name, blk, ref_ok in header_cases:
        (off, in_len, isize, crc), = ic.block_table(blk)
        assert not ref_ok and host_forms_accept(blk[off:off + in_len], isize, crc) == [False] * 3, name
        with pytest.raises(ValueError):                       # (the host's own block table and zlib refuse it too)
            bgzf.native_inflate(blk, 1)


def check_refusal_payloads_never_read_past_the_slack():
    """Every payload of group F at the END of a mapping whose next page is PROT_NONE, 8 bytes of slack behind it (as
    test_inflate_core.check_truncated_payloads_never_read_past_the_slack): a load past in_len + 8, by the one-phase or the tokenizing form of the
    shared decoder, is a segmentation fault of this child — no corrupt stream reaches a GPU before it has been through here."""
    import mmap
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    PAGE = mmap.PAGESIZE
    n_pages = 24
    m = mmap.mmap(-1, (n_pages + 1) * PAGE)
    base = C.addressof(C.c_char.from_buffer(m))
    assert libc.mprotect(base + n_pages * PAGE, PAGE, 0) == 0, C.get_errno()
    lib.fgx_inflate_block_host.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    two = lib.fgx_inflate_block_two_phase_host
    two.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    out = C.create_string_buffer(65536 + 64)
    payload_cases, header_cases = ic.group_f(ic.f_block())
    seen = 0
    for name, blk, ref_ok in payload_cases + header_cases:
        (off, in_len, isize, crc), = ic.block_table(blk)
        assert in_len + 8 <= n_pages * PAGE and isize <= 65536
        at = n_pages * PAGE - 8 - in_len
        m[at:at + in_len] = blk[off:off + in_len]
        m[at + in_len:n_pages * PAGE] = b"\0" * 8
        st = lib.fgx_inflate_block_host(base + at, in_len, out, isize, None)
        st2 = [two(base + at, in_len, out, isize, mode, None, None) for mode in (0, 1)]
        assert (st == 0) == (st2[0] == 0) == (st2[1] == 0), (name, st, st2)
        seen += 1
    assert seen == 68


def test_refusal_payloads_never_read_past_the_slack():
    from isolated import run_isolated
    run_isolated("test_inflate_cases", "check_refusal_payloads_never_read_past_the_slack")
