"""The device's BGZF inflate and deflate kernels (csrc/bgzf_device.hip) alone, through their direct entries, on the case set of
tests/inflate_cases.py: what only exists on the device — the LDS window of the payload (LdsBitReader / infl_fill_window), the LDS decode
tables of k_bgzf_tokenize / k_bgzf_inflate, the frontier schedule of k_bgzf_resolve_global, wave_crc32, the entry lists of bgzf_inflate_plan,
the choice of 8, 16, 32 or 64 tokenizer lanes, the atomicMax status word, and k_bgzf_deflate / k_bgzf_crc_write / k_bgzf_pack — against zlib.

Every inflate goes through fgx_bgzf_inflate_device_bench(reps=0): ONE pass over an output buffer filled with 0xA5, so a match the resolve pass
skipped, or copied from a byte that was not final yet, is in the bytes that come back (a second pass into the same buffer would find the
first pass's bytes there and hide it).  The device checks every block's CRC-32 itself, so a wrong kernel usually shows as the refusal of a valid
file: any refusal of a valid file is a failure.  tests/test_inflate_cases.py runs the same cases through the shared decoder core on the host."""
import ctypes as C
import random
import zlib

import pytest

import inflate_cases as ic
from fgumi_amd import VanillaUmiConsensusCaller, VanillaUmiConsensusOptions, lib, simulate_grouped_reads

pytestmark = pytest.mark.gpu

PAYLOAD = 0xFF00
REFUSED = "BGZF block %d of the chunk failed to inflate on the device"


def _caller():
    return VanillaUmiConsensusCaller("", "A", VanillaUmiConsensusOptions(min_reads=1))


def device_inflate(c, raw, cap):
    """(rc, inflated_len, bytes, error text) of one honest pass"""
    lib.fgx_bgzf_inflate_device_bench.restype = C.c_int
    lib.fgx_bgzf_inflate_device_bench.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64]
    src, out = C.create_string_buffer(raw, len(raw) + 64), C.create_string_buffer(cap + 64)
    ms, n = C.c_double(-1.0), C.c_uint64()
    rc = lib.fgx_bgzf_inflate_device_bench(c._h, src, len(raw), 0, C.byref(ms), C.byref(n), out, cap + 64)
    err = lib.fgx_last_error(c._h).decode() if rc else ""
    if rc == 0:
        assert ms.value == 0.0                                # reps == 0: the single pass, nothing timed
    return rc, n.value, out.raw[:n.value] if rc == 0 else b"", err


def device_deflate(c, data, cap=None):
    lib.fgx_bgzf_deflate_device_bench.restype = C.c_int
    lib.fgx_bgzf_deflate_device_bench.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    cap = ((len(data) + PAYLOAD - 1) // PAYLOAD) * 65536 if cap is None else cap
    out = C.create_string_buffer(max(cap, 1))
    n = C.c_uint64(12345)
    rc = lib.fgx_bgzf_deflate_device_bench(c._h, data, len(data), out, cap, C.byref(n))
    return rc, n.value, out.raw[:n.value] if rc == 0 else b"", (lib.fgx_last_error(c._h).decode() if rc else "")


def _first_difference(raw, names, want, got):
    """which block of the file holds the first wrong byte"""
    k = next((i for i in range(min(len(want), len(got))) if want[i] != got[i]), min(len(want), len(got)))
    pos = 0
    for name, (_, in_len, isize, _) in zip(names, ic.block_table(raw)):
        if pos <= k < pos + isize:
            return f"first wrong byte at {k}: byte {k - pos} of block {name} (isize {isize}, in_len {in_len}): want {want[k:k + 8].hex()} got {got[k:k + 8].hex()}"
        pos += isize
    return f"lengths differ: {len(want)} / {len(got)}"


def _check_file(c, raw, want, names, twice=True):
    for run in range(2 if twice else 1):                      # (twice in one process: the caller's device buffers are reused across calls)
        rc, n, got, err = device_inflate(c, raw, len(want))
        assert rc == 0, f"run {run}: a valid file was refused: {err}"
        assert n == len(want), (run, n, len(want))
        assert got == want, f"run {run}: " + _first_difference(raw, names, want, got)


def _group_file(group):
    if group == "E":
        frames = ic.group_e()
        raw, want = ic.file_of_frames(frames)
        return raw, want, [name for name, _, _ in frames]
    cases = getattr(ic, "group_" + group.lower())()
    raw, want = ic.file_of(cases)
    return raw, want, [name for name, _, _ in cases]


@pytest.mark.parametrize("group", ["A", "B", "C", "D", "E"])
def test_valid_files_inflate_to_what_zlib_gives(group):
    raw, want, names = _group_file(group)
    c = _caller()
    try:
        _check_file(c, raw, want, names)
    finally:
        c.close()


@pytest.mark.parametrize("n_blocks", [12, 8200, 16400, 33000])
def test_tokenizer_lane_dispatch(n_blocks):
    """bgzf_inflate_launch gives a tokenizer wavefront n / 1024 blocks, rounded up to a power of two: 12 blocks run k_bgzf_tokenize<8>, 8 200
    <16>, 16 400 <32>, 33 000 <64> (124 KB of LDS per workgroup)."""
    raw, want = ic.tiny_blocks_file(n_blocks, 77 + n_blocks)
    assert len(ic.block_table(raw)) == n_blocks
    c = _caller()
    try:
        rc, n, got, err = device_inflate(c, raw, len(want))
        assert rc == 0, err
        assert n == len(want)
        if got != want:
            k = next(i for i in range(len(want)) if want[i] != got[i])
            raise AssertionError(f"first wrong byte at {k} of {len(want)}")
    finally:
        c.close()


def check_one_phase():
    """(child process with FGX_INFL_TWO_PHASE=0: the switch is read once per process) groups A, C, D through k_bgzf_inflate"""
    import os
    assert os.environ.get("FGX_INFL_TWO_PHASE") == "0"
    c = _caller()
    for group in ("A", "C", "D"):
        raw, want, names = _group_file(group)
        _check_file(c, raw, want, names, twice=False)
    c.close()


def test_one_phase_kernel():
    from isolated import run_isolated
    run_isolated("test_gpu_bgzf_device", "check_one_phase", env={"FGX_INFL_TWO_PHASE": "0"}, timeout=120)


def check_refusals():
    """(child process) every case of group F as block 2 of a file of five blocks, between valid neighbours: refused exactly where the reference
    (zlib reaches eof, the length equals ISIZE, the CRC-32 equals the field) refuses, and the message names block 2."""
    a = {name: (p, d) for name, p, d in ic.group_a()}
    nb = [ic.frame(*a[name]) for name in ("A/isize1024", "A/isize100", "A/isize257", "A/isize4097")]
    nb_bytes = [a[name][1] for name in ("A/isize1024", "A/isize100", "A/isize257", "A/isize4097")]
    block = ic.f_block()
    payload_cases, header_cases = ic.group_f(block)
    assert len(payload_cases) == 64 and sum(1 for _, _, ok in payload_cases if not ok) >= ic.F_MIN_REFUSED
    c = _caller()
    wrong = []
    for name, blk, ref_ok in payload_cases + header_cases:
        raw = nb[0] + nb[1] + blk + nb[2] + nb[3]
        rc, n, got, err = device_inflate(c, raw, 4 * 65536)
        if ref_ok:
            if rc != 0 or got != nb_bytes[0] + nb_bytes[1] + block + nb_bytes[2] + nb_bytes[3]:
                wrong.append((name, "the reference accepts it", rc, err))
        elif rc == 0:
            wrong.append((name, "accepted, the reference refuses it"))
        elif REFUSED % 2 not in err:
            wrong.append((name, "refused, but not as block 2", err))
        elif name == "F/header/crc_flipped" and "CRC-32 mismatch" not in err:
            wrong.append((name, err))
    assert not wrong, wrong
    # blocks 1 and 3 both corrupt: the status word keeps one of them
    bad = [blk for name, blk, ok in payload_cases if not ok]
    rc, n, got, err = device_inflate(c, nb[0] + bad[0] + nb[1] + bad[-1] + nb[2], 4 * 65536)
    assert rc != 0 and (REFUSED % 1 in err or REFUSED % 3 in err), (rc, err)
    # ... and the caller inflates a valid file afterwards
    raw, want, names = _group_file("E")
    _check_file(c, raw, want, names, twice=False)
    c.close()


def test_refusals_match_the_reference():
    from isolated import run_isolated
    run_isolated("test_gpu_bgzf_device", "check_refusals", timeout=120)


# ---- deflate -------------------------------------------------------------------------------------------------------------------------------
DEFLATE_LENGTHS = [1, 2, PAYLOAD - 1, PAYLOAD, PAYLOAD + 1, 2 * PAYLOAD, 3 * PAYLOAD + 17]


def _records(n):
    fams = 400
    while True:
        blob = bytes(simulate_grouped_reads(fams, family_size=4).blob)
        if len(blob) >= n:
            return blob[:n]
        fams *= 2


def _deflate_content(kind, n):
    rng = random.Random(n * 7 + len(kind))
    if kind == "random":
        return rng.getrandbits(8 * n).to_bytes(n, "little")
    if kind == "zeros":
        return bytes(n)
    if kind == "acgt":
        return bytes(rng.choice(b"ACGT") for _ in range(n))
    if kind == "records":
        return _records(n)
    return (b"abcabcabd" * (n // 9 + 1))[:n]


def _check_deflated(c, data, kind):
    rc, n, packed, err = device_deflate(c, data)
    assert rc == 0, err
    table = ic.block_table(packed)                            # (asserts that the BSIZE chain covers out_len exactly)
    assert len(table) == (len(data) + PAYLOAD - 1) // PAYLOAD
    at = 0
    for i, (off, in_len, isize, crc) in enumerate(table):
        piece = data[i * PAYLOAD:(i + 1) * PAYLOAD]
        bsize = 18 + in_len + 8
        assert bsize <= 65536, (i, bsize)
        assert off == at + 18 and packed[at:at + 18] == bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, 6, 0, 66, 67, 2, 0, (bsize - 1) & 0xFF, (bsize - 1) >> 8]), i
        assert ic.reference_inflate(packed[off:off + in_len]) == (True, piece), (kind, len(data), i)
        assert isize == len(piece) and crc == (zlib.crc32(piece) & 0xFFFFFFFF), (kind, len(data), i)
        if kind == "random" and len(piece) == PAYLOAD:
            assert packed[off] == 0x01 and in_len == len(piece) + 5, (i, packed[off], in_len)      # the stored fallback: one final stored block
        at += bsize
    assert at == n == len(packed)
    rc, m, back, err = device_inflate(c, packed, len(data))
    assert rc == 0, err
    assert m == len(data) and back == data, (kind, len(data))


@pytest.mark.parametrize("kind", ["random", "zeros", "acgt", "records", "abcabcabd"])
def test_device_deflate_makes_valid_bgzf(kind):
    """k_bgzf_deflate / k_bgzf_crc_write / k_bgzf_pack and the scan of the block sizes: a last block of 1 byte, lengths that are an exact
    multiple of 0xFF00, content that does not compress (the stored fallback, csize == 0).  The loop over more than 16 384 lanes per launch
    (bgzf_deflate_device) needs over 1 GB of input: it stays untested here."""
    c = _caller()
    try:
        for n in DEFLATE_LENGTHS:
            _check_deflated(c, _deflate_content(kind, n), kind)
    finally:
        c.close()


def test_device_deflate_more_than_one_workgroup_of_lanes():
    """70 blocks of records: k_bgzf_deflate runs 64 lanes per workgroup, so the second workgroup's lanes (and their scratch slices) are in use"""
    c = _caller()
    try:
        _check_deflated(c, _records(70 * PAYLOAD), "records")
    finally:
        c.close()


def test_device_deflate_of_nothing_and_a_short_buffer():
    c = _caller()
    try:
        rc, n, packed, err = device_deflate(c, b"")
        assert rc == 0 and n == 0
        data = _deflate_content("random", 1000)
        rc, n, _, err = device_deflate(c, data, cap=100)
        assert rc != 0 and "output buffer" in err and n > 100, (rc, n, err)
        _check_deflated(c, data, "random")
    finally:
        c.close()
