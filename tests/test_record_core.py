"""The per-record rules of the simplex parsers on the HOST (fgumi_amd/csrc/record_core.h compiled by tests/devemu/record_core.cpp: the very functions
k_family, k_family_wave, k_simplex_wave2, k_simplex_seg, k_split_parse, k_deep_parse and k_wide_parse inline):

  * the mate clip of two single-M alignments == bam::mate_clip (bamrec.h, the op-by-op rule) == the oracle's orc_mate_clip, over the full grid
    pos, mpos 0 .. 24 x l_seq, ML 1 .. 10 x both strands of read and mate x {paired, unpaired, mate unmapped, other reference}, and at every corner of
    the ranges the 32-bit arithmetic is stated for (pos, mpos in {0, 2^30 - 1}, ML in {1, 9 999 999}, l_seq in {1, 65 535});
  * the `<n>M` reading of MC == a plain restatement ([0-9]{1,7}M, value > 0), whatever bytes follow the value;
  * the pairing hash depends on the name's bytes and its length alone — the same name inside different surrounding bytes, through the three fetch styles
    of the kernels (LDS slice, global record, the split kernel's head window) — and every byte of the name reaches a step of it;
  * the layout test and the streaming-shape rules, one record per rule at its boundary: accepted on one side, refused on the other;
  * the walk of clips around one aligned block, and the first record's MI / name rule."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "devemu", "record_core.cpp")
OUT = os.path.join(ROOT, "tests", "hostemu", "_build", "librecordcore.so")

F_PAIRED, F_UNMAPPED, F_FIRST, F_LAST, F_SECONDARY, F_SUPPLEMENTARY = 0x1, 0x4, 0x40, 0x80, 0x100, 0x800
LAYOUT_ODD, HEADER_ODD, FLAGS_ODD = 1, 2, 4


@pytest.fixture(scope="module")
def L():
    deps = [SRC] + [os.path.join(ROOT, "fgumi_amd", "csrc", f) for f in ("record_core.h", "bamrec.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        tmp = f"{OUT}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-w", SRC, "-o", tmp])
        os.replace(tmp, OUT)
    lib = C.CDLL(OUT)
    VP, U32, U64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.rcore_clip_grid.argtypes = [VP, U32, VP, U32, VP, U32, VP, U32, VP, VP, VP]
    lib.rcore_clip_grid.restype = U64
    lib.rcore_mc.argtypes = [C.c_char_p, U32, U32]
    lib.rcore_mc.restype = U32
    lib.rcore_name_hash.argtypes = [C.c_int, VP, U32, U32, VP, VP]
    lib.rcore_name_hash.restype = U32
    lib.rcore_shape.argtypes = [VP, U32, U32, C.c_int, U32, C.c_int, VP]
    lib.rcore_shape.restype = U32
    lib.rcore_single_block_op.argtypes = [U32, U32]
    lib.rcore_cigar_block.argtypes = [VP, U32, U32, VP]
    lib.rcore_cigar_block.restype = U32
    lib.rcore_first_record_odd.argtypes = [C.c_int, U32, U32]
    return lib


def _grid(L, pos, mpos, lseq, ml):
    pos, mpos = np.asarray(pos, dtype=np.int32), np.asarray(mpos, dtype=np.int32)
    lseq, ml = np.asarray(lseq, dtype=np.uint32), np.asarray(ml, dtype=np.uint32)
    n_bad, bad = C.c_uint64(0), np.zeros(8, dtype=np.int64)
    oracle = C.cast(orc.lib.orc_mate_clip, C.c_void_p)
    n = L.rcore_clip_grid(pos.ctypes.data, pos.size, mpos.ctypes.data, mpos.size, lseq.ctypes.data, lseq.size, ml.ctypes.data, ml.size, oracle, C.addressof(n_bad), bad.ctypes.data)
    assert n == pos.size * mpos.size * lseq.size * ml.size * 16
    assert n_bad.value == 0, dict(zip(("pos", "mpos", "l_seq", "ML", "flags", "closed_form", "bamrec", "oracle"), bad.tolist()), n_bad=n_bad.value)
    return n


def test_single_m_clip_over_the_full_grid(L):
    assert _grid(L, range(25), range(25), range(1, 11), range(1, 11)) == 25 * 25 * 10 * 10 * 16


def test_single_m_clip_at_the_range_corners(L):
    top = (1 << 30) - 1
    assert _grid(L, [0, top], [0, top], [1, 65535], [1, 9999999]) == 16 * 16
    # the corners' neighbourhood: reads that touch or just miss each other at the top of the range
    _grid(L, [top - 65535, top - 65534, top - 1, top], [top - 65535, top - 65534, top - 1, top], [1, 2, 65534, 65535], [1, 2, 65535, 65536, 9999999])


def _mc_plain(s):
    m = re.fullmatch(rb"[0-9]{1,7}M", s)
    return int(s[:-1]) if m and int(s[:-1]) > 0 else 0


def test_mc_single_m_reading(L):
    forms = [b"1M", b"9999999M", b"10000000M", b"0M", b"00M", b"M", b"5S", b"5M5S", b"+5M", b" 5M", b"100M", b"0000001M", b"150M", b"5MM", b"5m", b"12=", b"7X"]
    forms += [b"", b"M"] + [b"1" * k + b"M" for k in range(1, 9)] + [b"9" * k for k in range(1, 10)]      # every length 0 .. 9
    assert {len(f) for f in forms} >= set(range(10))
    for f in forms:
        for pad in (0, ord("M"), ord("7"), 0xFF):        # what lies behind the value in memory must not matter
            assert L.rcore_mc(f, len(f), pad) == _mc_plain(f), (f, pad)
    assert _mc_plain(b"9999999M") == 9999999 and _mc_plain(b"10000000M") == 0 and _mc_plain(b"00M") == 0


NAME_LENGTHS = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 254]


def _hash_plain(name):
    """The pairing hash restated: h = length; per whole 8 bytes h = rotl(h, 5) ^ lo, h = rotl(h, 11) + hi; a last step over the LAST 8 bytes (a name below 8:
    its bytes, zero-extended) when the length is no multiple of 8; h ^ h >> 15 ^ h << 7."""
    M = 0xFFFFFFFF
    rotl = lambda v, r: ((v << r) | (v >> (32 - r))) & M      # noqa: E731
    n, h, i = len(name), len(name), 0
    while i + 8 <= n:
        h = rotl(h, 5) ^ int.from_bytes(name[i:i + 4], "little")
        h = (rotl(h, 11) + int.from_bytes(name[i + 4:i + 8], "little")) & M
        i += 8
    if i < n:
        last = name[n - 8:] if n >= 8 else name + b"\0" * (8 - n)
        h = rotl(h, 5) ^ int.from_bytes(last[:4], "little")
        h = (rotl(h, 11) + int.from_bytes(last[4:], "little")) & M
    return (h ^ (h >> 15) ^ (h << 7)) & M


def test_name_hash_equals_its_plain_restatement_and_pinned_values(L):
    rng = np.random.default_rng(77)
    for n in NAME_LENGTHS + [2, 3, 20, 21, 40]:
        name = bytes(rng.integers(33, 127, size=n).astype(np.uint8))
        buf = b"\x55" * 32 + name + b"\x55" * 80
        assert _hash(L, 0, buf, 32, n) == _hash_plain(name), n
    # worked out from the restatement above, written down: a changed rotate amount, seed or final mix fails here even if both sides changed alike
    pins = {b"A": 0x01870806, b"read/1": 0x9DCFFB09, b"abcdefgh": 0x42BBB28C, b"abcdefghi": 0x460687E7, b"M01234:56:000000000-ABCDE:1:1101:15589:1332": 0xF192BE3F}
    for name, want in pins.items():
        assert _hash(L, 1, b"\0" * 32 + name + b"\0" * 80, 32, len(name)) == want == _hash_plain(name), name


def _hash(L, style, buf, off, n, steps=False):
    b = np.frombuffer(bytes(buf), dtype=np.uint8)
    if not steps:
        return L.rcore_name_hash(style, b.ctypes.data, off, n, None, None)
    st, k = np.zeros(64, dtype=np.uint64), C.c_uint32(0)
    h = L.rcore_name_hash(style, b.ctypes.data, off, n, st.ctypes.data, C.addressof(k))
    return h, st[:k.value].tolist()


@pytest.mark.parametrize("n", NAME_LENGTHS)
def test_name_hash_depends_on_the_name_and_its_length_only(L, n):
    rng = np.random.default_rng(9000 + n)
    name = bytes(rng.integers(33, 127, size=n).astype(np.uint8))
    seen = set()
    for fill in (0x00, 0xFF, 0x41, None):
        for off in (32, 33, 39, 64):                    # the record (and so the name) at any byte alignment
            pad = bytes(rng.integers(0, 256, size=off + n + 80).astype(np.uint8)) if fill is None else bytes([fill]) * (off + n + 80)
            buf = bytearray(pad)
            buf[off:off + n] = name
            for style in (0, 1, 2):
                if style == 2 and n + 5 > 48:           # (a name beyond the head window never reaches the split kernel's hash)
                    continue
                seen.add(_hash(L, style, buf, off, n))
    assert len(seen) == 1, (n, seen)
    assert next(iter(seen)) < (1 << 32)
    # the length is part of the hash: the same bytes as a shorter name give another stream of inputs (its last step differs)
    if n > 1:
        buf = bytearray(b"\0" * 32 + name + b"\0" * 80)
        assert _hash(L, 0, buf, 32, n, True)[1] != _hash(L, 0, buf, 32, n - 1, True)[1]


@pytest.mark.parametrize("n", NAME_LENGTHS)
def test_every_byte_of_the_name_reaches_a_step(L, n):
    """Sanity, not a collision bound: two names that differ in exactly one byte give different 8-byte step inputs — at a position inside the last eight
    bytes (or anywhere in a name below eight bytes) different inputs to the LAST step, elsewhere to the whole step that holds the byte."""
    rng = np.random.default_rng(9100 + n)
    name = bytearray(rng.integers(33, 127, size=n).astype(np.uint8))
    buf = bytearray(b"\xAA" * 32 + bytes(name) + b"\xAA" * 80)
    h0, s0 = _hash(L, 0, buf, 32, n, True)
    assert len(s0) == (n + 7) // 8
    for p in range(n):
        other = bytearray(buf)
        other[32 + p] ^= 0x20
        h1, s1 = _hash(L, 0, other, 32, n, True)
        assert len(s1) == len(s0) and s1 != s0, (n, p)
        if p >= n - 8:
            assert s1[-1] != s0[-1], (n, p)
        else:
            assert s1[p // 8] != s0[p // 8], (n, p)


def _hdr(pos=100, l_name=5, n_cig=1, flags=F_PAIRED | F_FIRST, l_seq=10, ref_id=0):
    return [ref_id & 0xFFFFFFFF, pos & 0xFFFFFFFF, l_name | (60 << 8), n_cig | (flags << 16), l_seq, 0, 200]


def _shape(L, d, length, max_cig=1, take_unmapped=True, head_window=0, frag_odd=False):
    a = np.array(d[:5], dtype=np.uint32)
    out = np.zeros(3, dtype=np.uint32)
    bits = L.rcore_shape(a.ctypes.data, length, max_cig, int(take_unmapped), head_window, int(frag_odd), out.ctypes.data)
    return bits, out.tolist()


def _aux_off(l_name, n_cig, l_seq):
    return 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq


def test_layout_test_at_its_boundaries(L):
    d = _hdr()
    a = _aux_off(5, 1, 10)
    bits, (so, qo, ao) = _shape(L, d, a)
    assert bits == 0 and (so, qo, ao) == (32 + 5 + 4, 32 + 5 + 4 + 5, a)          # aux_off == len: a record without tags
    assert _shape(L, d, a + 1)[0] == 0
    assert _shape(L, d, a - 1)[0] == LAYOUT_ODD                                      # aux_off == len + 1
    # l_seq 0, 1, 65 535, 65 536
    assert _shape(L, _hdr(l_seq=0), 100)[0] == HEADER_ODD
    assert _shape(L, _hdr(l_seq=1), _aux_off(5, 1, 1))[0] == 0
    assert _shape(L, _hdr(l_seq=65535), _aux_off(5, 1, 65535))[0] == 0
    assert _shape(L, _hdr(l_seq=65536), _aux_off(5, 1, 65536))[0] == LAYOUT_ODD
    assert _shape(L, _hdr(l_seq=0xFFFFFFFF), 0xFFFF)[0] & LAYOUT_ODD                 # (the offsets are summed in 64 bits: no wrap below len)
    # l_name 0 and 1 (l_name counts the NUL)
    assert _shape(L, _hdr(l_name=0), 100)[0] == LAYOUT_ODD
    assert _shape(L, _hdr(l_name=1), 100)[0] == 0


def test_streaming_shape_rules_at_their_boundaries(L):
    # n_cig 0 and 1 against the unmapped flag
    unm = F_PAIRED | F_FIRST | F_UNMAPPED
    assert _shape(L, _hdr(n_cig=1), 100)[0] == 0
    assert _shape(L, _hdr(n_cig=0), 100)[0] == HEADER_ODD
    assert _shape(L, _hdr(n_cig=2), 100)[0] == HEADER_ODD
    assert _shape(L, _hdr(n_cig=0, flags=unm), 100)[0] == 0
    assert _shape(L, _hdr(n_cig=1, flags=unm), 100)[0] == HEADER_ODD
    assert _shape(L, _hdr(n_cig=0, flags=unm), 100, take_unmapped=False)[0] == HEADER_ODD       # the methylation-aware mode, the clip-taking deep build
    # the clip-taking deep build: up to 16 ops
    assert _shape(L, _hdr(n_cig=16), 200, max_cig=16, take_unmapped=False)[0] == 0
    assert _shape(L, _hdr(n_cig=17), 200, max_cig=16, take_unmapped=False)[0] == HEADER_ODD
    assert _shape(L, _hdr(n_cig=0), 200, max_cig=16, take_unmapped=False)[0] == HEADER_ODD
    # pos -1, 0, 2^30 - 1, 2^30 (a mapped record; an unmapped one's pos is read by nobody)
    assert _shape(L, _hdr(pos=-1), 100)[0] == FLAGS_ODD
    assert _shape(L, _hdr(pos=0), 100)[0] == 0
    assert _shape(L, _hdr(pos=(1 << 30) - 1), 100)[0] == 0
    assert _shape(L, _hdr(pos=1 << 30), 100)[0] == FLAGS_ODD
    assert _shape(L, _hdr(pos=-1, n_cig=0, flags=unm), 100)[0] == 0
    # flags: secondary / supplementary; paired without FIRST or LAST; a fragment with FIRST (the split kernel's rule alone)
    assert _shape(L, _hdr(flags=F_PAIRED | F_FIRST | F_SECONDARY), 100)[0] == FLAGS_ODD
    assert _shape(L, _hdr(flags=F_PAIRED | F_LAST | F_SUPPLEMENTARY), 100)[0] == FLAGS_ODD
    assert _shape(L, _hdr(flags=F_PAIRED), 100)[0] == FLAGS_ODD
    assert _shape(L, _hdr(flags=F_PAIRED | F_LAST), 100)[0] == 0
    assert _shape(L, _hdr(flags=0), 100)[0] == 0
    assert _shape(L, _hdr(flags=F_FIRST), 100, frag_odd=False)[0] == 0
    assert _shape(L, _hdr(flags=F_FIRST), 100, frag_odd=True)[0] == FLAGS_ODD
    assert _shape(L, _hdr(flags=F_LAST), 100, frag_odd=True)[0] == FLAGS_ODD
    assert _shape(L, _hdr(flags=0), 100, frag_odd=True)[0] == 0
    # the split kernel's head window of 48 bytes: name (with its NUL) + the first CIGAR op
    assert _shape(L, _hdr(l_name=44), 200, head_window=48)[0] == 0
    assert _shape(L, _hdr(l_name=45), 200, head_window=48)[0] == HEADER_ODD
    assert _shape(L, _hdr(l_name=45), 200, head_window=0)[0] == 0
    # one M / = / X op of l_seq bases
    for t, ok in ((0, 1), (7, 1), (8, 1), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (9, 0)):
        assert L.rcore_single_block_op((10 << 4) | t, 10) == ok, t
    assert L.rcore_single_block_op((9 << 4) | 0, 10) == 0 and L.rcore_single_block_op((11 << 4) | 0, 10) == 0


def _ops(text):
    return [(int(n) << 4) | "MIDNSHP=X".index(c) for n, c in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def _reference_block(text, l_seq):
    """H* S* (M|=|X)+ S* H* with query length l_seq, restated on the text."""
    m = re.fullmatch(r"((?:\d+H)*)((?:\d+S)*)((?:\d+[M=X])+)((?:\d+S)*)((?:\d+H)*)", text)
    if not m:
        return None
    tot = lambda s: sum(int(n) for n in re.findall(r"\d+", s))      # noqa: E731
    lead, aln, trail = tot(m.group(2)), tot(m.group(3)), tot(m.group(4))
    return (lead, aln, trail, tot(text)) if aln > 0 and lead + aln + trail == l_seq else None


def test_clips_around_one_aligned_block(L):
    cases = ["10M", "3S7M", "7M3S", "2H3S5M", "3S4M3S2H", "1H1S8M1S1H", "4=2X4M", "5M5S5M", "5S", "10H", "3S7M2H1S", "2S3H5M", "5M2I3M", "5M2D5M", "4M1N6M", "5M1P5M",
             "3M3S4M", "1S1S8M", "9M", "11M", "2H10M2H"]
    for text in cases:
        ops = np.array(_ops(text), dtype=np.uint32)
        out = np.zeros(4, dtype=np.uint32)
        bits = L.rcore_cigar_block(ops.ctypes.data, ops.size, 10, out.ctypes.data)
        want = _reference_block(text, 10)
        assert bool(bits & 1) == (want is not None), (text, bits, out.tolist())
        if want:
            assert tuple(out.tolist()) == want, text
        assert bool(bits & 2) == bool(re.search(r"[IDNP]", text)), text
        assert not (bits & 2 and bits & 1), text


def test_first_record_rule(L):
    assert L.rcore_first_record_odd(0, 3, 0) == 1                          # no MI tag
    assert L.rcore_first_record_odd(1, 3, 0) == 0
    assert L.rcore_first_record_odd(1, 253, 0) == 0                        # `:<MI>` of 254 bytes + NUL: 255
    assert L.rcore_first_record_odd(1, 254, 0) == 1
    assert L.rcore_first_record_odd(1, 183, 70) == 0 and L.rcore_first_record_odd(1, 184, 70) == 1
