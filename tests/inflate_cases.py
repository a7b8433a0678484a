"""The case set of the BGZF inflate tests (TEST INFRASTRUCTURE; pure Python + zlib: no GPU, no product library): DEFLATE payloads at the shapes
where the device-only code around the shared decoder core can go wrong — the LDS window of the payload, the LDS decode tables, the frontier
schedule of k_bgzf_resolve_global, the 64-lane CRC-32 fold, the entry lists laid out by ISIZE, the tokenizer's lane dispatch, the status word.

A case is (name, payload, expected_bytes): `payload` is a raw DEFLATE stream, and zlib (`zlib.decompressobj(-15)`) — the REFERENCE — has
accepted it at build time and returned `expected_bytes` with `eof` set (_case asserts it: a case the reference does not accept is a bug of
the case, not of the kernel).  frame() / file_of() put cases into BGZF blocks; block_table() is the BSIZE chain as pipeline_stages.h walks it.

tests/test_inflate_cases.py runs the set through the decoder's host forms, tests/test_gpu_bgzf_device.py through the device kernels."""
import functools
import random
import zlib

EOF_PAYLOAD = b"\x03\x00"            # the empty fixed-Huffman block of the 28-byte BGZF EOF marker


# ---- builders ------------------------------------------------------------------------------------------------------------------------------
class BitWriter:
    """LSB-first bit writer (RFC 1951 3.1.1): values go in from their least significant bit, Huffman codes from their most significant one."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0
        self.total_bits = 0

    def bits(self, value, n):
        assert 0 <= value < (1 << n)
        self.acc |= value << self.n
        self.n += n
        self.total_bits += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, cl):
        code, length = cl
        rev = 0
        for _ in range(length):
            rev = (rev << 1) | (code & 1)
            code >>= 1
        self.bits(rev, length)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data
        self.total_bits += 8 * len(data)

    def getvalue(self):
        self.align()
        return bytes(self.out)


def canonical_codes(lengths):
    """{symbol: code length} -> {symbol: (code, length)}, the canonical assignment of RFC 1951 3.2.2."""
    out = {}
    code = 0
    for length in range(1, 16):
        for s in sorted(s for s, ln in lengths.items() if ln == length):
            out[s] = (code, length)
            code += 1
        code <<= 1
    return out


def flat_lengths(freq, max_len=15):
    """A complete code over the symbols of `freq` with lengths k - 1 and k only (the shorter ones to the more frequent symbols)."""
    syms = sorted(freq, key=lambda s: (-freq[s], s))
    n = len(syms)
    if n == 1:
        return {syms[0]: 1}                              # (the one incomplete code DEFLATE allows)
    k = (n - 1).bit_length()
    assert k <= max_len
    short = (1 << k) - n
    return {s: (k - 1 if i < short else k) for i, s in enumerate(syms)}


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def len_symbol(length, allowed=None):
    """(symbol, extra bits, extra value) of a match length; `allowed`: the length symbols the block's code has (257 is written with symbol
    284 + 30 where 285 would not do, as C1 needs)."""
    assert 3 <= length <= 258
    for i in range(28, -1, -1):
        if LEN_BASE[i] <= length < LEN_BASE[i] + (1 << LEN_EXTRA[i]) and (allowed is None or 257 + i in allowed):
            return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]
    raise AssertionError(("no length symbol", length))


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    for i in range(29, -1, -1):
        if DIST_BASE[i] <= dist:
            return i, DIST_EXTRA[i], dist - DIST_BASE[i]
    raise AssertionError(dist)


def rle_code_lengths(seq):
    """The code-length sequence of a dynamic header as (symbol, extra bits, extra value): zero runs of 11+ with 18, of 3 - 10 with 17 — except
    runs of 4 - 7, written as a 0 and a 16, which repeats a ZERO as well as any other length — and repeats of a non-zero length with 16."""
    out = []
    i = 0
    while i < len(seq):
        v = seq[i]
        j = i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, 7, r - 11))
                run -= r
            if 4 <= run <= 7:
                out.append((0, 0, 0))
                out.append((16, 2, run - 1 - 3))
                run = 0
            if run >= 3:
                out.append((17, 3, run - 3))
                run = 0
            out += [(0, 0, 0)] * run
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, 2, r - 3))
                run -= r
            out += [(v, 0, 0)] * run
        i = j
    return out


def play(tokens, prefix=b""):
    """The bytes a token list stands for — a literal is an int, a match a (length, distance) pair — after `prefix` (earlier blocks)."""
    out = bytearray(prefix)
    for t in tokens:
        if isinstance(t, tuple):
            length, dist = t
            assert 1 <= dist <= len(out), (t, len(out))
            for _ in range(length):
                out.append(out[-dist])
        else:
            out.append(t)
    return bytes(out[len(prefix):])


def dynamic_block(w, tokens, final, lit_lens=None, dist_lens=None, cl_lens=None, used_cl=None):
    """One dynamic-Huffman block (BTYPE 2) for `tokens` into the BitWriter.  The three codes are given as {symbol: length}, or made flat
    (flat_lengths) over the symbols the tokens use.  `used_cl` (a set) collects the code-length symbols the header wrote."""
    if lit_lens is None:
        f = {256: 1}
        for t in tokens:
            s = len_symbol(t[0])[0] if isinstance(t, tuple) else t
            f[s] = f.get(s, 0) + 1
        if len(f) == 1:
            f[0 if 0 not in f else 1] = 0                  # (a literal / length code has at least two symbols)
        lit_lens = flat_lengths(f)
    if dist_lens is None:
        f = {}
        for t in tokens:
            if isinstance(t, tuple):
                s = dist_symbol(t[1])[0]
                f[s] = f.get(s, 0) + 1
        dist_lens = flat_lengths(f) if f else {}
    lit_codes, dist_codes = canonical_codes(lit_lens), canonical_codes(dist_lens)
    hlit = max(max(lit_lens) + 1, 257)
    hdist = max(max(dist_lens) + 1 if dist_lens else 1, 1)
    seq = [lit_lens.get(s, 0) for s in range(hlit)] + [dist_lens.get(s, 0) for s in range(hdist)]
    rle = rle_code_lengths(seq)
    if cl_lens is None:
        f = {}
        for s, _, _ in rle:
            f[s] = f.get(s, 0) + 1
        if len(f) == 1:
            f[(next(iter(f)) + 1) % 19] = 0
        cl_lens = flat_lengths(f, 7)
    cl_codes = canonical_codes(cl_lens)
    hclen = max(i + 1 for i, s in enumerate(CL_ORDER) if cl_lens.get(s, 0))
    hclen = max(hclen, 4)
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.bits(cl_lens.get(s, 0), 3)
    for s, nb, v in rle:
        w.code(cl_codes[s])
        if nb:
            w.bits(v, nb)
        if used_cl is not None:
            used_cl.add(s)
    allowed = set(lit_lens)
    for t in tokens:
        if isinstance(t, tuple):
            s, nb, v = len_symbol(t[0], allowed)
            w.code(lit_codes[s])
            if nb:
                w.bits(v, nb)
            s, nb, v = dist_symbol(t[1])
            w.code(dist_codes[s])
            if nb:
                w.bits(v, nb)
        else:
            w.code(lit_codes[t])
    w.code(lit_codes[256])


def stored_block(w, data, final):
    assert len(data) <= 0xFFFF
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits(len(data) ^ 0xFFFF, 16)
    w.raw(data)


def frame(payload, data, before=b"", after=b"", crc=None, isize=None):
    """A BGZF block around a DEFLATE payload; `before` / `after`: whole extra subfields on either side of BC; crc / isize: the footer's
    fields when they are to differ from those of `data`."""
    xlen = len(before) + 6 + len(after)
    bsize = 12 + xlen + len(payload) + 8 - 1
    assert bsize <= 0xFFFF, bsize
    crc = (zlib.crc32(data) & 0xFFFFFFFF) if crc is None else crc
    isize = len(data) if isize is None else isize
    return (bytes([0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF, xlen & 0xFF, xlen >> 8]) + before + b"BC\x02\x00" + bytes([bsize & 0xFF, bsize >> 8]) + after
            + payload + crc.to_bytes(4, "little") + isize.to_bytes(4, "little"))


def subfield(si, data):
    return si + len(data).to_bytes(2, "little") + data


def file_of(cases):
    """(raw BGZF bytes, expected inflated bytes) of the cases' blocks back to back."""
    return b"".join(frame(p, d) for _, p, d in cases), b"".join(d for _, _, d in cases)


def block_table(raw):
    """The BSIZE chain as block_table (pipeline_stages.h) walks it: [(payload offset, in_len, isize, crc)] of every block."""
    out = []
    p = 0
    while len(raw) - p >= 18:
        assert raw[p:p + 3] == b"\x1f\x8b\x08" and raw[p + 3] & 4, p
        xlen = raw[p + 10] | (raw[p + 11] << 8)
        q, end, bsize = p + 12, p + 12 + xlen, 0
        while q + 4 <= end:
            slen = raw[q + 2] | (raw[q + 3] << 8)
            if q + 4 + slen > end:
                break
            if raw[q:q + 2] == b"BC" and slen == 2:
                bsize = (raw[q + 4] | (raw[q + 5] << 8)) + 1
            q += 4 + slen
        assert bsize >= 12 + xlen + 8 and len(raw) - p >= bsize, (p, bsize)
        out.append((p + 12 + xlen, bsize - 12 - xlen - 8, int.from_bytes(raw[p + bsize - 4:p + bsize], "little"), int.from_bytes(raw[p + bsize - 8:p + bsize - 4], "little")))
        p += bsize
    assert p == len(raw)
    return out


def reference_inflate(payload):
    """zlib's verdict on a raw DEFLATE stream: (reached eof, the bytes)."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload)
    except zlib.error:
        return False, b""
    return d.eof, out


def reference_accepts(payload, isize, crc):
    """The reference's verdict on a block: zlib reaches eof, the length equals ISIZE, the CRC-32 equals the field."""
    eof, out = reference_inflate(payload)
    return eof and len(out) == isize and (zlib.crc32(out) & 0xFFFFFFFF) == crc


def _case(name, payload, expected):
    eof, out = reference_inflate(payload)
    assert eof and out == expected, f"the reference does not accept case {name}"
    assert len(expected) <= 65536 and 12 + 6 + len(payload) + 8 <= 65536, name
    return (name, payload, expected)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return co.compress(data) + co.flush()


def record_like(rng, n):
    """Bytes shaped like BAM records (what the product's simulator makes, without the product library): a 36-byte fixed part whose fields
    change little from record to record, a read name, packed bases, runs of qualities, a few tags."""
    out = bytearray()
    pos = rng.randrange(1 << 20)
    fam = rng.randrange(1 << 16)
    while len(out) < n:
        l_seq = rng.choice((100, 150, 151))
        pos += rng.randrange(0, 40)
        if rng.random() < 0.2:
            fam += 1
        name = b"sim:%06d:%02d" % (fam, rng.randrange(8)) + b"\0"
        body = bytearray()
        body += (0).to_bytes(4, "little") + pos.to_bytes(4, "little") + bytes([len(name), rng.choice((20, 60)), 0x49, 0x12]) + (1).to_bytes(2, "little")
        body += rng.choice((99, 147, 83, 163)).to_bytes(2, "little") + l_seq.to_bytes(4, "little") + (0).to_bytes(4, "little") + (pos + 200).to_bytes(4, "little") + (350).to_bytes(4, "little")
        body += name + ((l_seq << 4) | 0).to_bytes(4, "little")
        body += bytes(rng.choice((0x11, 0x12, 0x14, 0x18, 0x21, 0x22, 0x24, 0x28, 0x41, 0x42, 0x44, 0x48, 0x81, 0x82, 0x84, 0x88)) for _ in range((l_seq + 1) // 2))
        q = bytearray()
        while len(q) < l_seq:
            q += bytes([rng.choice((37, 37, 37, 25, 11, 2))]) * rng.randrange(1, 40)
        body += q[:l_seq]
        body += b"MIZ%d\0" % fam + b"RXZ" + bytes(rng.choice(b"ACGT") for _ in range(8)) + b"\0"
        out += len(body).to_bytes(4, "little") + body
    return bytes(out[:n])


def mixed(rng, n):
    """a seeded mix of record-like and random bytes"""
    out = bytearray()
    while len(out) < n:
        k = rng.randrange(1, 600)
        out += record_like(rng, k) if rng.random() < 0.7 else bytes(rng.randrange(256) for _ in range(k))
    return bytes(out[:n])


# ---- A. sizes --------------------------------------------------------------------------------------------------------------------------------
A_SIZES = list(range(1, 131)) + [255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 65279, 65280, 65281, 65535]


@functools.lru_cache(maxsize=None)
def group_a():
    """One level-6 block per ISIZE of A_SIZES (odd sizes side by side: unaligned out_off; the partial first slice, empty low lanes and S = 1
    of wave_crc32; the < 8-byte tails of infl_store_pending; neighbours that must not be clobbered), an ISIZE-0 block (the EOF marker) after
    every tenth block and at the end."""
    rng = random.Random(0xA11CE)
    cases = []
    for i, n in enumerate(A_SIZES):
        d = mixed(rng, n)
        cases.append(_case(f"A/isize{n}", deflate(d, 6), d))
        if i % 10 == 9:
            cases.append(_case(f"A/empty_after_{n}", EOF_PAYLOAD, b""))
    cases.append(_case("A/empty_last", EOF_PAYLOAD, b""))
    assert sorted(len(d) for _, _, d in cases if d) == A_SIZES
    return tuple(cases)


# ---- B. encodings ----------------------------------------------------------------------------------------------------------------------------
B_ENCODINGS = [("l0", 0, zlib.Z_DEFAULT_STRATEGY), ("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l6", 6, zlib.Z_DEFAULT_STRATEGY), ("l9", 9, zlib.Z_DEFAULT_STRATEGY),
               ("fixed", 6, zlib.Z_FIXED), ("huffman_only", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE)]


def content(kind, rng, n, blob):
    """content kinds 0 .. 4 of tests/test_inflate_core.py::test_two_phase_inflate_equals_zlib (kind 2: record bytes out of `blob`)"""
    if kind == 0:
        return bytes(rng.randrange(256) for _ in range(n))
    if kind == 1:
        return bytes([rng.choice(b"ACGT")]) * n
    if kind == 2:
        o = rng.randrange(0, max(1, len(blob) - n))
        return blob[o:o + n]
    if kind == 3:
        return (b"abcabcabd" * 8000)[:n]
    unit = bytes(rng.randrange(256) for _ in range(37))
    return b"".join(unit[:k % 37] + bytes([k & 255]) for k in range(n // 19 + 40))[:n]


@functools.lru_cache(maxsize=None)
def group_b():
    """The grid of tests/test_inflate_core.py: levels 0, 1, 6, 9 and Z_FIXED / Z_HUFFMAN_ONLY / Z_RLE, content kinds 0 .. 4, n of 1, 64, 1000
    and 65280 (level 0 at 65280: two stored sub-blocks in one BGZF block)."""
    rng = random.Random(0xB0B)
    blob = record_like(rng, 200000)
    cases = []
    for tag, level, strategy in B_ENCODINGS:
        for n in (1, 64, 1000, 65280):
            for kind in range(5):
                d = content(kind, rng, n, blob)
                assert len(d) == n
                cases.append(_case(f"B/{tag}/n{n}/kind{kind}", deflate(d, level, strategy), d))
    two_stored = [p for name, p, d in cases if name.startswith("B/l0/n65280/")]
    for p in two_stored:                       # a non-final stored sub-block, then at least one more
        first = int.from_bytes(p[1:3], "little")
        assert p[0] == 0 and len(p) > 5 + first and p[5 + first] in (0, 1)
    return tuple(cases)


# ---- C. hand-assembled dynamic blocks ------------------------------------------------------------------------------------------------------
C1_LIT_SYMS = [65, 67, 71, 84, 256, 257, 285, 264, 265, 0, 255, 1, 2, 3, 4, 284]
C1_DIST_SYMS = [0, 1, 2, 3, 4, 29, 28, 10, 5, 6, 7, 8, 9, 11, 12, 13]
C1_LENGTHS = list(range(1, 15)) + [15, 15]
C1_CL_LENS = {**{s: 4 for s in range(15)}, 15: 5, 16: 6, 17: 7, 18: 7}
C1_MIN_ROUNDS = 128


def _c1():
    rng = random.Random(0xC1)
    lits = [65, 67, 71, 84, 0, 255, 1, 2, 3, 4]
    tokens = [rng.choice(lits) for _ in range(33000 - 40)] + [4, 3, 2, 1, 255, 0, 84, 71, 67, 65] * 4      # (the 15-bit literal among them)
    tokens += [(258, 32768), (3, 1), (258, 1), (258, 2), (258, 3), (258, 7), (257, 9), (12, 5), (11, 33), (227, 16385)]
    tokens += [(10, 10)] * 150                 # every match's source is the previous match's destination: a batch of 64 takes 64 rounds
    for _ in range(100):
        tokens += [rng.choice(lits), (3, 3)]
    tokens += [(258, 24577), (10, 48), (10, 49), (11, 127), (12, 128)]
    tokens += [rng.choice(lits) for _ in range(600)]
    w = BitWriter()
    used = set()
    dynamic_block(w, tokens, True, dict(zip(C1_LIT_SYMS, C1_LENGTHS)), dict(zip(C1_DIST_SYMS, C1_LENGTHS)), C1_CL_LENS, used)
    assert {16, 17, 18} <= used, used          # the header uses all three repeat codes
    d = play(tokens)
    assert len(d) == 37601 and 4 in d[:33000]
    return _case("C1/long_codes_serial_chain", w.getvalue(), d)


def _random_tokens(rng, n, pos):
    """tokens for exactly n bytes, the block beginning at output position `pos`"""
    tokens = []
    left = n
    while left:
        if left >= 3 and pos >= 1 and rng.random() < 0.5:
            length = min(rng.choice((3, 4, 5, 8, 13, 31, 32, 33, 64, 100, 258)), left)
            dist = rng.choice((1, 2, 3, 5, 8, 9, 17, 100, 1000, 32768, pos))
            dist = max(1, min(dist, pos, 32768))
            tokens.append((length, dist))
            pos += length
            left -= length
        else:
            k = min(left, rng.randrange(1, 30))
            tokens += [rng.randrange(256) for _ in range(k)]
            pos += k
            left -= k
    return tokens


def _c2():
    """a non-final dynamic block, a stored block of 700 bytes that starts in mid-byte, an empty stored block, a final dynamic block: 65 536 bytes"""
    rng = random.Random(0xC2)
    w = BitWriter()
    for n1 in range(30000, 30064):             # (the first block's length is varied until it ends in mid-byte)
        t1 = _random_tokens(random.Random(n1), n1, 0)
        w = BitWriter()
        dynamic_block(w, t1, False)
        if w.total_bits % 8 not in (0, 5):     # (0: the stored header would begin a byte; 5: its three bits would end one — no padding)
            break
    else:
        raise AssertionError("no first block that ends in mid-byte")
    d1 = play(t1)
    stored = bytes(rng.randrange(256) for _ in range(700))
    stored_block(w, stored, False)
    stored_block(w, b"", False)
    t2 = _random_tokens(rng, 65536 - len(d1) - 700, len(d1) + 700)
    dynamic_block(w, t2, True)
    d = d1 + stored + play(t2, d1 + stored)
    assert len(d) == 65536
    return _case("C2/four_deflate_blocks_isize_65536", w.getvalue(), d)


def _c3():
    """one literal, then (3, 1) up to ISIZE 65 536: the entry list at its per-ISIZE bound"""
    tokens = [0x5A] + [(3, 1)] * 21845
    w = BitWriter()
    dynamic_block(w, tokens, True)
    d = play(tokens)
    assert len(d) == 65536
    return _case("C3/entry_list_at_its_bound", w.getvalue(), d)


def _c4():
    """literal runs of exactly 254, 255, 256, 509, 510 and 511 between matches, a stored block of 255 * 3 bytes: zero-length entries in mid-batch"""
    rng = random.Random(0xC4)
    t1 = [rng.randrange(256) for _ in range(40)]
    for run in (254, 255, 256, 509, 510, 511):
        t1 += [(rng.choice((3, 9, 40)), rng.choice((1, 7, 30)))] + [rng.randrange(256) for _ in range(run)]
    t1 += [(5, 2)]
    w = BitWriter()
    dynamic_block(w, t1, False)
    d1 = play(t1)
    stored = bytes(rng.randrange(256) for _ in range(255 * 3))
    stored_block(w, stored, False)
    t2 = [(17, 255 * 3 + 4), (3, 1)] + [rng.randrange(256) for _ in range(254)] + [(258, 300)] * 30 + [rng.randrange(256) for _ in range(255)]
    dynamic_block(w, t2, True)
    return _case("C4/literal_runs_around_255", w.getvalue(), d1 + stored + play(t2, d1 + stored))


def _c5():
    """a match whose distance equals its position (it reaches the block's first byte), a match that ends exactly at ISIZE"""
    rng = random.Random(0xC5)
    tokens = [rng.randrange(256) for _ in range(40)] + [(20, 40)] + [rng.randrange(256) for _ in range(3)] + [(258, 63)]
    tokens += [rng.randrange(256) for _ in range(11)] + [(17, 332), (9, 1), (17, 9)]
    w = BitWriter()
    dynamic_block(w, tokens, True)
    return _case("C5/match_to_first_byte_and_to_isize", w.getvalue(), play(tokens))


@functools.lru_cache(maxsize=None)
def group_c():
    return (_c1(), _c2(), _c3(), _c4(), _c5())


# ---- D. payload lengths around the 128-byte input window -----------------------------------------------------------------------------------
D_IN_LENS = set(range(8, 41)) | set(range(112, 145)) | set(range(240, 273))


@functools.lru_cache(maxsize=None)
def group_d():
    """300 blocks of n = 1 .. 300 random bytes, Z_HUFFMAN_ONLY and Z_FIXED in turn, then fixed-Huffman blocks of further lengths until the
    in_len values hold every value of D_IN_LENS (the window's first fill, its end, its second fill: infl_fill_window / infl_refill)."""
    rng = random.Random(0xD0D0)
    cases = []
    for n in range(1, 301):
        d = bytes(rng.randrange(256) for _ in range(n))
        tag, strategy = (("huffman_only", zlib.Z_HUFFMAN_ONLY), ("fixed", zlib.Z_FIXED))[n & 1]
        cases.append(_case(f"D/{tag}/n{n}", deflate(d, 6, strategy), d))
    have = {len(p) for _, p, _ in cases}
    tries = 0
    while not D_IN_LENS <= have:
        tries += 1
        assert tries < 20000, sorted(D_IN_LENS - have)
        want = min(D_IN_LENS - have)
        n = max(1, int((want - 2) / 1.0625) + rng.randrange(-2, 3))
        d = bytes(rng.randrange(256) for _ in range(n))
        p = deflate(d, 6, zlib.Z_FIXED)
        if len(p) in D_IN_LENS - have:
            have.add(len(p))
            cases.append(_case(f"D/fixed/in_len{len(p)}", p, d))
    assert D_IN_LENS <= {len(p) for _, p, _ in cases}
    return tuple(cases)


# ---- E. extra subfields ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_e():
    """[(name, framed block, expected bytes)]: six blocks of group A with a second extra subfield of odd length before BC, after it, and
    both — the payload offset becomes odd, and the device must honour XLEN."""
    a = {name: (p, d) for name, p, d in group_a()}
    x, y = subfield(b"XY", b"\x01\x02\x03"), subfield(b"ZW", b"\xff" * 5)
    out = []
    for name, before, after in (("A/isize7", x, b""), ("A/isize1024", x, b""), ("A/isize100", b"", y), ("A/isize65535", b"", y), ("A/isize129", x, y), ("A/isize16385", y, x + x)):
        p, d = a[name]
        blk = frame(p, d, before, after)
        (off, in_len, isize, crc), = block_table(blk)
        assert blk[off:off + in_len] == p and isize == len(d) and crc == (zlib.crc32(d) & 0xFFFFFFFF)
        out.append((name.replace("A/", "E/"), blk, d))
    assert sum(1 for _, blk, _ in out if block_table(blk)[0][0] % 2 == 1) >= 4      # odd payload offsets
    return tuple(out)


def file_of_frames(frames):
    return b"".join(b for _, b, _ in frames), b"".join(d for _, _, d in frames)


# ---- the tokenizer's lane dispatch ---------------------------------------------------------------------------------------------------------
def tiny_blocks_file(n_blocks, seed):
    """(raw, expected) of n_blocks tiny blocks: ISIZE cycles 1 .. 40, stored and fixed-Huffman blocks in turn, one ISIZE-0 block among them
    (bgzf_inflate_launch picks 8, 16, 32 or 64 tokenizer lanes by the block count)."""
    rng = random.Random(seed)
    raw, want = [], []
    empty_at = n_blocks // 3
    for i in range(n_blocks):
        if i == empty_at:
            raw.append(frame(EOF_PAYLOAD, b""))
            continue
        n = i % 40 + 1
        d = rng.getrandbits(8 * n).to_bytes(n, "little") if i % 3 else bytes([rng.randrange(256)]) * n
        p = deflate(d, 0) if (i // 40) & 1 else deflate(d, 6, zlib.Z_FIXED)
        if i < 80 or i % 997 == 0:
            assert reference_inflate(p) == (True, d)
        raw.append(frame(p, d))
        want.append(d)
    return b"".join(raw), b"".join(want)


# ---- F. refusals -----------------------------------------------------------------------------------------------------------------------------
F_ENCODINGS = [("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l6", 6, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("l0", 0, zlib.Z_DEFAULT_STRATEGY)]
F_SEED = 0xF00D
F_MIN_REFUSED = 56


def f_block():
    """the block group F corrupts: 60 000 bytes of simulated BAM records (the one place of this module that needs the product library)"""
    from fgumi_amd import simulate_grouped_reads
    return bytes(simulate_grouped_reads(200, family_size=4).blob)[:60000]


def group_f(block):
    """`block`: 60 000 bytes of BAM records.  Returns (payload cases, header cases), each [(name, framed block, reference accepts)]:
    per encoding 12 single-bit flips of the payload and 4 truncations of in_len (BSIZE and the frame rebuilt around the shorter payload);
    then the CRC field flipped, ISIZE + 1, ISIZE - 1 and an ISIZE-0 block with a non-zero CRC.  The reference alone must refuse at least
    F_MIN_REFUSED of the 64 payload corruptions (a floor on how sharp the set is; change F_SEED if it ever fails)."""
    assert len(block) == 60000
    rng = random.Random(F_SEED)
    crc = zlib.crc32(block) & 0xFFFFFFFF
    payload_cases = []
    for tag, level, strategy in F_ENCODINGS:
        p = deflate(block, level, strategy)
        assert reference_accepts(p, len(block), crc)
        for k in range(12):
            b = bytearray(p)
            at, bit = rng.randrange(len(b)), rng.randrange(8)
            b[at] ^= 1 << bit
            payload_cases.append((f"F/{tag}/flip{k}@{at}.{bit}", frame(bytes(b), block), reference_accepts(bytes(b), len(block), crc)))
        for k in range(4):
            cut = rng.randrange(1, len(p))
            payload_cases.append((f"F/{tag}/cut{k}@{cut}", frame(p[:cut], block), reference_accepts(p[:cut], len(block), crc)))
    assert len(payload_cases) == 64
    refused = sum(1 for _, _, ok in payload_cases if not ok)
    assert refused >= F_MIN_REFUSED, refused
    p = deflate(block, 1)
    header_cases = [("F/header/crc_flipped", frame(p, block, crc=crc ^ 0x00010000), False),
                    ("F/header/isize_plus_1", frame(p, block, isize=len(block) + 1), False),
                    ("F/header/isize_minus_1", frame(p, block, isize=len(block) - 1), False),
                    ("F/header/empty_with_crc", frame(EOF_PAYLOAD, b"", crc=0xDEADBEEF), False)]
    for name, blk, _ in header_cases:
        (off, in_len, isize, c), = block_table(blk)
        assert not reference_accepts(blk[off:off + in_len], isize, c), name
    return payload_cases, header_cases
