"""Inputs of the FindBoundaries tests of boundaries.hip (check_boundary_kernels_on_hostile_streams in tests/test_apiemu.py on the CPU, tests/test_gpu_boundaries.py
on the GPU, tests/test_boundary_cases.py for the sequential host walkers) and the one runner the first two use (TEST INFRASTRUCTURE).

A case is (name, stream, start, want).  `Stream` lays records end to end and keeps the books while it does: the body offset and length of every whole record,
where the last whole record ends (`consumed`), whether a whole record has a block_size below 32 ("malformed").  That bookkeeping is the case's answer; `chain`, a
plain sequential walk of the block_size chain, is the second reference, and `check_case_set` holds the two to each other before any product code runs.

What boundaries.hip does with a stream (the kernels' own comments): a thread per SEG-byte segment GUESSES the first record start of its segment (the first offset
whose bytes look like a record followed by two more), walks on from there, and the walks are checked against each other from the given first record on; a wrong
guess costs repair rounds and must cost nothing else.  The groups:
  A  segment geometry without decoys: records that end on / start around a segment edge, short streams, start offsets, segments without any record start.
     Every guess is right: 0 repair rounds.
  B  decoys: whole fake record chains in the B:C payload of a true record (at least three links, so that the guess takes them), placed where a segment's guess
     meets them before any true start; fake links that jump far, point past the end or are malformed; true malformed records.  At least 1 repair round.
  C  the contract of the entry (cap, poisoned output arrays), D  one caller over all cases in a shuffled order (scratch of a longer table under a shorter one).
`guess` restates k_bound_guess in Python for one purpose only: to state, as conditions on the INPUT, which segments a case's decoys take (none in A, at least
one in B, at least 64 in B1, the named ones in B7).  No expected answer depends on it."""
import bisect
import ctypes as C
import dataclasses
import random
import struct

import numpy as np

import bamutil

SEG = 16384          # bytes per segment          (fgumi_amd/csrc/boundaries.hip: constexpr uint32_t SEG)
BLOCK = 256          # segments per thread block  (boundaries.hip: record_boundaries_device launches blocks of 256 threads)
NONE = -1            # "no record starts in this segment"
SPARE = 100          # elements behind `cap` in the output arrays: poisoned, and must stay so

# ---- records -----------------------------------------------------------------------------------------------------------------------------------------------

CORE = bamutil.make_record("r0001", ("ACGT" * 38)[:150], [30] * 150, flag=0, ref_id=0, pos=1234)       # a mapped 150 bp read, 150M; aux bytes are appended to it
S = 4 + len(CORE)                                                                                       # ... as it stands in a stream
MINI = bamutil.make_record("q", "", [], flag=0x4, ref_id=-1, pos=-1)                                   # the smallest record the guess accepts: 34 bytes
FAKE = bamutil.make_record("fake", "ACGT" * 10, [30] * 40, flag=0x4, ref_id=-1, pos=-1)                # the body of a fake link


def zfit(n):
    """`n` aux bytes: nothing, or one Z tag (4 bytes at least)"""
    assert n == 0 or n >= 4, n
    return b"" if n == 0 else b"XZZ" + b"x" * (n - 4) + b"\0"


def link(block_size=None):
    """a fake record as it would stand in a stream; `block_size` overrides the prefix (a far jump, a terminal link)"""
    return struct.pack("<I", len(FAKE) if block_size is None else block_size) + FAKE


F = len(link())
BAD_LINK = struct.pack("<I", 8) + bytes(8)                    # a fake link with block_size 8


def carrier(payload):
    """a true record whose B:C array is `payload`"""
    return CORE + b"zzBC" + struct.pack("<I", len(payload)) + payload


HEAD = S + 8                                                  # from a carrier's block_size prefix to the first byte of its payload
LONG = CORE + zfit(5 * SEG)                                   # a record of 5 segments and a bit


@dataclasses.dataclass
class Want:
    rc: int                    # 0, or 1 = malformed (a whole record with block_size < 32)
    off: np.ndarray            # body offsets
    len: np.ndarray
    consumed: int


@dataclasses.dataclass
class Case:
    name: str
    stream: bytes
    start: int
    want: Want

    @property
    def group(self):
        return self.name[0]

    @property
    def n_seg(self):
        return (len(self.stream) + SEG - 1) // SEG


class Stream:
    """Records laid end to end behind `header` bytes (the BAM header of the pipeline: `start` = its length)."""

    def __init__(self, header=b""):
        self.parts, self.pos, self.start = [bytes(header)], len(header), len(header)
        self.off, self.len, self.consumed, self.bad, self.closed = [], [], len(header), False, False

    def add(self, body, times=1):
        assert not self.closed
        rec = struct.pack("<I", len(body)) + body
        for _ in range(times):
            self.off.append(self.pos + 4)
            self.len.append(len(body))
            self.pos += len(rec)
        self.parts.append(rec * times)
        self.consumed = self.pos
        self.bad = self.bad or len(body) < 32
        return self

    def fit(self, target):
        """150 bp records, the last of them with a Z tag of the fitting length, so that the last one ends exactly on `target`"""
        left = target - self.pos
        assert left == 0 or left == S or left >= S + 4, (self.pos, target)
        n = max(0, (left - S - 4) // S)
        self.add(CORE, n)
        left -= n * S
        if left:
            self.add(CORE + zfit(left - S))
        assert self.pos == target
        return self

    def decoy(self, at, payload):
        """a carrier whose payload begins exactly on `at` (its own start lies HEAD bytes before)"""
        return self.fit(at - HEAD).add(carrier(payload))

    def cut(self, raw):
        """the first bytes of a record that does not end inside the stream"""
        self.parts.append(bytes(raw))
        self.pos += len(raw)
        self.closed = True
        return self

    def case(self, name, start=None, cut_at=None):
        s = b"".join(self.parts)
        assert len(s) == self.pos
        off, ln, consumed, bad = self.off, self.len, self.consumed, self.bad
        if cut_at is not None:                         # the stream cut at `cut_at`: the whole records in front of it
            k = bisect.bisect_right([o + l for o, l in zip(off, ln)], cut_at)
            s, off, ln = s[:cut_at], off[:k], ln[:k]
            consumed = off[-1] + ln[-1] if k else self.start
            bad = any(l < 32 for l in ln)
        st = self.start if start is None else start
        if st >= len(s):
            off, ln, consumed, bad = [], [], st, False
        w = Want(1, None, None, None) if bad else Want(0, np.asarray(off, dtype=np.uint64), np.asarray(ln, dtype=np.uint32), consumed)
        return Case(name, s, st, w)


def chain(stream, start):
    """The sequential walk (BoundaryFinder::find_boundaries): (body offsets, lengths, consumed, a whole record with block_size < 32)."""
    off, ln, p, bad = [], [], start, False
    while p + 4 <= len(stream):
        bs = int.from_bytes(stream[p:p + 4], "little")
        if p + 4 + bs > len(stream):
            break
        off.append(p + 4); ln.append(bs)
        bad = bad or bs < 32
        p += 4 + bs
    return np.asarray(off, dtype=np.uint64), np.asarray(ln, dtype=np.uint32), p, bad


# ---- k_bound_guess, restated (conditions on the inputs only) ---------------------------------------------------------------------------------------------------

def _u32(s, p):
    return int.from_bytes(s[p:p + 4], "little")


def _i32(s, p):
    return int.from_bytes(s[p:p + 4], "little", signed=True)


def looks_like_record(s, p):
    n = len(s)
    if p + 36 > n:
        return False
    bs = _u32(s, p)
    if bs < 32 or bs > 1 << 28:
        return False
    if min(_i32(s, p + 4), _i32(s, p + 8), _i32(s, p + 24), _i32(s, p + 28)) < -1:
        return False
    l_name, n_cig, l_seq = s[p + 12], _u32(s, p + 16) & 0xFFFF, _u32(s, p + 20)
    if l_name == 0 or l_seq > 1 << 28 or 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
        return False
    name = p + 36
    nul = name + l_name - 1
    if nul >= n:
        return True
    if s[nul] != 0 or any(ch < 0x21 or ch > 0x7E for ch in s[name:nul]):
        return False
    cig = nul + 1
    if n_cig and cig + 4 * n_cig <= n and n_cig <= 256:
        q_len = 0
        for i in range(n_cig):
            op = _u32(s, cig + 4 * i)
            if op & 15 > 8:
                return False
            if op & 15 in (0, 1, 4, 7, 8):
                q_len += op >> 4
        if l_seq and q_len != l_seq:
            return False
    return True


def guess(s, start, g):
    """what k_bound_guess proposes for segment g"""
    n = len(s)
    lo, hi = g * SEG, min(g * SEG + SEG, n)
    if g == start // SEG:
        return start
    if lo < start:
        return NONE
    for p in range(lo, hi):
        if p + 36 > n:
            break
        if s[p + 3] > 0x10 or not looks_like_record(s, p):          # (block_size <= 1 << 28: its top byte first, for speed)
            continue
        q = p + 4 + _u32(s, p)
        ok = q <= n
        for _ in range(2):
            if not (ok and q + 36 <= n):
                break
            ok = looks_like_record(s, q)
            if ok:
                q += 4 + _u32(s, q)
                ok = q <= n
        if ok:
            return p
    return NONE


def misguessed(case):
    """the segments whose guess is not the sequential walk's first record start of that segment (what the first check has to correct)"""
    off, _, _, _ = chain(case.stream, case.start)
    starts = [int(o) - 4 for o in off]
    out = []
    for g in range(case.start // SEG + 1, case.n_seg):           # (the segment of `start` is given, those before it hold the header)
        k = bisect.bisect_left(starts, g * SEG)
        true = starts[k] if k < len(starts) and starts[k] < g * SEG + SEG else NONE
        if guess(case.stream, case.start, g) != true:
            out.append(g)
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------------

def group_a():
    out = []
    # A1: a record ends exactly on k * SEG — as the stream's end, in front of 200 more records, in front of the first 1 .. 4 bytes of the next record
    for k in (1, 2, 3):
        out.append(Stream().fit(k * SEG).case(f"A1/ends_on_{k}seg"))
        out.append(Stream().fit(k * SEG).add(CORE, 200).case(f"A1/ends_on_{k}seg_then_200"))
        for b in (1, 2, 3, 4):
            out.append(Stream().fit(k * SEG).cut(link()[:b]).case(f"A1/ends_on_{k}seg_then_{b}_bytes"))
            assert out[-1].want.consumed == k * SEG
    # A2: a true record starts d bytes before a segment edge: the prefix straddles it (d < 4), the fixed part does (d = 35, 36)
    for i, d in enumerate((1, 2, 3, 4, 35, 36)):
        k = 1 + i % 3
        out.append(Stream().fit(k * SEG - d).add(CORE, 150).case(f"A2/starts_{d}_before_{k}seg"))
    # A3: short streams
    two = Stream().add(MINI, 2)
    for n in (0, 1, 2, 3) + tuple(range(4, 41, 3)):
        out.append(two.case(f"A3/len_{n}", cut_at=n))
    out.append(Stream().add(MINI).case("A3/one_minimal_record"))
    out.append(Stream().add(CORE).case("A3/one_record"))
    # A4: start offsets
    s = Stream().add(CORE, 70)
    out.append(s.case("A4/start_eq_len", start=s.pos))
    out.append(s.case("A4/start_gt_len", start=s.pos + 5))
    out.append(Stream(bytes(40000)).add(CORE, 300).case("A4/start_40000_behind_zeros"))
    out.append(Stream(random.Random(3).randbytes(40000)).add(CORE, 300).case("A4/start_40000_behind_random_bytes"))
    for d in (1, 2, 3):
        out.append(Stream(bytes(2 * SEG - d)).add(CORE, 130).case(f"A4/start_{d}_before_2seg"))
    # A5: segments without a record start
    out.append(Stream().add(CORE, 100).add(LONG).add(CORE, 100).case("A5/long_record_in_the_middle"))
    out.append(Stream().add(LONG).add(CORE, 100).case("A5/long_record_first"))
    out.append(Stream().add(CORE, 100).add(LONG).case("A5/long_record_last"))
    s = Stream().add(CORE, 100)
    out.append(s.cut(struct.pack("<I", len(LONG)) + LONG[:4 * SEG]).case("A5/cut_inside_a_long_record"))
    assert out[-1].want.consumed == 100 * S and out[-1].n_seg - out[-1].want.consumed // SEG >= 4
    return out


B1_SEGMENTS = 70


def b1():
    """A carrier across every segment edge: the fake chain begins on the edge or a few bytes behind it, the segment's first true record behind the carrier."""
    s = Stream()
    for g in range(1, B1_SEGMENTS + 1):
        s.decoy(g * SEG + (0, 1, 2, 3, 5, 17)[g % 6], link() * 3)
    return s.add(CORE, 20).case("B1/fake_chain_before_the_first_true_record")


def _b2(extra=None):
    s = Stream().add(CORE, 90).add(carrier(link() * 600))
    if extra is not None:                      # B6: a true record with a block_size below 32, second in its segment, well behind the carrier
        s.fit(8 * SEG).add(CORE).add(bytes(extra))
    return s.add(CORE, 150)


def b7():
    """> 256 segments: a far jump out of segment 250 that ends in 263 (it wipes 251 .. 262, across the thread blocks' edge), B1-style decoys in 255, 256, 257."""
    s = Stream().fit(250 * SEG - HEAD)
    jump = 263 * SEG + 100 - (250 * SEG + 2 * F + 4)
    s.add(carrier(link() * 2 + link(jump)))
    for g in (255, 256, 257):
        s.decoy(g * SEG + g % 3, link() * 3)
    return s.fit(280 * SEG + 1000).case("B7/far_jump_and_decoys_across_the_block_edge")


def group_b(which="all"):
    out = []
    if which in ("all", "rest"):
        out.append(b1())
        # B2: 600 fake records in one carrier (segments with no true start, each with a guess), whole and cut inside the carrier
        s = _b2()
        out.append(s.case("B2/600_fake_records"))
        out.append(s.case("B2/600_fake_records_cut_inside_the_carrier", cut_at=90 * S + HEAD + 400 * F + 50))
        assert len(out[-1].want.off) == 90 and out[-1].want.consumed == 90 * S
        # B3: the third link jumps 200 000 bytes: the fake walk ends about 12 true segments later
        out.append(Stream().decoy(10 * SEG, link() * 2 + link(200000)).fit(30 * SEG + 700).case("B3/far_jump"))
        # B4: the fourth link points past the end: the fake walk is terminal
        out.append(Stream().decoy(11 * SEG, link() * 3 + link(1 << 27)).fit(23 * SEG - 900).case("B4/terminal_decoy"))
        assert out[-1].n_seg == 23
        # B5: the fourth link has block_size 8: the discarded walk saw a malformed record, the stream holds none
        out.append(Stream().decoy(3 * SEG, link() * 3 + BAD_LINK + link() * 2).add(CORE, 100).case("B5/bad_link_in_a_fake_chain"))
        assert out[-1].want.rc == 0
        # B6: a true record with block_size 20 / 31, behind the carrier of B2 and without any decoy (there the guess of the bad record's segment refuses the
        # true first record, whose successor does not look like one, and proposes the record behind the bad one: a repair all the same)
        for bs in (20, 31):
            out.append(_b2(bs).case(f"B6/true_record_of_block_size_{bs}"))
            out.append(Stream().fit(3 * SEG).add(CORE).add(bytes(bs)).add(CORE, 150).case(f"B6/true_record_of_block_size_{bs}_no_decoy"))
            assert out[-1].want.rc == out[-2].want.rc == 1
        # B8: a carrier over a whole segment; the fake chain begins near that segment's end and ends, with the carrier, on the next true record
        at = 5 * SEG - 2 * F - 40
        s = Stream().fit(4 * SEG - 300).add(carrier(bytes(at - (4 * SEG - 300 + HEAD)) + link() * 3)).add(CORE, 100)
        assert s.off[-100] - 4 == at + 3 * F and at // SEG == 4 and (at + 3 * F) // SEG == 5
        out.append(s.case("B8/fake_walk_ends_on_a_true_record"))
    if which in ("all", "B7"):
        out.append(b7())
    return out


def all_cases():
    return group_a() + group_b()


def check_case_set(cases):
    """Before any product code: the builder's books equal the sequential walk; the decoys sit where the case says."""
    for c in cases:
        off, ln, consumed, bad = chain(c.stream, c.start)
        if c.want.rc:
            assert bad, c.name
        else:
            assert not bad and np.array_equal(off, c.want.off) and np.array_equal(ln, c.want.len) and consumed == c.want.consumed, c.name
        wrong = misguessed(c)
        assert len(c.stream) <= 5 << 20
        if c.group == "A":
            assert not wrong, (c.name, wrong)
        else:
            assert wrong, c.name
        if c.name.startswith("B1"):
            assert len(wrong) >= 64, len(wrong)
        if c.name.startswith("B7"):
            assert c.n_seg > BLOCK + 8 and len(c.stream) > 4.3 * (1 << 20) and {250, 255, 256, 257} <= set(wrong), wrong


# ---- the runner ------------------------------------------------------------------------------------------------------------------------------------------------

POISON = 0xA5


class HostMem:
    """tests/apiemu: device memory is host memory.  A stream is placed flush against a PROT_NONE page, no pad behind it: a read past `len` ends the process."""

    def __init__(self, cap):
        import mmap
        libc = C.CDLL(None, use_errno=True)
        libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
        page = mmap.PAGESIZE
        self.size = (cap + page - 1) // page * page
        self.m = mmap.mmap(-1, self.size + page)
        self.base = C.addressof(C.c_char.from_buffer(self.m))
        assert libc.mprotect(self.base + self.size, page, 0) == 0, C.get_errno()

    def put(self, stream):
        at = self.size - len(stream)
        self.m[at:self.size] = stream
        return self.base + at

    def arrays(self, n):
        self.off, self.len = np.full(n, POISON * 0x0101010101010101, dtype=np.uint64), np.full(n, POISON * 0x01010101, dtype=np.uint32)
        return self.off.ctypes.data, self.len.ctypes.data

    def fetch(self):
        return self.off, self.len


class DeviceMem:
    """tensors in HBM; the stream's tensor is exactly len(stream) bytes long"""

    def __init__(self, cap):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", torch.cuda.current_device())

    def put(self, stream):
        t = self.torch
        self.s = t.frombuffer(bytearray(stream), dtype=t.uint8).to(self.dev) if stream else t.empty(0, dtype=t.uint8, device=self.dev)
        assert self.s.numel() == len(stream)
        t.cuda.synchronize()
        return self.s.data_ptr()

    def arrays(self, n):
        t = self.torch
        self.off = t.from_numpy(np.full(n, POISON * 0x0101010101010101, dtype=np.uint64).view(np.int64)).to(self.dev)
        self.len = t.from_numpy(np.full(n, POISON * 0x01010101, dtype=np.uint32).view(np.int32)).to(self.dev)
        t.cuda.synchronize()
        return self.off.data_ptr(), self.len.data_ptr()

    def fetch(self):
        self.torch.cuda.synchronize()
        return self.off.cpu().numpy().view(np.uint64), self.len.cpu().numpy().view(np.uint32)


class Runner:
    def __init__(self, mode):
        from fgumi_amd import VanillaUmiConsensusCaller
        from fgumi_amd._lib import lib
        assert mode in ("device", "host")
        self.mode, self.lib = mode, lib
        self.c = VanillaUmiConsensusCaller("", "A")
        self.mem = (DeviceMem if mode == "device" else HostMem)(5 << 20)
        self.seen = {}

    def close(self):
        self.c.close()

    def call(self, case, ptr, off_ptr, len_ptr, cap):
        n, used = C.c_uint64(12345), C.c_uint64(12345)
        rc = self.lib.fgx_record_boundaries_device(self.c._h, ptr, len(case.stream), case.start, off_ptr, len_ptr, cap, C.byref(n), C.byref(used))
        rounds = int(self.lib.fgx_debug_last_boundary_rounds(self.c._h))
        self.check_rounds(case, rounds)
        return rc, n.value, used.value

    def check_rounds(self, case, rounds):
        self.seen.setdefault(case.name, []).append(rounds)
        assert rounds <= case.n_seg + 1, (case.name, rounds)
        if case.group == "A":
            assert rounds == 0, (case.name, rounds)
        else:
            assert rounds >= 1, (case.name, rounds)
            if self.mode == "host" and case.name[:2] in ("B3", "B4"):      # (the serial order of the host build makes this certain; on the GPU the true
                assert rounds >= 3, (case.name, rounds)                     # predecessor may discard the fake segment before its thread looks: any count from 1)

    def untouched(self, case, n):
        off, ln = self.mem.fetch()
        assert (off[n:] == POISON * 0x0101010101010101).all() and (ln[n:] == POISON * 0x01010101).all(), f"{case.name}: written past element {n}"
        return off[:n], ln[:n]

    def run(self, case):
        """count (cap = 0, null arrays), then fill with cap == n_rec: offsets, lengths, consumed and the return code, exactly"""
        w = case.want
        ptr = self.mem.put(case.stream)
        rc, n, used = self.call(case, ptr, None, None, 0)
        if w.rc:
            assert rc == 1 and b"block_size" in self.lib.fgx_last_error(self.c._h), (case.name, rc)
            op, lp = self.mem.arrays(SPARE)
            assert self.call(case, ptr, op, lp, SPARE)[0] == 1
            self.untouched(case, 0)
            return
        assert (rc, n, used) == (0, len(w.off), w.consumed), (case.name, rc, n, used, len(w.off), w.consumed)
        op, lp = self.mem.arrays(n + SPARE)
        assert self.call(case, ptr, op, lp, n) == (0, n, w.consumed), case.name
        off, ln = self.untouched(case, n)
        if not (np.array_equal(off, w.off) and np.array_equal(ln, w.len)):
            i = next(k for k in range(n) if off[k] != w.off[k] or ln[k] != w.len[k])
            raise AssertionError(f"{case.name}: record {i} of {n}: ({off[i]}, {ln[i]}) instead of ({w.off[i]}, {w.len[i]})")

    def contract(self, case):
        w, n = case.want, len(case.want.off)
        assert n > 10
        ptr = self.mem.put(case.stream)
        for cap in (n, n + 1, n + 37):                   # enough room: everything past n_rec untouched
            op, lp = self.mem.arrays(cap + SPARE)
            assert self.call(case, ptr, op, lp, cap) == (0, n, w.consumed), (case.name, cap)
            off, ln = self.untouched(case, n)
            assert np.array_equal(off, w.off) and np.array_equal(ln, w.len), (case.name, cap)
        for cap in (1, n // 2, n - 1):                   # too small: 2, the right count, nothing written
            op, lp = self.mem.arrays(cap + SPARE)
            rc, got, _ = self.call(case, ptr, op, lp, cap)
            assert (rc, got) == (2, n), (case.name, cap, rc, got)
            self.untouched(case, 0)
        assert self.call(case, ptr, None, None, 0) == (0, n, w.consumed), case.name


def check(which, mode):
    """`which`: "A", "B" (B1 .. B6 and B8), "B7", "CD" (the contract, then every case on one caller in a shuffled order), or "all"."""
    cases = {"A": group_a, "B": lambda: group_b("rest"), "B7": lambda: group_b("B7")}.get(which, all_cases)()
    check_case_set(cases)
    r = Runner(mode)
    try:
        if which in ("A", "B", "B7", "all"):
            for c in cases:
                r.run(c)
        if which in ("CD", "all"):
            by = {c.name: c for c in cases}
            for name in ("A1/ends_on_2seg_then_200", "B1/fake_chain_before_the_first_true_record"):
                r.contract(by[name])
            largest = max((c for c in cases if c.group == "B"), key=lambda c: len(c.stream))
            small = [c for c in cases if c.name.startswith("A3")]
            rest = [c for c in cases if c is not largest and c not in small]
            for seed in (41, 42):                        # the longest table directly in front of the shortest ones, somewhere in the shuffled rest
                rng = random.Random(seed)
                rng.shuffle(rest); rng.shuffle(small)
                at = rng.randrange(len(rest))
                for c in rest[:at] + [largest] + small + rest[at:]:
                    r.run(c)
    finally:
        r.close()
    print(f"boundaries {which} on the {mode} build: repair rounds", {k: v for k, v in r.seen.items() if k[0] == "B"})
