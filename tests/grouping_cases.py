"""Inputs of the MI-grouping tests of grouping.hip (check_grouping_kernels_on_hostile_streams in tests/test_apiemu.py on the CPU, tests/test_gpu_grouping.py on
the GPU) and the one runner both use (TEST INFRASTRUCTURE).

Every crafted record carries its expected answer, written by hand next to it: `None` where the reference skips the record, else the pair (MI value after
the transform, cell value) its group key is made of.  The rules, all of the reference:
  * crates/fgumi-raw-bam/src/tags.rs:13-48    find_tag_position / find_string_tag: the walk goes entry by entry (fields.rs:309-330 tag_value_size), the FIRST
                                              entry with the tag's two bytes decides, a type other than `Z` or a value without NUL gives None, an entry whose
                                              size cannot be told ends the walk; fields.rs:498-503 aux_data_slice: no aux block where its offset lies past the record
  * src/lib/mi_group.rs:227-242               get_mi_tag: no MI value -> the record is skipped; key = MI (transformed), and with a cell tag configured
                                              MI + '\t' + cell value, the cell value left out where find_string_tag gives None
  * src/lib/mi_group.rs:276-310               add_records: consecutive KEPT records with an equal key form a group (dropped records in between do not split it)
  * src/lib/commands/common.rs:384-397        consensus_pregroup_keep_flags: 0x100 / 0x800 always dropped, 0x4 dropped unless --allow-unmapped
  * crates/fgumi-umi/src/lib.rs:370-375       extract_mi_base: cut at the LAST '/', unless it leads the value
`expected` turns the per-record answers into kept indices and group sizes by those rules alone: it never parses a record.  `run_case` first holds the
oracle to that answer, then both entries of the product to the oracle, so two implementations that agree with each other but not with the reference fail."""
import ctypes as C
import dataclasses
import random
import struct

import numpy as np

import bamutil
import orc
from fgumi_amd import GroupedReads

OPTION_SETS = (dict(cell_tag="CB"), dict(cell_tag=None), dict(cell_tag="CB", strip_strand_suffix=True),       # (those of test_device_grouping_matches_oracle)
               dict(cell_tag=None, strip_strand_suffix=True, allow_unmapped=True))


# ---- records ---------------------------------------------------------------------------------------------------------------------------------------------

def R(aux=b"", flag=0, name="q"):
    """A 4-base record (44 bytes + aux; 40 + aux where 0x4 leaves it without a CIGAR) whose aux block is exactly `aux`."""
    return bamutil.make_record(name, "ACGT", [30] * 4, flag=flag, tags=[("", "raw", bytes(aux))])


def Z(tag, val):
    return tag.encode() + b"Z" + (val.encode() if isinstance(val, str) else bytes(val)) + b"\0"


def H(tag, val):
    return tag.encode() + b"H" + val.encode() + b"\0"


def N(tag, ty, val):
    """A fixed-size entry; `val` a number, or the payload's raw bytes."""
    fmt = {"A": "<c", "c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}[ty]
    raw = val if isinstance(val, bytes) else struct.pack(fmt, val)
    assert len(raw) == struct.calcsize(fmt)
    return tag.encode() + ty.encode() + raw


def B(tag, sub, payload=b"", count=None):
    """A `B` array of element type `sub` over the raw `payload`; `count` overrides the stored element count (malformed arrays)."""
    es = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}.get(sub, 1)
    n = len(payload) // es if count is None else count
    return tag.encode() + b"B" + sub.encode() + struct.pack("<I", n) + bytes(payload)


def stream(recs):
    """The records as one block_size-prefixed stream; the blob ends with the last record's last byte."""
    g = GroupedReads.from_groups([list(recs)])
    return g.blob, g.rec_off, g.rec_len


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Case:
    name: str
    kw: dict                   # group_records keywords (cell_tag as str or None)
    items: list                # [(record bytes, None | (mi, cell))]
    at_blob_end: bool = False  # the case is about its LAST record ending the blob

    def key(self, e):
        """mi_group.rs:230-241: the MI value, then '\\t' and the cell value where a cell tag is configured."""
        if e is None:
            return None
        mi, cb = (x.encode() if isinstance(x, str) else bytes(x) for x in e)
        return mi + b"\t" + cb if self.kw.get("cell_tag") else mi


def expected(case):
    """(kept record indices, group sizes) from the hand-written answers: records answered None are skipped, runs of equal keys among the rest are the groups."""
    kept, sizes, last = [], [], None
    for i, (_, e) in enumerate(case.items):
        k = case.key(e)
        if k is None:
            continue
        kept.append(i)
        if sizes and k == last:
            sizes[-1] += 1
        else:
            sizes.append(1)
        last = k
    return kept, sizes


def _case(name, kw, items, **more):
    return Case(name, dict(kw), list(items), **more)


CELL, NO_CELL = dict(cell_tag="CB"), dict(cell_tag=None)
MI1 = Z("MI", "1")
GOOD = (R(MI1), ("1", ""))

# one entry of every aux type (payloads that spell "MIZ..": a walk that scans bytes, not entries, finds a tag inside them)
LEADS = [("A", N("XA", "A", b"M")), ("c", N("Xc", "c", -5)), ("C", N("XC", "C", 200)), ("s", N("Xs", "s", -300)), ("S", N("XS", "S", 40000)),
         ("i", N("Xi", "i", b"MIZ\0")), ("I", N("XI", "I", 3_000_000_000)), ("f", N("Xf", "f", 0.25)), ("Z", Z("XZ", "MIZ7")), ("Z0", Z("XZ", "")),
         ("H", H("XH", "1AE301")), ("H0", H("XH", "")),
         ("Bc", B("Bc", "c", b"\x01\x02\x03")), ("BC", B("BC", "C", b"MIZ9\0")), ("Bs", B("Bs", "s", b"\0" * 6)), ("BS", B("BS", "S", b"MIZ9\0\0")),
         ("Bi", B("Bi", "i", b"\xff" * 12)), ("BI", B("BI", "I", b"MIZ\0" * 3)), ("Bf", B("Bf", "f", struct.pack("<3f", 1.5, -2.0, 0.0))),
         ("BA", B("BA", "A", b"MI")),                                            # (fields.rs:269-280: the size table knows 'A', so an array of it walks)
         ("B_count0", B("B0", "C")), ("Bi_count0", B("B0", "i")),
         ("Bs_1000", B("Bk", "s", bytes(range(250)) * 8)), ("BC_1001", B("Bk", "C", (b"MIZ9\0" * 201)[:1001]))]


def tag_walk_cases():
    """Case set A: MI (and the cell tag) behind, between and instead of other entries."""
    out = []
    for name, lead in LEADS + [("chain", b"".join(e for _, e in LEADS))]:
        for kw in (CELL, NO_CELL):
            out.append(_case(f"behind_{name}", kw, [(R(lead + Z("MI", "5")), ("5", "")), (R(Z("MI", "5")), ("5", "")), (R(lead + Z("MI", "6")), ("6", "")),
                                                     (R(lead + Z("CB", "x") + lead + Z("MI", "6")), ("6", "x")), (R(Z("MI", "6") + lead + Z("CB", "x")), ("6", "x"))]))
    # MI at every offset mod 8 from the aux start (Z and H values of 0 .. 15 bytes in front: offsets 4 .. 19), one key throughout
    items = [(R(Z("XZ", "p" * v) + Z("MI", "7") + Z("CB", "c")), ("7", "c")) for v in range(16)]
    items += [(R(H("XH", "AB" * v) + Z("MI", "8") + Z("CB", "c")), ("8", "c")) for v in range(8)]
    assert {(4 + v) % 8 for v in range(16)} == set(range(8))
    out += [_case("mi_at_every_offset_mod_8", kw, items) for kw in (CELL, NO_CELL)]
    # a type other than Z, and duplicates: the first occurrence decides (tags.rs:23-25, :42-44)
    mi_i, cb_i = N("MI", "i", 5), N("CB", "i", 5)
    items = [(R(mi_i), None), (R(N("MI", "A", b"1")), None), (R(H("MI", "1A")), None), (R(B("MI", "C", b"\x01\x02")), None),
             (R(mi_i + Z("MI", "1")), None),                                     # MI:i then MI:Z: the first one is not a string
             (R(Z("MI", "a") + Z("MI", "b")), ("a", "")), (R(Z("MI", "a")), ("a", "")), (R(Z("MI", "b") + Z("MI", "a")), ("b", "")),
             (R(MI1 + cb_i), ("1", "")), (R(MI1), ("1", "")), (R(MI1 + Z("CB", "")), ("1", "")), (R(MI1 + N("CB", "A", b"x")), ("1", "")),
             (R(MI1 + H("CB", "1A")), ("1", "")), (R(MI1 + B("CB", "C", b"x")), ("1", "")),
             (R(MI1 + cb_i + Z("CB", "x")), ("1", "")),                          # CB:i then CB:Z: no cell value
             (R(MI1 + Z("CB", "x")), ("1", "x")), (R(Z("CB", "x") + MI1), ("1", "x")), (R(MI1 + Z("CB", "x") + Z("CB", "y")), ("1", "x")),
             (R(Z("CB", "y") + MI1 + Z("CB", "x")), ("1", "y")), (R(Z("CB", "x") + mi_i), None), (R(Z("CB", "y") + MI1), ("1", "y"))]
    out += [_case("wrong_type_and_duplicates", kw, items) for kw in (CELL, NO_CELL)]
    out += malformed_cases() + blob_end_cases() + key_cases() + strand_suffix_cases() + tab_cases() + flag_cases()
    return out


def _l_seq_wraps():
    """l_seq = 0xFFFFFFFF: the aux offset is 32 + l_name + 2^31 + 2^32 - 1 (fields.rs:479-503, in usize) — past the record, so no aux block.  In 32-bit
    arithmetic it wraps to the name's NUL, from where the bytes below walk as `\\0X:A:v MI:Z:1`."""
    r = bytearray(R(b""))
    r[16:20] = b"\xff\xff\xff\xff"
    return bytes(r[:34]) + b"XAv" + MI1


MALFORMED = [   # (name, aux block or whole record, answer with a cell tag configured)
    ("unknown_type", b"XX?ab" + MI1, None), ("unknown_type_lower_z", b"XXzab\0" + MI1, None),
    ("b_unknown_subtype", B("XB", "?", b"\0") + MI1, None), ("b_subtype_z", B("XB", "Z", b"a\0") + MI1, None),
    ("b_count_past_the_end", B("XB", "C", b"ab", count=1000) + MI1, None),
    ("b_count_times_size_is_2_to_the_32", B("XB", "I", count=0x40000000) + MI1, None),       # usize: far past the record; wrapped to 32 bits it lands on MI
    ("b_count_all_ones", B("XB", "I", count=0xFFFFFFFF) + MI1, None),
    ("b_header_cut", b"XBBC\x01", None),
    ("z_without_nul", b"XZZabc" + b"MIZ1", None), ("h_without_nul", b"XHH1A" + b"MIZ1", None),
    ("mi_without_nul", b"MIZ1", None), ("mi_without_nul_9_bytes", b"MIZ" + b"1" * 9, None),   # (the next record's block_size holds NULs: the walk ends with the record)
    ("stray_1", b"M", None), ("stray_2", b"MI", None), ("stray_3", b"MIZ", None),
    ("fixed_value_cut", b"Xii\x01\x02", None), ("fixed_value_cut_then_mi", N("XA", "A", b"x") + b"Xii\x01\x02", None),
    ("no_aux_block", b"", None),
    ("junk_behind_mi", MI1 + b"XX?junk", ("1", "")), ("junk_between_mi_and_cb", MI1 + b"XX?" + Z("CB", "x"), ("1", "")),   # MI is found first; the cell walk ends at the junk
    ("cb_without_nul_behind_mi", MI1 + b"CBZx", ("1", "")), ("b_header_cut_behind_mi", MI1 + b"XBBC\x01", ("1", "")),
    ("three_strays_behind_mi", MI1 + b"CBZ", ("1", "")), ("fixed_value_cut_behind_mi", MI1 + b"XXC", ("1", "")),
    ("b_count0_ends_the_record", MI1 + B("XB", "C"), ("1", "")),
]


def malformed_cases():
    """good, malformed, good: the malformed record is skipped (or keyed as written) and the two good ones join across it."""
    out = [_case(f"malformed_{name}", kw, [GOOD, (R(aux), e), GOOD]) for name, aux, e in MALFORMED for kw in (CELL, NO_CELL)]
    good = R(MI1)
    whole = [("rec_len_0", b""), ("rec_len_31", good[:31]), ("cut_before_the_aux_block", good[:40]), ("l_seq_wraps_32_bits", _l_seq_wraps())]
    out += [_case(f"malformed_{name}", CELL, [GOOD, (rec, None), GOOD]) for name, rec in whole]
    return out


def blob_end_cases():
    """The same tails on the LAST record of the blob, blob_len = its end exactly (the byte-assembled header and count reads of find_z_tag_wide), and a
    well-formed MI whose NUL is the blob's last byte."""
    out = [_case(f"blob_end_{name}", kw, [GOOD, GOOD, (R(aux), e)], at_blob_end=True) for name, aux, e in MALFORMED for kw in (CELL, NO_CELL)]
    out += [_case("blob_end_mi_last", kw, [GOOD, (R(N("XA", "A", b"x") + MI1), ("1", ""))], at_blob_end=True) for kw in (CELL, NO_CELL)]
    out += [_case("blob_end_mi_last_17_bytes", CELL, [(R(Z("CB", "c") + Z("MI", "m" * 17)), ("m" * 17, "c"))] * 2, at_blob_end=True)]
    good = R(MI1)
    out += [_case(f"blob_end_{name}", CELL, [GOOD, (rec, None)], at_blob_end=True) for name, rec in (("rec_len_0", b""), ("rec_len_31", good[:31]))]
    return out


KEY_LENGTHS = list(range(18)) + [63, 64, 65, 300]


def _variants(base):
    """Values that differ from `base` in one place each."""
    n = len(base)
    v = [base + b"A"]                                                      # base is a proper prefix of it
    if n:
        v += [base[:-1] + b"#", b"#" + base[1:], base[:-1]]                # last byte, first byte, a proper prefix of base
    v += [base[:k] + b"#" + base[k + 1:] for k in (7, 8, 9) if k < n]
    assert all(x != base for x in v)
    return v


def key_cases():
    """Equal and almost-equal keys of every length around the 8-byte compare loop of k_group_bounds: base, base, base, variant, base, variant, ... — every
    neighbour differs in one place, and the three equal records have their tags at three different offsets."""
    out = []
    for n in KEY_LENGTHS:
        base = bytes(65 + (i * 7) % 26 for i in range(n))
        for part in ("mi", "cb"):
            def rec(v, shape=0):
                mi, cb = (Z("MI", v), Z("CB", "c")) if part == "mi" else (Z("MI", "1"), Z("CB", v))
                return R([mi + cb, Z("XZ", "pad") + mi + N("Xi", "i", 7) + cb, cb + mi][shape])

            def ans(v):
                return (v, "c") if part == "mi" else ("1", v)
            items = [(rec(base, s), ans(base)) for s in range(3)]
            for v in _variants(base):
                items += [(rec(v), ans(v)), (rec(base), ans(base))]
            if part == "cb" and n == 0:
                items += [(R(Z("MI", "1")), ("1", ""))]                   # an absent cell tag keys like an empty one
            out.append(_case(f"key_{part}_len_{n}", CELL, items))
            if part == "mi":
                out.append(_case(f"key_{part}_len_{n}", NO_CELL, items))
    return out


def strand_suffix_cases():
    vals = [("/", "/"), ("//", "/"), ("/A", "/A"), ("a/", "a"), ("a", "a"), ("a/B", "a"), ("a//", "a/"), ("a/b/A", "a/b"), ("a/b/B", "a/b"), ("a/b", "a"),
            ("abc", "abc"), ("x", "x"), ("x/A", "x"), ("", ""), ("/", "/")]                           # (value, extract_mi_base(value)), written out by hand
    out = []
    for cell in (CELL, NO_CELL):
        for cb in ("c", None):
            def rec(v):
                return R(Z("MI", v) + (Z("CB", cb) if cb is not None else b""))
            out.append(_case(f"strand_suffix_cut_cb_{cb}", dict(cell, strip_strand_suffix=True), [(rec(v), (base, cb or "")) for v, base in vals]))
            out.append(_case(f"strand_suffix_kept_cb_{cb}", cell, [(rec(v), (v, cb or "")) for v, _ in vals]))
    return out


def tab_cases():
    """mi_group.rs:230-241 builds ONE string MI + '\\t' + cell: "1\\tA" + "" and "1" + "A\\t" are both "1\\tA\\t"."""
    def rec(mi, cb):
        return (R(Z("MI", mi) + Z("CB", cb)), (mi, cb))
    return [_case("tab_same_concatenation", CELL, [rec("1\tA", ""), rec("1", "A\t"), rec("1\tA", "")]),                                  # one group of 3
            _case("tab_same_concatenation_long", CELL, [rec("M" * 20 + "\t" + "C" * 20, ""), rec("M" * 20, "C" * 20 + "\t"), rec("M" * 20 + "\t" + "C" * 20, "")]),
            _case("tab_same_total_other_bytes", CELL, [rec("1\tA", ""), rec("1", "A-"), rec("1\tA", ""), rec("1", "B\t"), rec("1\tA", ""), rec("1A", "\t"),
                                                        rec("1\tA", ""), rec("2", "A\t"), rec("", "\tA\t"), rec("1\tA", "")]),
            _case("tab_without_a_cell_tag", NO_CELL, [rec("1\tA", ""), rec("1", "A\t"), rec("1\tA", "")])]


def flag_cases():
    """common.rs:384-397, every combination of the three flags that decide, mixed with flags that do not."""
    out = []
    for allow in (False, True):
        items = []
        for drop in range(8):
            f = (0x100 if drop & 1 else 0) | (0x800 if drop & 2 else 0) | (0x4 if drop & 4 else 0)
            for other in (0, 0x1, 0x10, 0x1 | 0x40, 0x1 | 0x80, 0x1 | 0x10 | 0x40, 0x2 | 0x8 | 0x20 | 0x200 | 0x400):
                keep = not (f & 0x900) and (allow or not (f & 0x4))
                items.append((R(MI1, flag=f | other), ("1", "") if keep else None))
        out += [_case(f"flags_allow_unmapped_{int(allow)}", dict(kw, allow_unmapped=allow), items) for kw in (CELL, NO_CELL)]
    return out


# ---- case set B: generated streams -------------------------------------------------------------------------------------------------------------------------

SIZES = (1, 2, 255, 256, 257, 511, 513, 70000)
DROPS = ("none", "third", "ends", "run", "all_but_last", "all")
SHAPES = ("singletons", "one", "sized", "one_split_by_drops")
_HEADS = {}


def _small(flag, aux):
    """R(aux, flag) without re-encoding the fixed part (70 000-record streams)."""
    if flag not in _HEADS:
        _HEADS[flag] = R(b"", flag)
    return _HEADS[flag] + aux


def generated(n, drops, shape, seed):
    """(records, answers) of an n-record stream of ~60-byte records: group membership by `shape`, dropped records by `drops` (a dropped record keeps its
    group's MI where the drop is by flag, so a group's members sit on both sides of it)."""
    rng = random.Random(seed)
    gid, g = [], 0
    while len(gid) < n:
        k = {"singletons": 1, "one": n, "one_split_by_drops": n, "sized": rng.randint(1, 600)}[shape]
        gid += [g] * k
        g += 1
    gid = gid[:n]
    dropped = [False] * n
    if drops == "third":
        dropped = [rng.random() < 1 / 3 for _ in range(n)]
    elif drops == "ends":
        dropped[0] = dropped[-1] = True
    elif drops == "run":
        k = min(5000, max(1, n // 3))                       # 5 000 consecutive drops in the middle (a third of a short stream)
        a = (n - k) // 2
        dropped[a:a + k] = [True] * k
    elif drops == "all_but_last":
        dropped = [True] * (n - 1) + [False]
    elif drops == "all":
        dropped = [True] * n
    if shape == "one_split_by_drops" and drops == "none":
        dropped = [i % 3 == 1 for i in range(n)]
    recs, ans = [], []
    for i in range(n):
        mi, cb = f"{seed % 97}_{gid[i]}", "ACGT"[gid[i] % 4] * 4
        aux, flag = Z("MI", mi) + Z("CB", cb), rng.choice((0, 0, 0x1 | 0x40, 0x1 | 0x80 | 0x10))
        if dropped[i]:
            how = rng.choice(("0x100", "0x800", "0x4", "no_tag", "wrong_type"))
            if how == "no_tag":
                aux = Z("XM", mi) + Z("CB", cb)
            elif how == "wrong_type":
                aux = N("MI", "i", gid[i]) + Z("CB", cb) + Z("MI", mi)
            else:
                flag |= int(how, 16)
        recs.append(_small(flag, aux))
        ans.append(None if dropped[i] else (mi, cb))
    return recs, ans


def generated_case(n, drops, shape, seed, kw=CELL):
    recs, ans = generated(n, drops, shape, seed)
    return _case(f"generated_{n}_{drops}_{shape}_{seed}", kw, list(zip(recs, ans)))


def straddlers(grp_first, every=256):
    """How many groups hold kept records on both sides of a multiple of `every` in kept-record index."""
    g = np.asarray(grp_first, dtype=np.int64)
    return int(((g[1:] - 1) // every > g[:-1] // every).sum())


BIG = [("third", "sized", 11), ("none", "sized", 12), ("run", "singletons", 13), ("ends", "one_split_by_drops", 14), ("all_but_last", "one", 15), ("all", "sized", 16),
       ("none", "one", 17)]


# ---- the runner --------------------------------------------------------------------------------------------------------------------------------------------

class HostArrays:
    """The caller's two grouping entries over host arrays (tests/apiemu: device memory is host memory)."""

    def __init__(self, caller):
        self.c = caller

    def group_records(self, *a, **kw):
        return self.c.group_records(*a, **kw)

    def group_records_device(self, g, tag="MI", cell_tag="CB", strip_strand_suffix=False, allow_unmapped=False):
        from fgumi_amd._lib import GroupOptions, lib
        o = GroupOptions(tag.encode(), cell_tag.encode() if cell_tag else b"\0\0", int(strip_strand_suffix), int(allow_unmapped))
        n = g.n_rec
        blob = np.concatenate([g.blob, np.zeros(16, dtype=np.uint8)])
        off, ln, grp = np.zeros(max(1, n), dtype=np.uint64), np.zeros(max(1, n), dtype=np.uint32), np.zeros(n + 1, dtype=np.uint32)
        nk, ng = C.c_uint32(), C.c_uint32()
        rc = lib.fgx_group_records_device(self.c._h, C.byref(o), blob.ctypes.data, g.blob.size, g.rec_off.ctypes.data, g.rec_len.ctypes.data, n,
                                          off.ctypes.data, ln.ctypes.data, grp.ctypes.data, C.byref(nk), C.byref(ng))
        assert rc == 0, lib.fgx_last_error(self.c._h)
        return GroupedReads(g.blob, off[:nk.value], ln[:nk.value], grp[:ng.value + 1])


def _host(x, n, dtype):
    return np.asarray(x[:n].cpu().numpy() if hasattr(x, "cpu") else x[:n]).astype(dtype)


def run_stream(caller, blob, rec_off, rec_len, kw, mem="host", what="", want=None):
    """Both entries of `caller` (group_records on host buffers, group_records_device on the stream in device memory) against orc.group_records: rec_off,
    rec_len and grp_first, exactly.  `mem`: "host" (`caller` is a HostArrays) or "device" (tensors in HBM).  Returns the oracle's answer."""
    if want is None:
        want = orc.group_records(blob, rec_off, rec_len, **dict(kw, cell_tag=kw["cell_tag"].encode() if kw.get("cell_tag") else None))
    g = GroupedReads(blob, rec_off, rec_len, np.zeros(1, dtype=np.uint32))
    got = caller.group_records(blob, rec_off, rec_len, **kw)
    rd = caller.group_records_device(g.to_device() if mem == "device" else g, **kw)
    nk, ng = rd.n_rec, rd.n_grp
    for entry, (off, ln, grp) in (("fgx_group_records", (got.rec_off, got.rec_len, got.grp_first)),
                                  ("fgx_group_records_device", (_host(rd.rec_off, nk, np.uint64), _host(rd.rec_len, nk, np.uint32), _host(rd.grp_first, ng + 1, np.uint32)))):
        for name, a, b in (("rec_off", off, want[0]), ("rec_len", ln, want[1]), ("grp_first", grp, want[2])):
            if not np.array_equal(a, b):
                i = next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b)))
                raise AssertionError(f"{what} {kw}: {entry}: {name} differs from the oracle's at index {i} of {len(a)} / {len(b)}: {a[i:i + 4].tolist()} != {b[i:i + 4].tolist()}")
    return want


def run_case(caller, case, mem="host"):
    """The oracle against the case's hand-written answer, then the product against the oracle."""
    blob, off, ln = stream([r for r, _ in case.items])
    if case.at_blob_end:
        assert blob.size == int(off[-1]) + int(ln[-1])
    kept, sizes = expected(case)
    want = orc.group_records(blob, off, ln, **dict(case.kw, cell_tag=case.kw["cell_tag"].encode() if case.kw.get("cell_tag") else None))
    assert want[0].tolist() == [int(off[i]) for i in kept] and want[1].tolist() == [int(ln[i]) for i in kept], f"{case.name} {case.kw}: the oracle keeps other records than {kept}"
    assert np.diff(want[2].astype(np.int64)).tolist() == sizes and int(want[2][0]) == 0, f"{case.name} {case.kw}: the oracle's groups {np.diff(want[2].astype(np.int64)).tolist()}, expected {sizes}"
    run_stream(caller, blob, off, ln, case.kw, mem, case.name, want)
    return want


def _caller(mem):
    from fgumi_amd import VanillaUmiConsensusCaller
    c = VanillaUmiConsensusCaller("", "A")
    return c, (c if mem == "device" else HostArrays(c))


# ---- the checks (each one child process on the GPU; all of them in one on the host build) ---------------------------------------------------------------------

def check_tag_walk(mem="host"):
    c, entries = _caller(mem)
    cases = tag_walk_cases()
    for case in cases:
        run_case(entries, case, mem)
    c.close()
    print("tag walk:", len(cases), "cases,", sum(len(x.items) for x in cases), "records")


def check_scans(sizes=SIZES, mem="host"):
    """Case set B over `sizes`: every drop pattern on every group shape below 70 000 records, the combinations of BIG at 70 000."""
    c, entries = _caller(mem)
    for n in sizes:
        combos = BIG if n >= 70000 else [(d, s, 100 + 7 * i + j) for i, d in enumerate(DROPS) for j, s in enumerate(SHAPES)]
        for k, (drops, shape, seed) in enumerate(combos):
            case = generated_case(n, drops, shape, seed, dict(OPTION_SETS[k % 2], allow_unmapped=False))
            want = run_case(entries, case, mem)
            kept = len(want[0])
            if drops == "third" and n >= 255:          # conditions on the INPUT, on the oracle's answer: the stream really mixes kept and dropped records ...
                assert 0.2 * n <= kept <= 0.8 * n, (n, kept)
            if drops == "all":
                assert kept == 0 and want[2].tolist() == [0]
            if n >= 70000 and shape == "sized" and drops != "all":        # ... and its groups really cross the 256-thread blocks
                assert straddlers(want[2]) >= 100, (drops, straddlers(want[2]))
    c.close()


def check_scratch_reuse(mem="host"):
    """One caller over 70 000 records, then 3, none, 257, and 70 000 others: the scratch buffers of the larger call serve the smaller ones."""
    c, entries = _caller(mem)
    for rounds in range(2):
        for k, (n, seed) in enumerate(((70000, 21), (3, 22), (0, 23), (257, 24), (70000, 25))):
            kw = OPTION_SETS[(k + rounds) % 4]
            recs, _ = generated(n, "third", "sized", seed)
            if n == 3:
                recs = [R(Z("MI", "1/A"), flag=0x4), R(Z("MI", "1/B")), R(Z("MI", "1"))]
            want = run_stream(entries, *stream(recs), kw, mem, f"scratch reuse: call {k} of {n} records")
            assert n < 255 or 0.2 * n <= len(want[0]) <= 0.8 * n
    c.close()


def _with_drop_flags(g, every=7):
    """The flat stream of batch g with 0x100 set on every `every`-th record."""
    blob = np.array(g.blob, copy=True)
    blob[np.asarray(g.rec_off, dtype=np.int64)[::every] + 15] |= 0x01
    return blob


def layout_stream(name, duplex=False):
    import layouts
    from fgumi_amd import simulate_grouped_reads
    n = 100 if name == "huge_record" else 500 if duplex else 2000
    sim = dict(family_size=4, duplex=1) if duplex else dict(family_size=2, family_size_max=9)
    return layouts.apply(name, simulate_grouped_reads(n, seed=31, **sim), 5)


def check_layout(name, mem="host"):
    """Case set C: the layout's batch as a flat stream, with and without a drop flag on every seventh record, regrouped through both entries."""
    c, entries = _caller(mem)
    for duplex in (False, True):
        g = layout_stream(name, duplex)
        for kw in ((OPTION_SETS[2], dict(cell_tag=None, strip_strand_suffix=True)) if duplex else OPTION_SETS[:2]):
            want = run_stream(entries, g.blob, g.rec_off, g.rec_len, kw, mem, f"layout {name}")
            if kw["cell_tag"] is None or name != "duplicates":        # (`duplicates` gives some records of a family a CB of their own)
                assert np.array_equal(want[0], g.rec_off) and np.array_equal(want[2], g.grp_first), f"layout {name} {kw}: the oracle does not reproduce the generator's groups"
            want = run_stream(entries, _with_drop_flags(g), g.rec_off, g.rec_len, kw, mem, f"layout {name}, every seventh record dropped")
            assert len(want[0]) == g.n_rec - (g.n_rec + 6) // 7
    c.close()


def check_regrouped_layouts_feed_the_caller(mem="device"):
    """all_types and duplicates, every seventh record dropped: what fgx_group_records_device wrote (tensors in HBM; host arrays on the host build) handed
    to fgx_process_batch_device as it is gives the oracle's consensus over the oracle's grouping, byte for byte, counters included."""
    import fgx_opts
    from fgumi_amd._lib import Options, Output, lib
    o = fgx_opts.defaults(min_reads=1)
    c, entries = _caller(mem)
    for name in ("all_types", "duplicates"):
        g = layout_stream(name)
        blob = _with_drop_flags(g)
        off, ln, grp = orc.group_records(blob, g.rec_off, g.rec_len, cell_tag=None)
        assert len(off) == g.n_rec - (g.n_rec + 6) // 7 and len(grp) - 1 == g.n_grp
        flat = GroupedReads(blob, g.rec_off, g.rec_len, np.zeros(1, dtype=np.uint32))
        if mem == "device":
            from fgumi_amd._lib import hip_memcpy_d2h as fetch
            rg = entries.group_records_device(flat.to_device(), cell_tag=None)
            args = (rg.blob.data_ptr(), rg.blob_len, rg.rec_off.data_ptr(), rg.rec_len.data_ptr(), rg.n_rec, rg.grp_first.data_ptr(), rg.n_grp)
        else:
            def fetch(p, n):
                return C.string_at(p, n) if n else b""
            rg = entries.group_records_device(flat, cell_tag=None)
            padded = np.concatenate([blob, np.zeros(64, dtype=np.uint8)])
            args = (padded.ctypes.data, blob.size, rg.rec_off.ctypes.data, rg.rec_len.ctypes.data, rg.n_rec, rg.grp_first.ctypes.data, rg.n_grp)
        assert rg.n_rec == len(off) and rg.n_grp == len(grp) - 1
        h = lib.fgx_create(C.byref(Options.from_buffer_copy(bytes(o))))
        assert h, lib.fgx_global_error().decode()
        try:
            out, nd, dp = Output(), C.c_uint32(), C.c_void_p()
            rc = lib.fgx_process_batch_device(h, *args, C.byref(out), C.byref(nd), C.byref(dp))
            assert rc == 0, lib.fgx_last_error(h).decode()
            deferred = set(np.frombuffer(fetch(dp.value, 4 * nd.value), dtype=np.uint32).tolist()) if nd.value else set()
            assert len(deferred) < 0.1 * rg.n_grp, (name, len(deferred))        # (the device entry may hand groups back: then the oracle over the others)
            og = GroupedReads(blob, off, ln, grp)
            if deferred:
                og = GroupedReads.from_groups([og.records(i) for i in range(og.n_grp) if i not in deferred])
            want = orc.process(o, og.blob, og.rec_off, og.rec_len, og.grp_first)
            assert want["count"] > g.n_grp
            assert (fetch(out.data, int(out.data_len)) if out.data_len else b"") == want["data"], f"{name}: consensus over the device's grouping differs from the oracle's"
            assert int(out.count) == want["count"] and np.array_equal(np.array(list(out.stats), dtype=np.uint64)[:len(want["stats"])], want["stats"]), name
            print("fed the caller:", name, rg.n_rec, "records in", rg.n_grp, "groups,", len(deferred), "deferred,", int(out.count), "consensus records")
        finally:
            lib.fgx_destroy(h)
    c.close()


def check_everything_on_the_host_build():
    """Every case set on grouping.hip compiled for the host (tests/apiemu), host arrays standing in for the tensors in HBM."""
    import layouts
    check_tag_walk("host")
    check_scans(SIZES, "host")
    check_scratch_reuse("host")
    for name in layouts.LAYOUTS:
        check_layout(name, "host")
    check_regrouped_layouts_feed_the_caller("host")
