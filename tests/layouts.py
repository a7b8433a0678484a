"""Record-layout rewriter (TEST INFRASTRUCTURE, host Python): the same reads in the layouts real `fgumi group` output has, and in the
layouts that sit on the edges of the device kernels' windows and rules.

`simgen.h` writes one layout only: names of 20/21 characters, one `M` op, an aux block of RX, MI, MC (~31 bytes).  Each layout below
takes a `GroupedReads` and returns a new one holding the same reads (same bases, qualities, flags, positions, groups) with other names,
CIGARs or tags.  Every layout is a pure function of its seed; mates keep equal names.  Nothing here decides what a layout should
produce: the oracle does."""
import random
import struct

from fgumi_amd import GroupedReads

SIZES = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
OPS = "MIDNSHP=X"


class Rec:
    """One BAM record body split into its parts; the aux block as a list of (key, type, payload) with the payload's raw bytes."""

    def __init__(self, rec: bytes):
        (self.ref_id, self.pos, l_name, self.mapq, self.bin, n_cig, self.flag, l_seq, self.mate_ref, self.mate_pos,
         self.tlen) = struct.unpack_from("<iiBBHHHIiii", rec, 0)
        p = 32
        self.name = rec[p:p + l_name - 1]
        p += l_name
        self.cigar = list(struct.unpack_from(f"<{n_cig}I", rec, p))
        p += 4 * n_cig
        self.l_seq = l_seq
        self.seq = rec[p:p + (l_seq + 1) // 2]
        p += (l_seq + 1) // 2
        self.qual = rec[p:p + l_seq]
        p += l_seq
        self.tags = []
        while p + 3 <= len(rec):
            key, ty = rec[p:p + 2], chr(rec[p + 2])
            q = p + 3
            if ty in "ZH":
                e = rec.index(b"\0", q) + 1
            elif ty == "B":
                e = q + 5 + struct.unpack_from("<I", rec, q + 1)[0] * SIZES[chr(rec[q])]
            else:
                e = q + SIZES[ty]
            self.tags.append((key, ty, rec[q:e]))
            p = e
        assert p == len(rec), "trailing bytes in the aux block"

    def tag(self, key):
        for k, ty, v in self.tags:
            if k == key:
                return ty, v
        return None

    def cigar_str(self):
        return "".join(f"{c >> 4}{OPS[c & 15]}" for c in self.cigar)

    def encode(self) -> bytes:
        head = struct.pack("<iiBBHHHIiii", self.ref_id, self.pos, len(self.name) + 1, self.mapq, self.bin, len(self.cigar), self.flag, self.l_seq,
                           self.mate_ref, self.mate_pos, self.tlen)
        aux = b"".join(k + t.encode() + v for k, t, v in self.tags)
        return head + self.name + b"\0" + struct.pack(f"<{len(self.cigar)}I", *self.cigar) + self.seq + self.qual + aux


def aux_len(tags):
    return sum(3 + len(v) for _, _, v in tags)


def z(key, val):
    return (key.encode() if isinstance(key, str) else key, "Z", (val.encode() if isinstance(val, str) else val) + b"\0")


def num(key, ty, val):
    fmt = {"A": "<c", "c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}[ty]
    return (key.encode(), ty, struct.pack(fmt, val))


def barr(key, sub, n, rng):
    lo, hi = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1), "I": (0, 2 ** 32 - 1), "f": (0, 0)}[sub]
    vals = [rng.uniform(-1e3, 1e3) if sub == "f" else rng.randint(lo, hi) for _ in range(n)] if n <= 1000 else [0] * n
    return (key.encode(), "B", sub.encode() + struct.pack("<I", n) + struct.pack(f"<{n}{'bBhHiIf'['cCsSiIf'.index(sub)]}", *vals))


def filler(key, total):
    """A Z tag of exactly `total` bytes (key + type + value + NUL); total >= 4."""
    assert total >= 4, total
    return z(key, "F" * (total - 4))


def _rewrite(g: GroupedReads, fn, seed) -> GroupedReads:
    """fn(rng, group index, [Rec]) rewrites one group's records in place."""
    groups = []
    for gi in range(g.n_grp):
        recs = [Rec(r) for r in g.records(gi)]
        fn(random.Random(seed * 1_000_003 + gi), gi, recs)
        groups.append([r.encode() for r in recs])
    return GroupedReads.from_groups(groups)


def _renamer(make):
    """Names per group: records that shared a name before share one after (mates stay mates)."""
    def rename(rng, gi, recs):
        names = {}
        for r in recs:
            if r.name not in names:
                names[r.name] = make(rng, gi, len(names)).encode()
            r.name = names[r.name]
    return rename


def illumina_name(rng, gi, t):
    return f"A{rng.randint(10000, 99999)}:{rng.randint(100, 999)}:H{rng.randint(1000, 9999)}DSXY:{rng.randint(1, 4)}:{rng.randint(1101, 2678)}:{gi % 32768:05d}:{t:05d}"


def _core_tags(r):
    return [t for t in r.tags if t[0] in (b"MI", b"RX", b"MC", b"CB")]


def illumina(g, seed=0):
    """Names of ~38 characters; an aux block of 120 - 200 bytes: RG MQ AS XS NM MD ms (and QX / OX / BX) before and after MI / RX / MC, shuffled."""
    rename = _renamer(illumina_name)

    def fn(rng, gi, recs):
        rename(rng, gi, recs)
        for r in recs:
            rl = r.l_seq
            extra = [z("RG", "A"), num("MQ", "C", rng.choice([0, 37, 60])), num("AS", "C", rng.randint(100, 150)), num("XS", "C", rng.randint(0, 99)),
                     num("NM", "C", rng.randint(0, 4)), z("MD", f"{rl // 2}A{rl - rl // 2 - 1}"), num("ms", "s", rng.randint(1000, 6000))]
            if rng.random() < 0.6:
                extra += [z("QX", "".join(rng.choice("FF:,") for _ in range(8))), z("OX", "ACGTACGT"), z("BX", "ACGTACGT-TTGA")]
            tags = _core_tags(r) + extra
            rng.shuffle(tags)
            pad = rng.randint(120, 200) - aux_len(tags)
            if pad >= 4:
                tags.insert(rng.randint(0, len(tags)), filler("XP", pad))
            r.tags = tags
    return _rewrite(g, fn, seed)


def window_edges(g, seed=0):
    """Names of 42 / 43 / 44 characters (l_name + 4 = 47 / 48 / 49 around the split record kernel's 48-byte head window); aux blocks of exactly
    63 / 64 / 65 bytes (around its 64-byte tag window) with MI first or last, and blocks in which MI straddles byte 64."""
    def make(rng, gi, t):
        n = rng.choice([42, 43, 44])
        return (f"E{gi}_{t}_" + "x" * n)[:n]
    rename = _renamer(make)

    def fn(rng, gi, recs):
        rename(rng, gi, recs)
        for r in recs:
            mi = [t for t in r.tags if t[0] == b"MI"]
            rest = [t for t in _core_tags(r) if t[0] != b"MI"]
            shape = rng.choice(["first", "last", "straddle"])
            if shape == "straddle":   # MI's entry begins before byte 64 and ends after it; a 4-byte A tag behind it
                mi_len = aux_len(mi)
                lead = 64 + mi_len // 2 + 1 - mi_len - aux_len(rest)
                r.tags = rest + [filler("XF", lead)] + mi + [num("XA", "A", b"x")]
                assert aux_len(r.tags[:-2]) < 64 < aux_len(r.tags[:-1]), r.tags
            else:
                total = rng.choice([63, 64, 65])
                fill = filler("XF", total - aux_len(mi) - aux_len(rest))
                r.tags = mi + rest + [fill] if shape == "first" else rest + [fill] + mi
                assert aux_len(r.tags) == total
    return _rewrite(g, fn, seed)


def all_types(g, seed=0):
    """One tag of every value type before MI: A c C s S i I f H, and B arrays of every element type with 0, 1 or 1000 elements."""
    def fn(rng, gi, recs):
        for r in recs:
            lead = [num("Xa", "A", b"q"), num("Xc", "c", -5), num("XC", "C", 200), num("Xs", "s", -300), num("XS", "S", 40000), num("Xi", "i", -70000),
                    num("XI", "I", 3_000_000_000), num("Xf", "f", 0.25), (b"XH", "H", b"1AE301\0")]
            big = rng.choice("cCsSiIf")
            for sub in "cCsSiIf":
                lead.append(barr("B" + sub, sub, 1000 if sub == big and rng.random() < 0.5 else rng.choice([0, 1]), rng))
            rng.shuffle(lead)
            r.tags = lead + _core_tags(r) + [num("Xz", "i", 7)]
    return _rewrite(g, fn, seed)


def duplicates(g, seed=0):
    """A second, different MI / RX / MC / CB after the first one of each (SAM: the first occurrence is the tag)."""
    def fn(rng, gi, recs):
        for r in recs:
            tags = list(r.tags)
            if r.tag(b"CB") is None and rng.random() < 0.5:
                tags.append(z("CB", "CELLA"))
            dup = []
            for key, val in ((b"MI", f"{gi}9/B"), (b"RX", "TTTT-GGGG"), (b"MC", "3S20M"), (b"CB", "OTHER")):
                if any(t[0] == key for t in tags) and rng.random() < 0.8:
                    dup.append(z(key, val))
            rng.shuffle(dup)
            r.tags = tags + [num("XX", "C", 1)] + dup
    return _rewrite(g, fn, seed)


def long_values(g, seed=0, prefix_len=0, mi_totals=(253, 254, 0)):
    """MI values with prefix_len + 1 + len(MI) = 253 / 254 (`mi_totals`; 255 makes a consensus name longer than BAM allows: the reference
    refuses the batch) or short; RX and CB of 255 / 256 bytes; names of 100+ characters (fgumi-style `:UMI` suffixes)."""
    def make(rng, gi, t):
        return illumina_name(rng, gi, t) + ":" + "".join(rng.choice("ACGT") for _ in range(rng.randint(62, 90)))
    rename = _renamer(make)

    def fn(rng, gi, recs):
        rename(rng, gi, recs)
        mi_total = rng.choice(mi_totals)
        rx_len = rng.choice([255, 256, 0])
        cb_len = rng.choice([255, 256, 0])
        rx_val = "".join(rng.choice("ACGT") for _ in range(rx_len))
        for r in recs:
            tags = []
            for key, ty, v in r.tags:
                if key == b"MI" and mi_total:
                    old = v[:-1].decode()
                    base, sfx = (old[:-2], old[-2:]) if old[-2:] in ("/A", "/B") else (old, "")
                    n = mi_total - 1 - prefix_len - len(sfx)
                    tags.append(z("MI", (base + "u" * n)[:n] + sfx))
                elif key == b"RX" and rx_len:
                    tags.append(z("RX", rx_val))
                else:
                    tags.append((key, ty, v))
            if cb_len:
                tags = [t for t in tags if t[0] != b"CB"] + [z("CB", ("C" * cb_len))]
            r.tags = tags
    return _rewrite(g, fn, seed)


def huge_record(g, seed=0, every=1):
    """One record of every `every`-th group longer than 65 535 bytes: a B array of 66 000 bytes in front of MI."""
    def fn(rng, gi, recs):
        if gi % every == 0 and recs:
            r = recs[rng.randrange(len(recs))]
            r.tags = [barr("ZB", "C", 66000, rng)] + r.tags
    return _rewrite(g, fn, seed)


def clipped(g, seed=0):
    """Soft clips (n_cig 2 - 3: `5S145M`, `145M5S`, `3S140M7S`) on the reads of one-M-op records, and every MC tag rewritten to the mate's
    new CIGAR."""
    def fn(rng, gi, recs):
        new = {}
        for r in recs:
            if len(r.cigar) == 1 and (r.cigar[0] & 15) == 0 and r.l_seq >= 30 and rng.random() < 0.7:
                a = rng.choice([0, rng.randint(1, 8)])
                b = rng.choice([0, rng.randint(1, 8)]) if a else rng.randint(1, 8)
                r.cigar = ([a << 4 | 4] if a else []) + [(r.l_seq - a - b) << 4] + ([b << 4 | 4] if b else [])
            new[(r.name, r.flag & 0xC0)] = r.cigar_str()
        for r in recs:
            mate = new.get((r.name, (r.flag & 0xC0) ^ 0xC0))
            if mate is not None and r.tag(b"MC") is not None:
                r.tags = [z("MC", mate) if k == b"MC" else (k, t, v) for k, t, v in r.tags]
    return _rewrite(g, fn, seed)


LAYOUTS = {"illumina": illumina, "window_edges": window_edges, "all_types": all_types, "duplicates": duplicates, "long_values": long_values,
           "huge_record": huge_record, "clipped": clipped}


def apply(name, g, seed=0, **kw):
    return LAYOUTS[name](g, seed, **kw)
