// record_core.h — what the simplex kernels decide about ONE raw BAM record before any lane, LDS slice or launch comes into it, as host + device
// functions: the fixed header, the layout test, the streaming-shape rules, the `<n>M` reading of MC, the mate clip of two single-M alignments, the
// walk of "clips around one aligned block", the pairing hash of the read name, and the unpacking of the aux walk's result.  One source for the
// parsers of fastpath.hip and its include files (k_family, k_family_wave, k_simplex_wave2, k_simplex_seg, k_split_parse, k_deep_parse, k_wide_parse)
// and for tests/devemu/record_core.cpp, where the same functions run on the host against bam::mate_clip and the oracle (tests/test_record_core.py).
//
// Reference rules restated here: crates/fgumi-raw-bam/src/overlap.rs:181-357 (bases extending past the mate), vanilla_caller.rs:1119-1124 (absent
// qualities), 1795-1797 and 1897-1908 (the first record's MI tag and the consensus read name).  The byte sources differ between the kernels (an LDS
// slice, the global record, the split kernel's head window): whatever reads bytes takes values or small callables, never a pointer convention.
#pragma once
#include "bamrec.h"

// (device code: inlined where it is called, like the kernels' own helpers)
#if defined(__HIPCC__)
#define REC_HD __host__ __device__ __forceinline__
#else
#define REC_HD inline
#endif

namespace fgx {

// The result of aux_walk (fastpath.hip): bit 0 MC, 1 <tag>, 2 RX, 3 <cell tag> of `got`; pk_* = value offset | value length << 16
struct AuxTags {
  uint32_t got, oddw;                          // keys found with a Z value ; <tag> / RX / <cell tag> values longer than 255 bytes
  uint32_t pk_mc, pk_mi, pk_rx, pk_cb;         // value offset in LDS | value length << 16
};

namespace record {

constexpr int32_t POS_LIMIT = 1 << 30;         // the kernels' closed forms take pos / mate pos in [0, 2^30)
constexpr uint32_t MAX_L_SEQ = 65535;          // per-record state keeps lengths and offsets in 16 bits

// ---- the fixed header, from the record's first dwords (values, not a pointer: k_split_parse holds them in registers).  Dwords 0 - 4 here, the mate's two
// apart below; the eighth, tlen, is read by nobody ----------------------------------------------------------------------------------------------
struct FixedHeader {
  int32_t ref_id, pos;
  uint32_t l_name, n_cig, flags, l_seq;        // l_name counts the NUL
};
REC_HD FixedHeader decode_header(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t d4) {
  FixedHeader H;
  H.ref_id = (int32_t)d0; H.pos = (int32_t)d1; H.l_name = d2 & 0xFF; H.n_cig = d3 & 0xFFFF; H.flags = d3 >> 16; H.l_seq = d4;
  return H;
}
// dwords five and six: where the mate lies.  Apart from the header: only the mate clip reads them, and a kernel that fetches its bytes from memory does so there
struct MateFields { int32_t ref_id, pos; };
REC_HD MateFields decode_mate(uint32_t d5, uint32_t d6) { MateFields M; M.ref_id = (int32_t)d5; M.pos = (int32_t)d6; return M; }
REC_HD bool mate_in_range(const MateFields& M) { return M.pos >= 0 && M.pos < POS_LIMIT; }

// ---- the layout test: where SEQ, QUAL and the tag block start in a record of `len` bytes; odd = the record does not hold them, a sequence
// beyond MAX_L_SEQ, or no read name at all (l_name counts the NUL).  The offsets are meaningful only where !odd (then aux_off <= len) ----------
struct Layout { uint32_t seq_off, qual_off, aux_off; bool odd; };
REC_HD Layout layout(const FixedHeader& H, uint32_t len) {
  const unsigned long long seq_off = 32ull + H.l_name + 4ull * H.n_cig;
  const unsigned long long qual_off = seq_off + ((unsigned long long)H.l_seq + 1) / 2;
  const unsigned long long aux_off = qual_off + H.l_seq;
  Layout L;
  L.seq_off = (uint32_t)seq_off; L.qual_off = (uint32_t)qual_off; L.aux_off = (uint32_t)aux_off;
  L.odd = aux_off > len || H.l_seq > MAX_L_SEQ || H.l_name == 0;
  return L;
}

// ---- the streaming shape (k_simplex_wave2, k_simplex_seg, k_split_parse, k_deep_parse, k_wide_parse): a primary record of an end, either mapped
// at pos in [0, 2^30) with one M/=/X op of l_seq bases, or unmapped without a CIGAR.  A record that is odd sends its family on --------------------
// Header part.  What differs between the kernels:
//   max_cig        1; WG_CIG_OPS in k_deep_parse<.., .., CLIPS = 1>, whose CIGAR may be clips around one aligned block (CigarBlock below)
//   take_unmapped  an unmapped record without a CIGAR is in the shape; false in k_deep_parse<.., .., 1> and in the methylation-aware mode
//                  (meth_mode), which needs a position for every read
//   head_window    0; SP_HEAD in k_split_parse, which keeps name + first CIGAR op in a window of that many bytes behind the fixed header
REC_HD bool streaming_header_odd(const FixedHeader& H, uint32_t max_cig, bool take_unmapped, uint32_t head_window) {
  const bool unm = (H.flags & bam::F_UNMAPPED) != 0;
  if (H.l_seq == 0) return true;
  if (unm ? (!take_unmapped || H.n_cig != 0) : (H.n_cig == 0 || H.n_cig > max_cig)) return true;
  return head_window != 0 && H.l_name + 4u > head_window;
}
// Flag and position part.  `frag_with_mate_flags_odd`: k_split_parse alone refuses an unpaired record that carries FIRST or LAST (a fragment for
// the caller, a mate for the overlap step); the other four kernels keep it — whether they mean to is not recorded anywhere (profiles/record_core.md)
REC_HD bool streaming_flags_odd(const FixedHeader& H, bool frag_with_mate_flags_odd) {
  const uint32_t f = H.flags;
  if (f & (bam::F_SECONDARY | bam::F_SUPPLEMENTARY)) return true;
  if ((f & bam::F_PAIRED) && !(f & (bam::F_FIRST | bam::F_LAST))) return true;                   // counted, but in no end
  if (frag_with_mate_flags_odd && !(f & bam::F_PAIRED) && (f & (bam::F_FIRST | bam::F_LAST))) return true;
  return !(f & bam::F_UNMAPPED) && (H.pos < 0 || H.pos >= POS_LIMIT);
}
// the CIGAR of a mapped record of the shape: one M / = / X op of l_seq bases
REC_HD bool single_block_op(uint32_t op, uint32_t l_seq) {
  const uint32_t t = op & 15;
  return (t == 0 || t == 7 || t == 8) && (op >> 4) == l_seq;
}

// ---- clips around one aligned block: H* S* (M|=|X)+ S* H* — `lead` soft-clipped query bases, `aln` aligned ones, `trail` behind them; `tot` = the
// lengths of all ops, hard clips included.  Feed the ops in order; ok = the shape holds so far, cplx = an I / D / N / P op was seen (not ok then) ---
struct CigarBlock { uint32_t phase, lead, aln, trail, tot; bool ok, cplx; };   // phase 0: leading clips, 1: the block, 2: trailing clips
REC_HD CigarBlock cigar_block_start() { CigarBlock B; B.phase = B.lead = B.aln = B.trail = B.tot = 0; B.ok = true; B.cplx = false; return B; }
REC_HD void cigar_block_op(CigarBlock& B, uint32_t op) {
  const uint32_t t = op & 15, ln = op >> 4;
  B.tot += ln;
  if (t == 0 || t == 7 || t == 8) { if (B.phase == 2) B.ok = false; B.phase = 1; B.aln += ln; }
  else if (t == 4) { if (B.phase == 0) B.lead += ln; else { B.phase = 2; B.trail += ln; } }
  else if (t == 5) { if (B.phase == 1) B.phase = 2; }
  else { B.ok = false; if (t == 1 || t == 2 || t == 3 || t == 6) B.cplx = true; }
}
// the walked ops are a read of l_seq query bases around a block that is not empty
REC_HD bool cigar_block_fits(const CigarBlock& B, uint32_t l_seq) { return B.ok && B.aln != 0 && (unsigned long long)B.lead + B.aln + B.trail == l_seq; }

// ---- `<n>M` from an MC value of mc_len bytes: 1 - 7 digits and an M, n > 0.  Returns n (<= 9 999 999), 0 = MC is not of this form.  v8() fetches the
// value's first eight bytes, little endian; it is called only for mc_len in 2 .. 8 (it may bring up to six bytes past the value) ----------------------
template <class V8>
REC_HD uint32_t mc_single_m(uint32_t mc_len, V8&& v8) {
  if (mc_len < 2 || mc_len > 8) return 0;
  const unsigned long long v = v8();
  uint32_t k = 0, val = 0;
  while (k < mc_len - 1) { const uint32_t ch = (uint32_t)(v >> (8 * k)) & 0xFF; if (ch < '0' || ch > '9') break; val = val * 10 + (ch - '0'); k++; }
  return (k == mc_len - 1 && ((v >> (8 * k)) & 0xFF) == 'M') ? val : 0;
}

// ---- the mate clip of two single-M alignments (overlap.rs:181-357 in closed form): how many query bases of a read of L bases at pos extend past
// a mate of ML bases at mpos.  Range argument, stated once: the callers guard 0 <= pos, mpos < 2^30, 1 <= ML <= 9 999 999 (seven digits of MC; a
// mate in hand: <= 65 535) and 1 <= L <= 65 535, so every term below lies within +-(2^30 + 10^7 + 2^16) and 32-bit signed arithmetic is exact —
// none of the reference's saturating steps can trigger.  The result is <= L.
// The overlap itself, for a pair already known to be FR (the CODEC caller decides that from the mate in hand): `rev` = this read is the reverse one
REC_HD uint32_t single_m_overlap_clip(bool rev, int32_t pos, int32_t L, int32_t mpos, int32_t ML) {
  const int32_t tp = pos + 1, mp = mpos + 1;
  const int32_t read_end = tp - 1 + L, mate_end = mp - 1 + ML;
  int32_t cl = 0;
  if (rev) {
    if (!(tp > mate_end) && !(read_end < mp)) {
      const int32_t fs = tp > mp ? tp : mp;
      int32_t rb = fs - tp; if (rb > L) rb = L;
      int32_t mb = fs - mp; if (mb > ML) mb = ML;
      cl = rb > mb ? rb - mb : 0;
    }
  } else {
    if (!(read_end < mp) && !(mate_end < tp)) {
      const int32_t ls = read_end < mate_end ? read_end : mate_end;
      int32_t ra = ls - tp + 1; if (ra > L) ra = L;
      int32_t ma = ls - mp + 1; if (ma > ML) ma = ML;
      const int32_t rp = L - ra, mq = ML - ma;
      cl = rp > mq ? rp - mq : 0;
    }
  }
  return (uint32_t)cl;
}
// The whole rule from this record's header and its MC's `<ML>M`: is_fr_pair (paired, mate mapped, one reference, opposite strands, the forward
// read not behind the reverse one's end), then the overlap.  `ref_id`: H.ref_id, or the caller's stand-in for it.
REC_HD uint32_t single_m_mate_clip(const FixedHeader& H, int32_t ref_id, const MateFields& M, int32_t ML) {
  const uint32_t f = H.flags;
  const bool rv = (f & bam::F_REVERSE) != 0, mrv = (f & bam::F_MATE_REVERSE) != 0;
  const int32_t L = (int32_t)H.l_seq, tp = H.pos + 1, mp = M.pos + 1;
  bool fr = (f & bam::F_PAIRED) && !(f & bam::F_MATE_UNMAPPED) && ref_id == M.ref_id && rv != mrv;
  if (fr) fr = rv ? (mp < tp + (L - 1)) : (tp < mp + (ML - 1));
  return fr ? single_m_overlap_clip(rv, H.pos, L, M.pos, ML) : 0u;
}

// ---- the pairing hash of a read name: 30 bits of rotate / xor / add (32-bit multiplies issue at a quarter of the rate) over whole 8-byte steps, then
// one step over the LAST 8 bytes (it may overlap the step before; a name below 8 bytes: its bytes, zero-extended).  A filter only: candidates are
// compared byte by byte afterwards.  w32(o) / w64(o) fetch 4 / 8 bytes at offset o from the name's start, little endian; w64 is called with o == 0
// alone, for a name below 8 bytes, and may bring bytes past the name (they are masked off) ---------------------------------------------------
template <class W32, class W64>
REC_HD uint32_t name_hash30(uint32_t name_len, W32&& w32, W64&& w64) {
  auto rotl = [](uint32_t v, uint32_t r) { return (v << r) | (v >> (32u - r)); };
  uint32_t h = name_len, i = 0;
  for (; i + 8 <= name_len; i += 8) { h = rotl(h, 5) ^ w32(i); h = rotl(h, 11) + w32(i + 4); }
  if (i < name_len) {
    uint32_t w0, w1;
    if (name_len >= 8) { w0 = w32(name_len - 8); w1 = w32(name_len - 4); }
    else { const unsigned long long v = w64(0u) & ((1ULL << (8 * name_len)) - 1ULL); w0 = (uint32_t)v; w1 = (uint32_t)(v >> 32); }
    h = rotl(h, 5) ^ w0; h = rotl(h, 11) + w1;
  }
  return h ^ (h >> 15) ^ (h << 7);
}

// ---- the aux walk's result, unpacked; offsets as aux_walk was given them (its a0 included) -------------------------------------------------
struct TagFields {
  bool has_mc, has_mi, has_rx, has_cb;
  uint32_t mc_lo, mc_len, mi_lo, mi_len, rx_lo, rx_len, cb_lo, cb_len;
};
REC_HD TagFields unpack_tags(const AuxTags& ax) {
  TagFields T;
  T.has_mc = (ax.got & 1u) != 0; T.mc_lo = ax.pk_mc & 0xFFFF; T.mc_len = ax.pk_mc >> 16;
  T.has_mi = (ax.got & 2u) != 0; T.mi_lo = ax.pk_mi & 0xFFFF; T.mi_len = ax.pk_mi >> 16;
  T.has_rx = (ax.got & 4u) != 0; T.rx_lo = ax.pk_rx & 0xFFFF; T.rx_len = ax.pk_rx >> 16;
  T.has_cb = (ax.got & 8u) != 0; T.cb_lo = ax.pk_cb & 0xFFFF; T.cb_len = ax.pk_cb >> 16;
  return T;
}
// The first record of a family must carry the MI tag, and `<prefix>:<MI>` must be a legal read name (below 255 bytes with its NUL): fatal in the
// reference otherwise (vanilla_caller.rs:1897-1908, 1795-1797) — the family is not a device kernel's
REC_HD bool first_record_odd(bool has_mi, uint32_t mi_len, uint32_t prefix_len) { return !has_mi || prefix_len + 1 + mi_len >= 255; }

}  // namespace record
}  // namespace fgx
