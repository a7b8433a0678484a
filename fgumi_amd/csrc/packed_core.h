// packed_core.h — the arithmetic of k_split_cols's PACKED column pass (round 5) as host + device functions: one source for the kernel
// (simplex_split.inc, run_cols_packed) and for tests/devemu, where the same functions run on the host against a column-by-column
// restatement and the oracle's ConsensusBaseBuilder (tests/test_packed_core.py).
//
// A lane of the pass owns EIGHT neighbouring tile positions of one end: position p of its group is quality byte p of a 64-bit word of a
// quality row and code nibble (p ^ 1) of a 32-bit word of a sequence row (BAM packs the even position into the high nibble).  Per row the
// codes of observations below --min-input-base-quality are cleared; the lane keeps the OR of the codes and two words of byte counters
// (8 x the number of codes that are not 0: low nibbles = odd positions, high nibbles = even positions).  A column shows ONE base when its
// OR is 1, 2, 4 or 8; its counter is then the number of its observations.  From unanimous_cap_depth (gate_core.h) observations on such a
// column is (base, cap) whatever the qualities are; a column of no observation is ('N', 2 | 0); every other column — a second base, a
// non-ACGT code, one base seen fewer times — is FLAGGED: its observations travel to k_call_full (or, a single observation: to the table
// of fill_t1).  A code 0 ('=') of good quality is no observation for the reference (ConsensusBaseBuilder::add ignores what is not ACGT,
// base_builder.rs:836-868; k_call_full skips it the same way) and adds nothing here.
#pragma once
#include <cstdint>
#include "consensus_math.h"

namespace fgx {
namespace pk {

constexpr uint32_t H = 0x80808080u;

// v_perm_b32: byte i of the result = byte sel[i] of the eight bytes {a (4 - 7), b (0 - 3)}; selector 0x0C = the constant 0
FGX_HD uint32_t perm(uint32_t a, uint32_t b, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(a, b, sel);
#else
  const unsigned long long src = ((unsigned long long)a << 32) | b;
  uint32_t r = 0;
  for (int i = 0; i < 4; i++) {
    const uint32_t s = (sel >> (8 * i)) & 0xFFu;
    const uint32_t byte = s < 8u ? (uint32_t)(src >> (8 * s)) & 0xFFu : 0u;      // (only the selectors this file uses)
    r |= byte << (8 * i);
  }
  return r;
#endif
}
FGX_HD uint32_t bitrev32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bitreverse32(x);
#else
  x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1); x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
  x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4); return __builtin_bswap32(x);
#endif
}

// Two three-input boolean functions, one instruction each on gfx950 (v_bitop3_b32; byte of the truth table: a = 0xF0, b = 0xCC, c = 0xAA).  Spelled out
// because the compiler, left alone, reassociates an OR chain over the rows (four instructions per word where two do) and shares x | b
// between its two uses below (four where three do).
FGX_HD uint32_t or_andn(uint32_t z, uint32_t t, uint32_t q) {      // z | (t & ~q)
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
  return __builtin_amdgcn_bitop3_b32(t, q, z, 0xBA);
#else
  return z | (t & ~q);
#endif
}
FGX_HD uint32_t or_and(uint32_t x, uint32_t b, uint32_t c) {       // (x | b) & c
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
  return __builtin_amdgcn_bitop3_b32(x, b, c, 0xA8);
#else
  return (x | b) & c;
#endif
}

// positions of the group at or past the end's read length are no columns: masks of the quality bytes that count (bit 7 of each)
FGX_HD void count_masks(uint32_t lenE, uint32_t k, uint32_t* nfl, uint32_t* nfh) {
  *nfl = H; *nfh = H;
  const uint32_t nv = lenE > 8u * k ? lenE - 8u * k : 0u;
  if (nv < 8u) { const unsigned long long f = ~(0x8080808080808080ull << (8u * nv)); *nfl &= (uint32_t)f; *nfh &= (uint32_t)(f >> 32); }
}
// any quality of the group's positions below the floor?  (x - floor) & ~x & 0x80 per byte: not zero <=> some byte is (exact as a TEST for
// floors up to 128: a borrow can only raise a false flag above a true one)
FGX_HD bool any_below(uint32_t qx, uint32_t qy, uint32_t mb4, uint32_t nfl, uint32_t nfh) {
  return ((((qx - mb4) & ~qx & nfl) | ((qy - mb4) & ~qy & nfh))) != 0u;
}
// the code nibbles to keep: 0xF where the position's quality is at or above the floor.  Bit 7 of each byte of gl / gh = "at or above"
// (no borrow between bytes: q | 0x80 >= 128 >= floor; a quality >= 128 is above every floor this pass takes).  Without a branch: two
// byte permutes bring the flags of the even and of the odd positions into the order of the sequence bytes (byte i of a sequence word =
// positions 2 i, high nibble, and 2 i + 1, low nibble), the odd ones move to bit 3, and (x << 1) - (x >> 3) widens bit 7 to 0xF0 and bit 3
// to 0x0F in one subtraction (0x100 - 0x10, 0x10 - 0x01; the top byte's 0x100 falls off the word, as it should).
FGX_HD uint32_t keep_mask(uint32_t qx, uint32_t qy, uint32_t mb4) {
  const uint32_t gl = ((qx | H) - mb4) | qx, gh = ((qy | H) - mb4) | qy;
  const uint32_t ev = perm(gh, gl, 0x06040200u), od = perm(gh, gl, 0x07050301u);
  const uint32_t f = (ev & H) | ((od >> 4) & 0x08080808u);
  return (f << 1) - (f >> 3);
}
// (the restatement bit by bit, as the pass ran up to round 6: tests/test_packed_rows_core.py holds the two against each other)
FGX_HD uint32_t keep_mask_bitwise(uint32_t qx, uint32_t qy, uint32_t mb4) {
  const uint32_t gl = ((qx | H) - mb4) | qx, gh = ((qy | H) - mb4) | qy;
  uint32_t keep = 0;
  keep |= (uint32_t)((int32_t)(gl << 24) >> 31) & 0x000000F0u; keep |= (uint32_t)((int32_t)(gl << 16) >> 31) & 0x0000000Fu;
  keep |= (uint32_t)((int32_t)(gl << 8) >> 31) & 0x0000F000u;  keep |= (uint32_t)((int32_t)gl >> 31) & 0x00000F00u;
  keep |= (uint32_t)((int32_t)(gh << 24) >> 31) & 0x00F00000u; keep |= (uint32_t)((int32_t)(gh << 16) >> 31) & 0x000F0000u;
  keep |= (uint32_t)((int32_t)(gh << 8) >> 31) & 0xF0000000u;  keep |= (uint32_t)((int32_t)gh >> 31) & 0x0F000000u;
  return keep;
}

// CLEAN rows (round 7).  The only writer of qualities between staging and the column pass is the overlap correction, and it writes a
// quality below the floor only together with code 0 (shared_base: `drop`); the clip phase only clears codes.  So a family whose RAW
// qualities — at the positions below each read's own length — are all at or above the floor reaches the column pass with code 0 under
// every sub-floor quality: b & keep_mask(q) == b for every row, and the row loop needs no quality at all (acc_row_seq).  The test, once
// per family on the staged tile: a lane takes group k of its end and ORs (q - floor) & ~q over the end's rows; bit 7 of a byte is set
// where the byte is below the floor; a borrow can only raise a false flag (or hide a true one) ABOVE a true one, and the length mask cuts
// positions from the top: what it keeps of a word holds a flag exactly when it holds a byte below the floor.  Exact as a test of the group
// for floors up to 128 (a byte of 128 and above is below no such floor); above 128 nothing is clean.
struct Below { uint32_t lo, hi; };
FGX_HD void below_reset(Below& z) { z.lo = 0; z.hi = 0; }
FGX_HD void below_row(Below& z, uint32_t qx, uint32_t qy, uint32_t mb4) { z.lo = or_andn(z.lo, qx - mb4, qx); z.hi = or_andn(z.hi, qy - mb4, qy); }
// rows of ONE length: the masks of count_masks(that length, k) once, behind the last row
FGX_HD bool below_any(const Below& z, uint32_t nfl, uint32_t nfh) { return ((z.lo & nfl) | (z.hi & nfh)) != 0u; }
// a row of its own length (a read shorter than its end's rows: what lies behind it in its last 16-byte chunk is tag text)
FGX_HD void below_row_len(Below& z, uint32_t qx, uint32_t qy, uint32_t mb4, uint32_t l_seq, uint32_t k) {
  uint32_t nfl, nfh;
  count_masks(l_seq, k, &nfl, &nfh);
  z.lo |= (qx - mb4) & ~qx & nfl; z.hi |= (qy - mb4) & ~qy & nfh;
}

struct Acc { uint32_t f_or, A8, B8; };     // OR of the codes (eight nibbles); 8 x the codes that are not 0 per byte: low nibbles, high nibbles
FGX_HD void acc_reset(Acc& a) { a.f_or = 0; a.A8 = 0; a.B8 = 0; }
// one row of the lane's group whose codes stand as they are (a clean family's): b = its eight codes
FGX_HD void acc_row_seq(Acc& a, uint32_t b) {
  a.f_or |= b;
  const uint32_t x = (b & 0x77777777u) + 0x77777777u;                          // bit 3 of each nibble of x | b: the nibble is not 0
  a.A8 += or_and(x, b, 0x08080808u); a.B8 += or_and(x, b, 0x80808080u) >> 4;
}
// one row of the lane's group: q = its eight qualities (qx: positions 0 - 3), b = its eight codes.  (Up to round 6 the clearing ran behind
// any_below(.., nfl, nfh), a divergent block of 27 instructions for the whole wavefront as soon as one lane held a sub-floor quality —
// every row of a family with overlapping mates; the masks no longer matter: codes at positions past the end are no columns.)
FGX_HD void acc_row(Acc& a, uint32_t qx, uint32_t qy, uint32_t b, uint32_t mb4, uint32_t /*nfl*/ = 0, uint32_t /*nfh*/ = 0) { acc_row_seq(a, b & keep_mask(qx, qy, mb4)); }

// What the lane's eight slots are: slot s = column c_lo + s of its end (forward end: position s of the group; reverse end: position
// 7 - s, complemented).  code2 / qual2: a byte per slot; dep4: 16 bits per slot; flag2 / valid2: bit 7 of the slot's byte — flagged
// (k_call_full's) / a column of the end.  Slots [lo_s, hi_s) are the columns.
struct Out { uint32_t code2[2], qual2[2], dep4[4], flag2[2], valid2[2]; int32_t c_lo, lo_s, hi_s; };
FGX_HD void finalize(const Acc& a, bool inl, bool lrev, uint32_t lenE, uint32_t cntE, uint32_t k, uint32_t nsafe, uint32_t cap, uint32_t min_cons_bq, uint32_t min_reads, Out& o) {
  uint32_t f_or = a.f_or, Ce = a.A8 >> 3, Co = a.B8 >> 3;                      // observations per column, a byte each: odd / even positions
  // reverse end: bit reversal of the OR word complements the codes AND puts them in column order; the counters are byte-swapped
  if (lrev) { f_or = bitrev32(f_or); const uint32_t t = __builtin_bswap32(Ce); Ce = __builtin_bswap32(Co); Co = t; }
  o.c_lo = lrev ? (int32_t)lenE - 8 - 8 * (int32_t)k : 8 * (int32_t)k;         // (below zero for the reverse end's last group)
  const int32_t hi_r = (int32_t)cntE - o.c_lo;
  o.lo_s = o.c_lo < 0 ? -o.c_lo : 0; o.hi_s = !inl || hi_r < 0 ? 0 : hi_r > 8 ? 8 : hi_r;
  unsigned long long V = 0;
  if (o.hi_s > o.lo_s) {
    const unsigned long long hiM = o.hi_s >= 8 ? ~0ull : (1ull << (8 * o.hi_s)) - 1ull, loM = (1ull << (8 * (o.lo_s > 7 ? 7 : o.lo_s))) - 1ull;
    V = hiM & ~loM & 0x8080808080808080ull;
  }
  const uint32_t N4 = nsafe * 0x01010101u;
  const bool cap_lt = cap < min_cons_bq;                                       // (the cap itself is below --min-consensus-base-quality: every answered column is masked)
  const uint32_t QA4 = (cap_lt ? (uint32_t)FGX_MIN_PHRED : cap) * 0x01010101u, QZ4 = (min_reads > 0u ? 0u : (uint32_t)FGX_MIN_PHRED) * 0x01010101u;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    // the four slots of this half, a byte each: OR of the codes (O), observations (C)
    const uint32_t Pb = perm(f_or, f_or, h ? 0x03030202u : 0x01010000u);       // bytes {b, b, b', b'}: slots 2i (high nibble), 2i + 1 (low nibble)
    const uint32_t O = ((Pb >> 4) & 0x000F000Fu) | (Pb & 0x0F000F00u);
    const uint32_t C = perm(Ce, Co, h ? 0x07030602u : 0x05010400u);
    const uint32_t Vh = h ? (uint32_t)(V >> 32) : (uint32_t)V;
    // one base: the byte is 1, 2, 4 or 8  <=>  not 0 and x & (x - 1) == 0  ((x | 0x80) - 1: no borrow between bytes)
    const uint32_t Z = O & ((O | H) - 0x01010101u) & 0x0F0F0F0Fu;
    const uint32_t nzO = (O + 0x7F7F7F7Fu) & H, nzZ = (Z + 0x7F7F7F7Fu) & H;
    const uint32_t ge = ((C | H) - N4) & H;                                    // at least nsafe observations (both below 128: no borrow)
    const uint32_t capF = Vh & nzO & ~nzZ & ge;                                // (base, cap)
    o.flag2[h] = Vh & nzO & ~capF;                                             // some observation and no answer here
    o.valid2[h] = Vh;
    const uint32_t capM = (capF << 1) - (capF >> 7);                           // 0xFF in the bytes of the flags
    o.code2[h] = cap_lt ? 0x0F0F0F0Fu : ((O & capM) | (0x0F0F0F0Fu & ~capM));
    o.qual2[h] = (QA4 & capM) | (QZ4 & ~capM);
    const uint32_t D = C & capM;
    o.dep4[2 * h] = perm(0u, D, 0x0C010C00u); o.dep4[2 * h + 1] = perm(0u, D, 0x0C030C02u);
  }
}

// ---- the overlap correction of two mates on packed words (round 8; simplex_split.inc phase 2; overlapping.rs:236-336) ---------------------
// A lane takes one pair and EIGHT neighbouring shared positions.  The groups are aligned to the mate whose first shared base is its base 0
// ("A": one of the two offsets of a pair is always 0): A's qualities are two whole dwords, its codes one whole word, and they belong to the
// lane alone.  The other mate ("B") starts `off` positions into its read: its bytes are gathered from the neighbouring aligned words with a
// funnel shift (ov_gather_q / ov_gather_c) and what changes goes back as XOR deltas (ov_scatter_q / ov_scatter_c) — a word of B is shared by
// two neighbouring groups, their positions in it are disjoint, so the deltas compose in any order, and a lane that loads a word after a
// neighbour's delta finds its own positions as they were.
//
// The rule per shared position (c1, c2 the codes, qa, qb the qualities; symmetric in the mates): nothing if either code is 15; c1 == c2: both
// qualities min(qa + qb, 93); else both qualities max(|qa - qb|, 2) and both codes the one of the higher quality (15 on a tie); a new quality
// below the floor clears both codes (`drop`, also on agreement: the clean rows above rest on it).  Both mates end with ONE quality and ONE code.
// Byte-wise sums are exact while qa + qb < 256: the kernel sends a family with a shared quality of 128 or more down its byte-wise path
// (ov_high is the test); the arithmetic below masks bit 7 away so that such a byte OUTSIDE the overlap cannot carry into a neighbour.
FGX_HD uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t n) {  // v_alignbyte_b32: ({hi, lo} >> 8 n), low word; n = 0 .. 3
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, n);
#else
  return (uint32_t)(((((unsigned long long)hi) << 32) | lo) >> (8u * (n & 3u)));
#endif
}
FGX_HD uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t n) {   // v_alignbit_b32: ({hi, lo} >> n), low word; n = 0 .. 31
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, n);
#else
  return (uint32_t)(((((unsigned long long)hi) << 32) | lo) >> (n & 31u));
#endif
}
FGX_HD uint32_t popc(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_popcount(x);
#else
  x = x - ((x >> 1) & 0x55555555u); x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
  return (((x + (x >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24;
#endif
}
FGX_HD uint32_t widen(uint32_t h) { return h - (h >> 7); }   // bit 7 of each byte -> 0x7F (h holds bits 7 only): a select mask for bytes below 128 — every quality the step computes, every code
FGX_HD uint32_t swap_nibbles(uint32_t x) { return ((x & 0x0F0F0F0Fu) << 4) | ((x >> 4) & 0x0F0F0F0Fu); }   // BAM order (even position high) <-> position order
// the four codes of half h of a word, a byte each: from BAM order / from position order
FGX_HD uint32_t expand_bam(uint32_t c, int h) { const uint32_t P = perm(c, c, h ? 0x03030202u : 0x01010000u); return ((P >> 4) & 0x000F000Fu) | (P & 0x0F000F00u); }
FGX_HD uint32_t expand_pos(uint32_t c, int h) { const uint32_t P = perm(c, c, h ? 0x03030202u : 0x01010000u); return (P & 0x000F000Fu) | ((P >> 4) & 0x0F000F00u); }
// ... and back: eight bytes of at most 15 to one word
FGX_HD uint32_t compress_bam(uint32_t lo, uint32_t hi) { return perm((hi << 4) | (hi >> 8), (lo << 4) | (lo >> 8), 0x06040200u); }
FGX_HD uint32_t compress_pos(uint32_t lo, uint32_t hi) { return perm(hi | (hi >> 4), lo | (lo >> 4), 0x06040200u); }

// positions of group k inside the overlap [0, cn): 0xFF per byte (k < ceil(cn / 8); a lane outside the index space passes cn = 0)
FGX_HD void ov_in_masks(uint32_t cn, uint32_t k, uint32_t* ml, uint32_t* mh) {
  const uint32_t nv = cn > 8u * k ? cn - 8u * k : 0u;
  const unsigned long long m = nv >= 8u ? ~0ull : (1ull << (8u * nv)) - 1ull;
  *ml = (uint32_t)m; *mh = (uint32_t)(m >> 32);
}
// B's eight qualities from the three aligned dwords that hold bytes [4 (off / 4) + 8 k, + 12) of its row; s = off & 3
FGX_HD void ov_gather_q(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t s, uint32_t* qx, uint32_t* qy) { *qx = alignbyte(d1, d0, s); *qy = alignbyte(d2, d1, s); }
// B's eight codes in POSITION order from the two aligned words that hold positions [8 (off / 8) + 8 k, + 16); sn = off & 7
FGX_HD uint32_t ov_gather_c(uint32_t w0, uint32_t w1, uint32_t sn) { return alignbit(swap_nibbles(w1), swap_nibbles(w0), 4u * sn); }
// the deltas of B on their way back: the dwords of ov_gather_q / the words of ov_gather_c (BAM order again)
FGX_HD void ov_scatter_q(uint32_t dx, uint32_t dy, uint32_t s, uint32_t* e /* [3] */) {
  const unsigned long long D = (((unsigned long long)dy) << 32) | dx, L = D << (8u * s);
  e[0] = (uint32_t)L; e[1] = (uint32_t)(L >> 32); e[2] = (uint32_t)((D >> 8) >> (56u - 8u * s));    // (s = 0: shifted out)
}
FGX_HD void ov_scatter_c(uint32_t d, uint32_t sn, uint32_t* f /* [2] */) {
  f[0] = swap_nibbles(d << (4u * sn)); f[1] = swap_nibbles((d >> 4) >> (28u - 4u * sn));
}
// a quality of 128 or more at a shared position: the family is the byte-wise step's
FGX_HD bool ov_high(uint32_t qax, uint32_t qay, uint32_t qbx, uint32_t qby, uint32_t ml, uint32_t mh) { return ((((qax | qbx) & ml) | ((qay | qby) & mh)) & H) != 0u; }

// four positions: qa, qb the qualities, ca, cb the codes as bytes, inr = ov_in_masks, mb4 = 4 x the floor (at most 128).  Bit 7 of a byte of
// agree / dis / chg: a valid agreement / a valid disagreement / an agreement whose sum differs from qa or qb.
struct OvHalf { uint32_t newq, newc, validM, agree, dis, chg; };
FGX_HD void ov_half(uint32_t qa, uint32_t qb, uint32_t ca, uint32_t cb, uint32_t inr, uint32_t mb4, OvHalf& o) {
  const uint32_t L = 0x7F7F7F7Fu;
  qa &= L; qb &= L;
  const uint32_t isN = ((ca + 0x71717171u) | (cb + 0x71717171u)) & H;          // a code is 15 (codes are at most 15: no carry)
  const uint32_t ne = ((ca ^ cb) + L) & H;
  const uint32_t valid = inr & ~isN & H;
  const uint32_t s = qa + qb;                                                  // (both below 128: no carry)
  const uint32_t overM = widen((s | ((s & L) + 0x22222222u)) & H);             // 94 and more: bit 7 of s, or of (s & 127) + 34
  const uint32_t nq = ((s & L) & ~overM) | (0x5D5D5D5Du & overM);                // (a sum below 94 has no bit 7)
  const uint32_t xg = (qa | H) - qb, yg = (qb | H) - qa;                       // bit 7: qa >= qb / qb >= qa; below it the difference mod 128 (no borrow)
  const uint32_t ageM = widen(xg & H);
  const uint32_t ad = ((xg & ageM) | (yg & ~ageM)) & L;
  const uint32_t lt2M = widen(~((ad | H) - 0x02020202u) & H);
  const uint32_t dq = (ad & ~lt2M) | (0x02020202u & lt2M);
  const uint32_t neM = widen(ne);
  o.newq = (dq & neM) | (nq & ~neM);
  const uint32_t dropM = widen(~((o.newq | H) - mb4) & H);                     // the new quality (at most 93) is below the floor
  o.newc = (((ca & ageM) | (cb & ~ageM)) | (0x0F0F0F0Fu & widen(xg & yg & ne))) & ~dropM;   // (an agreement: ca == cb; a tie: N)
  o.validM = widen(valid);                                                     // (a valid position's qualities are below 128 on both mates: ov_high)
  o.agree = valid & ~ne; o.dis = valid & ne;
  o.chg = o.agree & (((nq ^ qa) | (nq ^ qb)) + L);
}
// One lane's step.  In: A's qualities and code word (BAM order) as loaded, B's as gathered, the masks, the floor.  Out: A's words to store, B's
// deltas (qualities: bytes in A's alignment; codes: position order) and the counts — agreements | disagreements << 16, changed agreements.
// The two halves ONE AFTER THE OTHER (the empty asm makes the second wait for the first): interleaved, as the scheduler would have them, their
// temporaries take the kernel past 64 vector registers — eight wavefronts per SIMD — and into scratch.
#if defined(__HIP_DEVICE_COMPILE__)
#define FGX_PK_THEN(a, b, c, d, e, f, g, h, i, j) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h), "+v"(i), "+v"(j))
#else
#define FGX_PK_THEN(a, b, c, d, e, f, g, h, i, j) ((void)0)
#endif
struct OvStep { uint32_t qa[2], ca, dq[2], dc, n_ad, n_chg; };
FGX_HD void ov_step(uint32_t qax, uint32_t qay, uint32_t caw, uint32_t qbx, uint32_t qby, uint32_t cbp, uint32_t ml, uint32_t mh, uint32_t mb4, OvStep& o) {
  uint32_t a8[2], d8[2];                                                       // A's new codes and B's code deltas, a byte each
  o.n_ad = 0; o.n_chg = 0;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const uint32_t qa = h ? qay : qax, qb = h ? qby : qbx, ca = expand_bam(caw, h), cb = expand_pos(cbp, h);
    OvHalf r;
    ov_half(qa, qb, ca, cb, h ? mh : ml, mb4, r);
    o.qa[h] = (r.newq & r.validM) | (qa & ~r.validM);
    a8[h] = (r.newc & r.validM) | (ca & ~r.validM);
    o.dq[h] = (r.newq ^ qb) & r.validM;
    d8[h] = (r.newc ^ cb) & r.validM;
    o.n_ad += popc(r.agree) + (popc(r.dis) << 16); o.n_chg += popc(r.chg);
    if (h == 0) FGX_PK_THEN(o.qa[0], a8[0], o.dq[0], d8[0], o.n_ad, o.n_chg, qay, qby, caw, cbp);
  }
  o.ca = compress_bam(a8[0], a8[1]); o.dc = compress_pos(d8[0], d8[1]);
}

// One observation of base b and quality q: ConsensusBaseBuilder::add from zero leaves s[b] = correct[q], s[other] = error_per_alt[q]
// exactly (Kahan's first step adds to 0), and the call (try_unanimous_fast_path, else call_full: base_builder.rs:883-1081) is a function
// of q alone — evaluated here by the very functions k_call_full runs (column_call, consensus_math.h), once per caller.  t1[q] = the
// consensus quality, 0xFF where the call does not come back with the observed base (the column then travels like any other).
inline void fill_t1(uint8_t* t1 /* [96] */, const ConsensusTables& t) {
  for (uint32_t q = 0; q < 96; q++) {
    t1[q] = 0xFF;
    if (q > 93) continue;
    ColumnAcc acc;
    acc.reset();
    acc.add(0, t.correct[q], t.error_per_alt[q]);
    if (!m_isfinite(acc.s[0]) || !m_isfinite(acc.s[1])) continue;
    int bi = -1;
    uint8_t ql = 0;
    column_call(t, acc.s, acc.obs, &bi, &ql);
    if (bi == 0) t1[q] = ql;
  }
}

// Two observations of ONE base, qualities q1 then q2 in file order (round 6): the same evaluation — two steps of ConsensusBaseBuilder::add
// (the Kahan sums in the reference's order), then the call.  t2[q1 * 94 + q2] = the consensus quality, 0xFF where the call does not come
// back with the observed base.  Such columns are the second most frequent kind the packed pass flags (1.1 per depth-8 family of `simulate`
// data: the read-through zone, where a random subset of the rows survives the overlap correction); answered from the table they need no
// k_call_full item.
constexpr uint32_t T2_DIM = 94, T2_BYTES = T2_DIM * T2_DIM;
inline void fill_t2(uint8_t* t2 /* [T2_BYTES] */, const ConsensusTables& t) {
  for (uint32_t q1 = 0; q1 < T2_DIM; q1++)
    for (uint32_t q2 = 0; q2 < T2_DIM; q2++) {
      uint8_t& out = t2[q1 * T2_DIM + q2];
      out = 0xFF;
      ColumnAcc acc;
      acc.reset();
      acc.add(0, t.correct[q1], t.error_per_alt[q1]);
      acc.add(0, t.correct[q2], t.error_per_alt[q2]);
      if (!m_isfinite(acc.s[0]) || !m_isfinite(acc.s[1])) continue;
      int bi = -1;
      uint8_t ql = 0;
      column_call(t, acc.s, acc.obs, &bi, &ql);
      if (bi == 0) out = ql;
    }
}

}  // namespace pk
}  // namespace fgx
