// record_writers.inc — pass B of the device-resident pipeline: the kernels that serialise consensus records (one wavefront per record or family).
// Included by fastpath.hip inside `namespace fgx { namespace {` after k_call_full and before simplex_wave2.inc.
//
// What comes before: the column kernels (k_family, k_family_wave<MODE>, the split / segment / deep simplex kernels) and k_call_full have left the
// single-strand calls of every column in the scratch arrays (col_code / col_qual / col_depth / col_err / col_obs, col_obs_all under a strand cap,
// meth_flag in the methylation-aware mode), the descriptor of every record (EndDesc / DuplexDesc / CodecDesc) and, after the scan of the record
// sizes, its offset in the output.
//
// What is here: k_emit (simplex: emit_load / emit_store / emit_pair, emit_generic for any length), the duplex and CODEC position rules (duplex_call /
// duplex_column, CodecGeom / codec_column), the field writers (FieldWriterFlat, FieldWriterNested with its any-length forms, put_string / put_i16 /
// put_seq_qual), k_count_slow, and the four duplex / CODEC record kernels: k_emit_duplex_fast / k_emit_codec_fast (registers only, the usual record)
// and k_emit_duplex / k_emit_codec (field after field, any length; launched only when k_count_slow counted a record the fast writers refuse).
//
// What comes after: the simplex column kernels' include files, duplex_meth.inc (the methylation tags behind RX; its duplex bases are duplex_call's)
// and the host driver, which launches all of it.

// byte j of an integer tag `ab:<c|C|S>:v` (smallest type, signed first; v fits an int16 here)
__device__ __forceinline__ uint8_t int_tag_byte(uint32_t j, char a, char b, uint32_t v) {
  return j == 0 ? (uint8_t)a : j == 1 ? (uint8_t)b : j == 2 ? (uint8_t)(v <= 127 ? 'c' : v <= 255 ? 'C' : 'S') : j == 3 ? (uint8_t)v : (uint8_t)(v >> 8);
}

// One wavefront serialises one consensus record (block_size prefix, 32-byte core, name, packed bases, quals, tags
// `RG cD cM cE [cd ce] MI [CB] RX` — vanilla_caller.rs:1767-1881).  The kernel is bound by memory round trips per
// wavefront, not by bytes: so (hot path, consensus <= 192 columns and short names/tags) EVERY load of the record is
// issued before the first store — one wait instead of one per field — descriptor fields are scalar loads, and every
// field group is one full-wave store in which each lane computes the byte it owns (fixed header bytes included).
#ifndef FGX_EMIT_FLAT
#define FGX_EMIT_FLAT 1   /* k_emit's small fields as straight-line code (0: the nested conditionals of rounds 2 - 4, for measurements) */
#endif
struct EmitCtx {
  uint8_t* q; const uint8_t* first; const uint8_t* code; const uint8_t* cq; const uint16_t* cd; const uint16_t* ce;
  uint32_t Lc, name_len, mi_len, mi_off, flag, rec_size;
};

// unaligned global dwords (gfx950 takes them in one instruction)
// (the parsers' pair: gld32 / gld64, fastpath.hip — the same bodies; kept apart because sharing them moves k_emit's registers, profiles/record_core.md)
__device__ __forceinline__ uint32_t gld32u(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint2 gld64u(const uint8_t* p) { uint2 v; __builtin_memcpy(&v, p, 8); return v; }
__device__ __forceinline__ void gst32u(uint8_t* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }
__device__ __forceinline__ void gst16u(uint8_t* p, uint32_t v) { const uint16_t w = (uint16_t)v; __builtin_memcpy(p, &w, 2); }

// The record's fields, each lane computing the byte it owns as nested conditionals over the lane number (the form of rounds 2 - 4).  Two groups of members:
//  * one full-wave store for a field of at most 64 bytes.  k_emit_codec_fast keeps these: the straight-line forms of FieldWriterFlat (below) cost it four
//    registers and with them a wavefront per SIMD (79 -> 83; 0.54 -> 0.53 G raw reads/s, profiles/r04_experiments.md);
//  * the any-length forms of the per-field writers (emit_generic, k_emit_duplex, k_emit_codec): field after field, one load -> store round trip per 64
//    bytes, the value of position i from a callable — what put_string / put_i16 / put_seq_qual are to the register-resident kernels.
struct FieldWriterNested {
  uint8_t* q; uint32_t lane;
  // byte i of the headers: `xyZ` (i < 3) and `xyBs` + the 32-bit count (i < 8)
  static __device__ __forceinline__ uint8_t head3(uint32_t i, char t0, char t1) { return i == 0 ? (uint8_t)t0 : i == 1 ? (uint8_t)t1 : (uint8_t)'Z'; }
  static __device__ __forceinline__ uint8_t head8(uint32_t i, char t0, char t1, uint32_t L) {
    return i == 0 ? (uint8_t)t0 : i == 1 ? (uint8_t)t1 : i == 2 ? (uint8_t)'B' : i == 3 ? (uint8_t)'s' : (uint8_t)(L >> (8 * ((i - 4) & 3)));
  }
  // one store: bytes [0, n) with n <= 64, byte i = f(i)
  template <class F> __device__ __forceinline__ void small(uint32_t n, F f) { if (lane < n) q[lane] = f(lane); q += n; }
  __device__ __forceinline__ void z_small(char t0, char t1, const uint8_t* src, uint32_t n) {       // Z tag, n + 4 <= 64
    const uint32_t k = lane >= 3 ? lane - 3 : 0;
    const uint8_t b = src[k < n ? k : (n ? n - 1 : 0)];
    small(3 + n + 1, [&](uint32_t i) { return i < 3 ? head3(i, t0, t1) : k < n ? b : (uint8_t)0; });
  }
  __device__ __forceinline__ void scalars(char s, bool m_second, uint32_t dmax, uint32_t dmin, float rate) {   // <s>D <s>E <s>M (duplex) or <s>D <s>M <s>E (CODEC)
    uint8_t v;
    const uint32_t u = __float_as_uint(rate);
    if (m_second) {
      if (lane < 4) v = int_tag_byte(lane, s, 'D', dmax);
      else if (lane < 8) v = int_tag_byte(lane - 4, s, 'M', dmin);
      else { const uint32_t j = lane - 8; v = j == 0 ? (uint8_t)s : j == 1 ? (uint8_t)'E' : j == 2 ? (uint8_t)'f' : (uint8_t)(u >> (8 * ((j - 3) & 3))); }
    } else {
      if (lane < 4) v = int_tag_byte(lane, s, 'D', dmax);
      else if (lane < 11) { const uint32_t j = lane - 4; v = j == 0 ? (uint8_t)s : j == 1 ? (uint8_t)'E' : j == 2 ? (uint8_t)'f' : (uint8_t)(u >> (8 * ((j - 3) & 3))); }
      else v = int_tag_byte(lane - 11, s, 'M', dmin);
    }
    if (lane < 15) q[lane] = v;
    q += 15;
  }
  __device__ __forceinline__ void header3(char t0, char t1) { small(3, [&](uint32_t i) { return head3(i, t0, t1); }); }
  __device__ __forceinline__ void header8(char t0, char t1, uint32_t L) { small(8, [&](uint32_t i) { return head8(i, t0, t1, L); }); }
  // block_size + fixed core: ref_id -1, pos -1, l_read_name, mapq 0, bin 4680, n_cigar_op 0, flag, l_seq, next_ref -1, next_pos -1, tlen 0
  __device__ __forceinline__ void core(uint32_t rec_size, uint32_t name_len, uint32_t flag, uint32_t L) {
    if (lane < 36) {
      const uint32_t dw = lane >> 2;
      const uint32_t v = dw == 0 ? rec_size : dw == 3 ? ((name_len + 1) | (4680u << 16)) : dw == 4 ? (flag << 16) : dw == 5 ? L : dw == 8 ? 0u : 0xFFFFFFFFu;
      q[lane] = (uint8_t)(v >> (8 * (lane & 3)));
    }
    q += 36;
  }
  // ---- any length ----
  template <class F> __device__ __forceinline__ void bytes(uint32_t n, F f) { for (uint32_t i = lane; i < n; i += 64) q[i] = f(i); q += n; }   // bytes [0, n), byte i = f(i)
  __device__ __forceinline__ void name(const char* prefix, uint32_t prefix_len, const uint8_t* mi, uint32_t name_len) {   // `<prefix>:<MI>` and its NUL
    bytes(name_len + 1, [&](uint32_t i) { return i < prefix_len ? (uint8_t)prefix[i] : i == prefix_len ? (uint8_t)':' : i < name_len ? mi[i - prefix_len - 1] : (uint8_t)0; });
  }
  __device__ __forceinline__ void z_any(char t0, char t1, const uint8_t* src, uint32_t n) {         // Z tag from a byte string in global memory
    bytes(3 + n + 1, [&](uint32_t i) { return i < 3 ? head3(i, t0, t1) : i - 3 < n ? src[i - 3] : (uint8_t)0; });
  }
  template <class B> __device__ __forceinline__ void string_any(char t0, char t1, uint32_t L, B byte_of) {   // Z tag of L bytes, byte i = byte_of(i)
    bytes(3 + L + 1, [&](uint32_t i) { return i < 3 ? head3(i, t0, t1) : i - 3 < L ? (uint8_t)byte_of(i - 3) : (uint8_t)0; });
  }
  template <class V> __device__ __forceinline__ void i16_any(char t0, char t1, uint32_t L, V val_of) {        // B:s array of L int16 values
    bytes(8 + 2 * L, [&](uint32_t i) -> uint8_t {
      if (i < 8) return head8(i, t0, t1, L);
      const uint32_t k = i - 8, w = val_of(k >> 1);
      return (k & 1) ? (uint8_t)(w >> 8) : (uint8_t)w;
    });
  }
  template <class C, class Q> __device__ __forceinline__ void seq_qual_any(uint32_t L, C code_of, Q qual_of) {   // 4-bit packed bases, then qualities
    bytes((L + 1) / 2, [&](uint32_t i) { const uint32_t hi = code_of(2 * i), lo = 2 * i + 1 < L ? code_of(2 * i + 1) : 0u; return (uint8_t)((hi << 4) | lo); });
    bytes(L, [&](uint32_t i) { return (uint8_t)qual_of(i); });
  }
};

__device__ __forceinline__ uint8_t cdcmce_byte(uint32_t lane, uint32_t n_cd, uint32_t n_cm, uint32_t maxd, uint32_t mind, float rate) {
  if (lane < n_cd) return int_tag_byte(lane, 'c', 'D', maxd);
  if (lane < n_cd + n_cm) return int_tag_byte(lane - n_cd, 'c', 'M', mind);
  const uint32_t j = lane - n_cd - n_cm, u = __float_as_uint(rate);
  return j == 0 ? 'c' : j == 1 ? 'E' : j == 2 ? 'f' : (uint8_t)(u >> (8 * (j - 3)));
}

// depth and error statistics of one strand (or of both together) over the positions of a record: the <s>D <s>M <s>E tags
struct StrandStats {
  uint32_t dmax = 0, dmin = 0xFFFFFFFFu, sd = 0, se = 0;
  __device__ __forceinline__ void add(uint32_t d, uint32_t e) { dmax = d > dmax ? d : dmax; dmin = d < dmin ? d : dmin; sd += d; se += e; }
  __device__ __forceinline__ void reduce() { dmax = wave_max(dmax); dmin = wave_min(dmin); sd = wave_sum(sd); se = wave_sum(se); }   // over the wavefront
  __device__ __forceinline__ float rate() const { return sd ? (float)se / (float)sd : 0.0f; }
};
// a record's three (strand A, strand B, both) over the wavefront; L: the record's length (without a position there is no minimum)
__device__ __forceinline__ void reduce_stats(StrandStats& A, StrandStats& B, StrandStats& AB, uint32_t L) {
  A.reduce(); B.reduce(); AB.reduce();
  if (L == 0) { A.dmin = 0; B.dmin = 0; AB.dmin = 0; }
}

// any length: field after field (one load → store round trip per 64 bytes)
__device__ void emit_generic(const EmitParams& P, const EndDesc& D, const EmitCtx& X, uint32_t lane) {
  const uint32_t Lc = X.Lc;
  const uint8_t* mi = X.first + X.mi_off;
  StrandStats S;
  for (uint32_t i = lane; i < Lc; i += 64) S.add(X.cd[i], X.ce[i]);
  FieldWriterNested W{X.q, lane};
  W.core(X.rec_size, X.name_len, X.flag, Lc);
  W.name(P.prefix, P.prefix_len, mi, X.name_len);
  W.seq_qual_any(Lc, [&](uint32_t i) { return X.code[i]; }, [&](uint32_t i) { return X.cq[i]; });
  W.z_any('R', 'G', (const uint8_t*)P.rg, P.rg_len);
  S.reduce();
  if (Lc == 0) S.dmin = 0;
  // cD cM cE: the widths of the integer tags vary here (int_tag_width), unlike the one-byte forms of the duplex and CODEC records
  const uint32_t n_cd = 3 + int_tag_width(S.dmax), n_cm = 3 + int_tag_width(S.dmin);
  W.small(n_cd + n_cm + 7, [&](uint32_t i) { return cdcmce_byte(i, n_cd, n_cm, S.dmax, S.dmin, S.rate()); });
  if (P.per_base_tags) {
    W.i16_any('c', 'd', Lc, [&](uint32_t i) { return X.cd[i]; });
    W.i16_any('c', 'e', Lc, [&](uint32_t i) { return X.ce[i]; });
  }
  W.z_any(P.tag0, P.tag1, mi, X.mi_len);
  if (D.has_cb) W.z_any(P.cell0, P.cell1, P.blob + D.kept_off + D.cb_off, D.cb_len);
  if (D.has_rx) W.z_any('R', 'X', (const uint8_t*)D.rx, D.rx_len);
}

// One wavefront per FAMILY: its (up to three) records one after the other.  A third of the slots is empty on paired data (the
// fragment slot), and a wavefront that only finds `valid == 0` still costs a launch and a memory round trip; the descriptor
// carries blob OFFSETS, so the record's strings are one dependent load away instead of two (2.35 → 2.20 ms per 2 M records).
// (Assembling the record through LDS — whole-record image with byte writes, or dword-staged column arrays with dword payload
// copies — was measured three times, rounds 1 and 2: 3.4 – 4.0 ms.  The wave's lifetime is a chain of memory round trips, and
// every LDS hop adds one; registers-only streaming below is the fastest form found.)
// A record in two halves: everything it reads (emit_load: every load of the record issued back to back, nothing waited for), and
// the reductions + stores (emit_store).  k_emit issues the loads of ALL the family's records before the first store: a wavefront's
// life is a chain of memory round trips, and the records' round trips now run side by side instead of one after the other.
struct EmitLoads {
  EmitCtx X;
  uint2 cw; uint32_t qw, dw[2], ew[2], ao[2], so, qo, j3;
  uint8_t nb, rgb, mib, cbb, rxb;
  uint32_t cb_len, rx_len;
  bool has_cb, has_rx, generic;
};
__device__ __forceinline__ void emit_load(const EmitParams& P, const EndDesc& D, uint64_t out_off, uint32_t lane, EmitLoads& R) {
  // the descriptor's fields come out of LDS into vector registers; they are the same in every lane, and saying so (readfirstlane)
  // turns every address below into scalar base + 32-bit lane offset
  EmitCtx& X = R.X;
  X.q = P.out + (out_off - P.out_base);
  X.Lc = uni(D.cons_len);
  X.first = P.blob + uniform_u64(D.first_off);
  X.mi_len = uni(D.mi_len); X.mi_off = uni(D.mi_off);
  X.name_len = P.prefix_len + 1 + X.mi_len;
  X.rec_size = uni(D.rec_size);
  X.flag = bam::F_UNMAPPED;
  const uint32_t d_type = uni(D.type);
  if (d_type == 1) X.flag |= bam::F_PAIRED | bam::F_FIRST | bam::F_MATE_UNMAPPED;
  else if (d_type == 2) X.flag |= bam::F_PAIRED | bam::F_LAST | bam::F_MATE_UNMAPPED;
  const uint64_t col_off = uniform_u64(D.col_off);
  X.code = P.col_code + col_off; X.cq = P.col_qual + col_off; X.cd = P.col_depth + col_off; X.ce = P.col_err + col_off;
  const uint32_t Lc = X.Lc, name_len = X.name_len, mi_len = X.mi_len, mi_off = X.mi_off;
  R.has_cb = uni(D.has_cb) != 0; R.has_rx = uni(D.has_rx) != 0;
  R.cb_len = R.has_cb ? uni(D.cb_len) : 0; R.rx_len = R.has_rx ? uni(D.rx_len) : 0;
  R.generic = Lc > 192 || Lc < 8 || name_len + 1 > 64 || P.rg_len + 4 > 64 || R.cb_len + 4 > 64;
  if (R.generic) return;                                       // (any length: emit_generic, field after field)

  // Payloads move as (unaligned) dwords: lane l owns bytes [4l, 4l + 4) of a field, and the lane past the last whole dword
  // takes the field's LAST four bytes instead (an overlapping store of the same values) — no byte-granular tail.
  const uint32_t seq_bytes = (Lc + 1) / 2;
  R.so = min(4 * lane, seq_bytes - 4);                                                  // sequence: 4 output bytes = 8 columns
  R.qo = min(4 * lane, Lc - 4);                                                         // qualities: 4 columns
  R.cw = gld64u(X.code + 2 * R.so);                                                     // (column Lc may be read: one byte of slack)
  R.qw = gld32u(X.cq + R.qo);
#pragma unroll
  for (int t = 0; t < 2; t++) {                                                         // per-base arrays: 4 bytes = 2 columns
    R.ao[t] = min(4 * (lane + 64 * t), 2 * Lc - 4);
    R.dw[t] = gld32u((const uint8_t*)X.cd + R.ao[t]); R.ew[t] = gld32u((const uint8_t*)X.ce + R.ao[t]);
  }
  const uint32_t j3 = lane >= 3 ? lane - 3 : 0;
  R.j3 = j3;
  const uint32_t ni = lane > P.prefix_len ? lane - P.prefix_len - 1 : 0;
  const uint8_t pfx = (uint8_t)P.prefix[lane < P.prefix_len ? lane : 0];                       // d_strings keeps 16 bytes of slack
  const uint8_t nmb = X.first[mi_off + (ni < mi_len ? ni : mi_len)];                            // index mi_len is the tag's NUL
#if FGX_EMIT_FLAT
  {   // (nmb is the tag's NUL from lane name_len on: two one-level selects)
    const uint8_t colon_or_mi = lane == P.prefix_len ? (uint8_t)':' : nmb;
    R.nb = lane < P.prefix_len ? pfx : colon_or_mi;
  }
#else
  R.nb = lane < P.prefix_len ? pfx : lane == P.prefix_len ? (uint8_t)':' : lane < name_len ? nmb : (uint8_t)0;
#endif
  R.rgb = (uint8_t)P.rg[j3 < P.rg_len ? j3 : 0];
  R.mib = X.first[mi_off + (j3 < mi_len ? j3 : mi_len)];
  const uint8_t* fk = R.has_cb ? P.blob + uniform_u64(D.kept_off) + uni(D.cb_off) : X.first;
  R.cbb = fk[j3 < R.cb_len ? j3 : 0];
  R.rxb = (uint8_t)D.rx[j3 < FAST_RX_CAP ? j3 : 0];
}
__device__ __forceinline__ void emit_store(const EmitParams& P, const EndDesc& D, uint32_t lane, const EmitLoads& R) {
  const EmitCtx& X = R.X;
  if (R.generic) { emit_generic(P, D, X, lane); return; }
  const uint32_t Lc = X.Lc, name_len = X.name_len, mi_len = X.mi_len, seq_bytes = (Lc + 1) / 2, j3 = R.j3;
  const uint32_t so = R.so, qo = R.qo, cb_len = R.cb_len, rx_len = R.rx_len;
  const bool has_cb = R.has_cb, has_rx = R.has_rx;
  // ---- cD / cM / cE (vanilla_caller.rs:1800-1810): max / min depth, Σerrors / Σdepth as f32 ---------------------
  // every column counted once: a lane's low half is a duplicate when its offset was pulled back to the field's last dword
  uint32_t maxd = 0, mind = 0xFFFFFFFFu, sumd = 0, sume = 0;
#pragma unroll
  for (int t = 0; t < 2; t++) {
    const uint32_t nat = 4 * (lane + 64 * t);
    const bool in = nat < 2 * Lc, lo_own = in && nat == R.ao[t];
    const uint32_t dl = R.dw[t] & 0xFFFF, dh = R.dw[t] >> 16, el = R.ew[t] & 0xFFFF, eh = R.ew[t] >> 16;
    if (lo_own) { maxd = dl > maxd ? dl : maxd; mind = dl < mind ? dl : mind; sumd += dl; sume += el; }
    if (in) { maxd = dh > maxd ? dh : maxd; mind = dh < mind ? dh : mind; sumd += dh; sume += eh; }
  }
  maxd = wave_max(maxd); mind = wave_min(mind); sumd = wave_sum(sumd); sume = wave_sum(sume);
  maxd = uni(maxd); mind = uni(mind); sumd = uni(sumd); sume = uni(sume);   // (every lane holds the totals: the tag widths below, and with them every later address, are scalar)
  const float ce_rate = sumd > 0 ? (float)sume / (float)sumd : 0.0f;
  const uint32_t n_cd = 3 + int_tag_width(maxd), n_cm = 3 + int_tag_width(mind);

  // ---- stores -----------------------------------------------------------------------------------------------------------
  uint8_t* q = X.q;
#if FGX_EMIT_FLAT
  // The small fields are chains of "lane k holds byte k" choices over wave-uniform values.  Written as nested conditionals they compile into
  // nested exec-mask regions (the kernel executed more scalar instructions than vector ones: 611 against 530 per family); written as below
  // — uniform words built by the scalar unit, a lane's byte taken with one shift, one-level selects — they are straight-line code.
  const uint32_t l3 = lane < 3u ? lane : 3u, sh3 = 8u * l3;                             // (a 24-bit header word >> sh3: its byte for lanes 0 - 2, 0 from lane 3 on)
  auto ztag = [&](uint32_t c3, uint32_t len, uint32_t body) -> uint32_t {               // byte `lane` of the tag  XY:Z:<len bytes> NUL
    const uint32_t u = (lane - 3u < len) ? body : 0u;                                    // (unsigned: false for lanes 0 - 2)
    return (c3 >> sh3) | u;
  };
  {   // block_size + fixed core: ref_id -1, pos -1, l_read_name, mapq 0, bin 4680, n_cigar_op 0, flag, l_seq, next_ref -1, next_pos -1, tlen 0
    uint32_t v = 0xFFFFFFFFu;
    if (lane == 0) v = X.rec_size;
    if (lane == 3) v = (name_len + 1) | (4680u << 16);
    if (lane == 4) v = X.flag << 16;
    if (lane == 5) v = Lc;
    if (lane == 8) v = 0u;
    if (lane < 9) gst32u(q + 4 * lane, v);
  }
#else
  if (lane < 9) {   // block_size + fixed core: ref_id -1, pos -1, l_read_name, mapq 0, bin 4680, n_cigar_op 0, flag, l_seq, next_ref -1, next_pos -1, tlen 0
    const uint32_t v = lane == 0 ? X.rec_size : lane == 3 ? ((name_len + 1) | (4680u << 16)) : lane == 4 ? (X.flag << 16) : lane == 5 ? Lc : lane == 8 ? 0u : 0xFFFFFFFFu;
    gst32u(q + 4 * lane, v);
  }
#endif
  q += 36;
  if (lane < name_len + 1) q[lane] = R.nb;
  q += name_len + 1;
  if (4 * lane < seq_bytes) {   // eight columns → four bytes, high nibble first; a column past the end packs as 0
    const uint32_t c0 = 2 * so;
    uint32_t lo4 = R.cw.x, hi4 = R.cw.y;                                               // codes of columns c0..c0+3 / c0+4..c0+7, one byte each
    if (c0 + 7 >= Lc) hi4 &= 0x00FFFFFFu;                                              // (only column c0 + 7 can be past the end: Lc odd)
    const uint32_t b0 = ((lo4 << 4) | (lo4 >> 8)) & 0xFF, b1 = ((lo4 >> 12) | (lo4 >> 24)) & 0xFF;
    const uint32_t b2 = ((hi4 << 4) | (hi4 >> 8)) & 0xFF, b3 = ((hi4 >> 12) | (hi4 >> 24)) & 0xFF;
    gst32u(q + so, b0 | (b1 << 8) | (b2 << 16) | (b3 << 24));
  }
  q += seq_bytes;
  if (4 * lane < Lc) gst32u(q + qo, R.qw);
  q += Lc;
#if FGX_EMIT_FLAT
  {
    const uint32_t b = ztag('R' | ('G' << 8) | ('Z' << 16), P.rg_len, R.rgb);
    if (lane < 3 + P.rg_len + 1) q[lane] = (uint8_t)b;
  }
  q += 3 + P.rg_len + 1;
  {   // cD cM cE and, when asked for, the header of the cd array right behind them: one store.  Four uniform 64-bit words (an integer tag
      // is `ab` + its type + one or two value bytes, cE is `cEf` + the four bytes of the rate, the array header `cdBs` + its count)
    const uint32_t n3 = n_cd + n_cm + 7, nh = P.per_base_tags ? 8u : 0u;
    auto int_word = [](uint32_t a, uint32_t b, uint32_t v) -> unsigned long long {
      const uint32_t ty = v <= 127 ? (uint32_t)'c' : v <= 255 ? (uint32_t)'C' : (uint32_t)'S';
      return (unsigned long long)(a | (b << 8) | (ty << 16)) | ((unsigned long long)v << 24);
    };
    const unsigned long long w_cd = int_word('c', 'D', maxd), w_cm = int_word('c', 'M', mind);
    const unsigned long long w_ce = (unsigned long long)('c' | ('E' << 8) | ('f' << 16)) | ((unsigned long long)__float_as_uint(ce_rate) << 24);
    const unsigned long long w_hd = (unsigned long long)('c' | ('d' << 8) | ('B' << 16) | ('s' << 24)) | ((unsigned long long)Lc << 32);
    unsigned long long w = w_hd;
    uint32_t k = lane - n3;
    if (lane < n3) { w = w_ce; k = lane - n_cd - n_cm; }
    if (lane < n_cd + n_cm) { w = w_cm; k = lane - n_cd; }
    if (lane < n_cd) { w = w_cd; k = lane; }
    const uint32_t b = (uint32_t)(w >> (8u * (k & 7u)));
    if (lane < n3 + nh) q[lane] = (uint8_t)b;
    q += n3;
  }
#else
  if (lane < 3 + P.rg_len + 1) q[lane] = lane == 0 ? 'R' : lane == 1 ? 'G' : lane == 2 ? 'Z' : j3 < P.rg_len ? R.rgb : (uint8_t)0;
  q += 3 + P.rg_len + 1;
  {   // cD cM cE and, when asked for, the header of the cd array right behind them: one store
    const uint32_t n3 = n_cd + n_cm + 7, nh = P.per_base_tags ? 8u : 0u;
    if (lane < n3 + nh) {
      const uint32_t i = lane - n3;
      q[lane] = lane < n3 ? cdcmce_byte(lane, n_cd, n_cm, maxd, mind, ce_rate)
                          : (uint8_t)(i == 0 ? 'c' : i == 1 ? 'd' : i == 2 ? 'B' : i == 3 ? 's' : (Lc >> (8 * (i - 4))));
    }
    q += n3;
  }
#endif
  if (P.per_base_tags) {
    q += 8;
#pragma unroll
    for (int t = 0; t < 2; t++) if (4 * (lane + 64 * t) < 2 * Lc) gst32u(q + R.ao[t], R.dw[t]);
    q += 2 * Lc;
    if (lane < 2) gst32u(q + 4 * lane, lane == 0 ? ('c' | ('e' << 8) | ('B' << 16) | ('s' << 24)) : Lc);
    q += 8;
#pragma unroll
    for (int t = 0; t < 2; t++) if (4 * (lane + 64 * t) < 2 * Lc) gst32u(q + R.ao[t], R.ew[t]);
    q += 2 * Lc;
  }
#if FGX_EMIT_FLAT
  {
    const uint32_t b = ztag((uint32_t)(uint8_t)P.tag0 | ((uint32_t)(uint8_t)P.tag1 << 8) | ('Z' << 16), mi_len, R.mib);
    if (lane < 3 + mi_len + 1) q[lane] = (uint8_t)b;
  }
  q += 3 + mi_len + 1;
  if (has_cb) {
    const uint32_t b = ztag((uint32_t)(uint8_t)P.cell0 | ((uint32_t)(uint8_t)P.cell1 << 8) | ('Z' << 16), cb_len, R.cbb);
    if (lane < 3 + cb_len + 1) q[lane] = (uint8_t)b;
    q += 3 + cb_len + 1;
  }
  if (has_rx) {
    const uint32_t b = ztag('R' | ('X' << 8) | ('Z' << 16), rx_len, R.rxb);
    if (lane < 3 + rx_len + 1) q[lane] = (uint8_t)b;
  }
  (void)j3;
#else
  if (lane < 3 + mi_len + 1) q[lane] = lane == 0 ? (uint8_t)P.tag0 : lane == 1 ? (uint8_t)P.tag1 : lane == 2 ? 'Z' : j3 < mi_len ? R.mib : (uint8_t)0;
  q += 3 + mi_len + 1;
  if (has_cb) { if (lane < 3 + cb_len + 1) q[lane] = lane == 0 ? (uint8_t)P.cell0 : lane == 1 ? (uint8_t)P.cell1 : lane == 2 ? 'Z' : j3 < cb_len ? R.cbb : (uint8_t)0; q += 3 + cb_len + 1; }
  if (has_rx) { if (lane < 3 + rx_len + 1) q[lane] = lane == 0 ? 'R' : lane == 1 ? 'X' : lane == 2 ? 'Z' : j3 < rx_len ? R.rxb : (uint8_t)0; }
#endif
}

// ---- round 6: BOTH records of a pair family at once — record R1 in lanes 0 - 31, record R2 in lanes 32 - 63 -----------------------------------
// k_emit executed 450 vector + 357 scalar instructions per family for two records written one after the other (profiles/r05y_pmc_5M_families.json):
// most of them for the small fields (a store per field, a lane per byte, a dozen of 64 lanes busy) and for wave-uniform address arithmetic that is
// redone per record.  Here the two records share every instruction.  A lane takes EIGHT columns of its half's record — 8 B of codes -> 4 B of
// packed bases, 8 B of qualities, 16 B each of cd / ce: 19 lanes of a half for 150 columns, the group of the last lane pulled back so that it ends
// with the record (an overlapping store of the same values; its duplicate columns are masked out of the sums) —, the small fields are a lane per
// byte of the half's record, and every address is ONE scalar base (record R1, the scratch columns of R1) + a 32-bit lane offset: R2 follows R1
// in the output, and its columns follow R1's in the scratch.  cD / cM / cE: the four reductions stop at the half (five DPP steps).
// Taken when both records are there, 8 <= Lc <= 256 and every string field fits 32 lanes (emit_pair_takes, fastpath.h: k_split_finish asks the same
// function); returns false (nothing touched) otherwise.
// (round 7) fr_cnt != 0: k_call_full left this family's answers in slots [fr_first, fr_first + fr_cnt) of P.full_res instead of the scratch planes
// (fastpath.h, FullResult).  Lane j < fr_cnt loads result j with the column loads.  The lanes put their groups into the wavefront's 3 KB of `patch`
// (LDS, a lane's group at the lane's index: aligned), the lane of a result overwrites its column's code, quality, depth and errors there — in the
// lane whose group holds the column and, where the half's pulled-back last group holds it too, in that lane as well; the code groups start at cs,
// the others at c0 —, and every lane takes its groups back before the reductions.  One round trip through LDS whatever the number of results, and
// nothing on the vector ALU, which this kernel is short of: a broadcast loop costs ~40 vector instructions per result against the kernel's 394 per family.
constexpr uint32_t EMIT_PATCH_BYTES = 64u * (8u + 8u + 16u + 16u);
#ifndef FGX_EMIT_PAIR
#define FGX_EMIT_PAIR 1
#endif
typedef unsigned short em_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t em_pkmax(uint32_t a, uint32_t b) { em_u16x2 x, y; __builtin_memcpy(&x, &a, 4); __builtin_memcpy(&y, &b, 4); x = __builtin_elementwise_max(x, y); uint32_t r; __builtin_memcpy(&r, &x, 4); return r; }
__device__ __forceinline__ uint32_t em_pkmin(uint32_t a, uint32_t b) { em_u16x2 x, y; __builtin_memcpy(&x, &a, 4); __builtin_memcpy(&y, &b, 4); x = __builtin_elementwise_min(x, y); uint32_t r; __builtin_memcpy(&r, &x, 4); return r; }
__device__ __forceinline__ uint32_t em_sum2(uint32_t pair, uint32_t acc) { em_u16x2 x; const em_u16x2 one = {1, 1}; __builtin_memcpy(&x, &pair, 4); return __builtin_amdgcn_udot2(x, one, acc, false); }   // acc + both 16-bit halves
// reductions over each HALF of the wavefront: the four row-local steps of FGX_WAVE_REDUCE, then row_bcast:15 into rows 1 and 3 — lane 31 holds the
// result of lanes 0 - 31, lane 63 that of lanes 32 - 63
#define FGX_HALF_REDUCE(v, idn, OP) do { \
    v = OP(v, wave_dpp<0xB1, 0xF>(idn, v)); v = OP(v, wave_dpp<0x4E, 0xF>(idn, v)); v = OP(v, wave_dpp<0x141, 0xF>(idn, v)); v = OP(v, wave_dpp<0x140, 0xF>(idn, v)); \
    v = OP(v, wave_dpp<0x142, 0xA>(idn, v)); } while (0)
__device__ __forceinline__ bool emit_pair(const EmitParams& P, const EndDesc* D /* [3]: slots F, R1, R2 in LDS */, uint64_t oo1, uint64_t oo2, uint32_t lane,
                                          uint8_t* const patch, const uint32_t fr_first, const uint32_t fr_cnt) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const EndDesc& D1 = D[1];
  const EndDesc& D2 = D[2];
  const uint32_t Lc1 = uni(D1.cons_len), Lc2 = uni(D2.cons_len);
  const uint32_t mi_len = uni(D1.mi_len), mi_off = uni(D1.mi_off);
  const uint64_t first_off = uniform_u64(D1.first_off);
  const uint64_t col1 = uniform_u64(D1.col_off), col2 = uniform_u64(D2.col_off);
  const bool hcb1 = uni(D1.has_cb) != 0, hcb2 = uni(D2.has_cb) != 0, hrx1 = uni(D1.has_rx) != 0, hrx2 = uni(D2.has_rx) != 0;
  const uint32_t cbl1 = hcb1 ? uni(D1.cb_len) : 0u, cbl2 = hcb2 ? uni(D2.cb_len) : 0u, rxl1 = hrx1 ? uni(D1.rx_len) : 0u, rxl2 = hrx2 ? uni(D2.rx_len) : 0u;
  const uint32_t name_len = P.prefix_len + 1u + mi_len, rg_len = P.rg_len;
  const bool ok = emit_pair_takes(Lc1, Lc2, name_len, rg_len, mi_len, cbl1, cbl2, rxl1, rxl2,
                                  uniform_u64(D2.first_off) == first_off && uni(D2.mi_len) == mi_len && uni(D2.mi_off) == mi_off, col2 - col1, oo2 - oo1);
  if (!ok) return false;
  const uint32_t l = lane & 31u;
  const bool hb = lane >= 32u;
  const uint32_t Lc = hb ? Lc2 : Lc1;
  const uint32_t dcol = hb ? (uint32_t)(col2 - col1) : 0u, dq = hb ? (uint32_t)(oo2 - oo1) : 0u;
  const uint32_t ty1 = uni(D1.type), ty2 = uni(D2.type), rs1 = uni(D1.rec_size), rs2 = uni(D2.rec_size);   // (uniform reads by every lane, then the half's pick)
  const uint32_t d_type = hb ? ty2 : ty1, rec_size = hb ? rs2 : rs1;
  const bool hcb = hb ? hcb2 : hcb1, hrx = hb ? hrx2 : hrx1;
  const uint32_t cb_len = hb ? cbl2 : cbl1, rx_len = hb ? rxl2 : rxl1;
  // ---- loads: everything the two records read, before the first store ---------------------------------------------------------------------
  const uint32_t n0 = 8u * l;
  const bool pay = n0 < Lc;                                                             // this lane holds columns of its record
  const uint32_t c0 = min(n0, Lc - 8u);                                                 // first column of the lane's group (the last group is pulled back)
  const uint32_t cs = min(n0, ((Lc + 1u) & ~1u) - 8u);                                  // ... of its group of packed bases: even (column Lc may be read: slack)
  const uint8_t* const code = P.col_code + col1;
  const uint8_t* const cq = P.col_qual + col1;
  const uint8_t* const cdb = (const uint8_t*)(P.col_depth + col1);
  const uint8_t* const ceb = (const uint8_t*)(P.col_err + col1);
  uint2 cw = gld64u(code + (dcol + cs));
  uint2 qw = gld64u(cq + (dcol + c0));
  u32x4 dv, ev;
  __builtin_memcpy(&dv, cdb + 2u * (dcol + c0), 16);
  __builtin_memcpy(&ev, ceb + 2u * (dcol + c0), 16);
  FullResult fr;
  fr.w0 = FULL_RESULT_NONE << 16; fr.w1 = 0u;
  if (fr_cnt != 0u && lane < fr_cnt) { const uint2 v = *(const uint2*)(P.full_res + ((size_t)fr_first + lane)); fr.w0 = v.x; fr.w1 = v.y; }
  const uint8_t* const first = P.blob + first_off;
  const uint32_t j3 = l >= 3u ? l - 3u : 0u;
  const uint32_t ni = l > P.prefix_len ? l - P.prefix_len - 1u : 0u;
  const uint8_t pfx = (uint8_t)P.prefix[l < P.prefix_len ? l : 0u];                     // d_strings keeps 16 bytes of slack
  const uint8_t nmb = first[mi_off + (ni < mi_len ? ni : mi_len)];                      // index mi_len is the tag's NUL
  const uint8_t rgb = (uint8_t)P.rg[j3 < rg_len ? j3 : 0u];
  const uint8_t mib = first[mi_off + (j3 < mi_len ? j3 : mi_len)];
  uint8_t cbb = 0;
  if (hcb1 || hcb2) {                                                                   // (wave-uniform; the half without the tag reads byte 0 of the family's first record)
    const uint64_t k1 = hcb1 ? uniform_u64(D1.kept_off) + uni(D1.cb_off) : first_off, k2 = hcb2 ? uniform_u64(D2.kept_off) + uni(D2.cb_off) : first_off;
    const uint8_t* const fk = P.blob + (hb ? k2 : k1);
    cbb = fk[j3 < cb_len ? j3 : 0u];
  }
  const uint8_t rxb = (uint8_t)D[hb ? 2 : 1].rx[j3 < (uint32_t)FAST_RX_CAP ? j3 : 0u];
  // ---- k_call_full's answers for this family (wave-uniform: a family without items pays this branch) ---------------------------------------
  if (fr_cnt != 0u) {
    uint8_t* const pc = patch, * const pq = patch + 512u, * const pd = patch + 1024u, * const pe = patch + 2048u;
    __builtin_memcpy(pc + 8u * lane, &cw, 8); __builtin_memcpy(pq + 8u * lane, &qw, 8);
    __builtin_memcpy(pd + 16u * lane, &dv, 16); __builtin_memcpy(pe + 16u * lane, &ev, 16);
    wave_sync();
    const uint32_t r_code = (fr.w0 >> 16) & 0xFFu;
    if (r_code != FULL_RESULT_NONE) {
      const uint32_t d2 = (uint32_t)(col2 - col1);
      const uint32_t rel = ((fr.w0 & 0xFFFFu) - (uint32_t)col1) & 0xFFFFu;                // the column, counted from R1's first
      const bool h2 = rel >= d2 && rel - d2 < Lc2;                                      // (R1's columns end before R2's begin)
      const uint32_t rh = h2 ? rel - d2 : rel, Lh = h2 ? Lc2 : Lc1, Le = (Lh + 1u) & ~1u, l0 = h2 ? 32u : 0u;
      if (rh < Lh) {
        const uint32_t la = rh >> 3, ll = (Lh - 1u) >> 3;                                 // the lane of the column's natural group; the half's last lane with columns
        const uint32_t ga = min(8u * la, Lh - 8u), gl = min(8u * ll, Lh - 8u);            // first column of their groups (c0)
        const uint32_t ea = min(8u * la, Le - 8u), el = min(8u * ll, Le - 8u);            // ... of their groups of codes (cs)
        const uint8_t r_q = (uint8_t)(fr.w0 >> 24);
        const uint16_t r_e = (uint16_t)(fr.w1 & 0xFFFFu), r_d = (uint16_t)(fr.w1 >> 16);
        pc[8u * (l0 + la) + (rh - ea)] = (uint8_t)r_code;
        pq[8u * (l0 + la) + (rh - ga)] = r_q;
        __builtin_memcpy(pd + 16u * (l0 + la) + 2u * (rh - ga), &r_d, 2);
        __builtin_memcpy(pe + 16u * (l0 + la) + 2u * (rh - ga), &r_e, 2);
        if (la != ll && rh >= el) pc[8u * (l0 + ll) + (rh - el)] = (uint8_t)r_code;
        if (la != ll && rh >= gl) {
          pq[8u * (l0 + ll) + (rh - gl)] = r_q;
          __builtin_memcpy(pd + 16u * (l0 + ll) + 2u * (rh - gl), &r_d, 2);
          __builtin_memcpy(pe + 16u * (l0 + ll) + 2u * (rh - gl), &r_e, 2);
        }
      }
    }
    wave_sync();
    __builtin_memcpy(&cw, pc + 8u * lane, 8); __builtin_memcpy(&qw, pq + 8u * lane, 8);
    __builtin_memcpy(&dv, pd + 16u * lane, 16); __builtin_memcpy(&ev, pe + 16u * lane, 16);
  }
  // ---- cD / cM / cE (vanilla_caller.rs:1800-1810): max / min depth, sum of errors / sum of depths as f32, per half -------------------------
  uint32_t maxd, mind, sumd = 0, sume = 0;
  {
    const uint32_t skip16 = 16u * (n0 - c0);                                            // bits of duplicate columns at the low end of a pulled-back group
    const uint32_t d4[4] = {dv.x, dv.y, dv.z, dv.w}, e4[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int32_t sb = (int32_t)skip16 - 32 * k;
      const uint32_t m = sb <= 0 ? 0xFFFFFFFFu : sb == 16 ? 0xFFFF0000u : 0u;
      sumd = em_sum2(d4[k] & m, sumd); sume = em_sum2(e4[k] & m, sume);
    }
    const uint32_t mx = em_pkmax(em_pkmax(d4[0], d4[1]), em_pkmax(d4[2], d4[3])), mn = em_pkmin(em_pkmin(d4[0], d4[1]), em_pkmin(d4[2], d4[3]));   // (duplicates do not move a maximum)
    maxd = max(mx & 0xFFFFu, mx >> 16); mind = min(mn & 0xFFFFu, mn >> 16);
    if (!pay) { maxd = 0u; mind = 0xFFFFFFFFu; sumd = 0u; sume = 0u; }
  }
  FGX_HALF_REDUCE(maxd, 0u, wr_max); FGX_HALF_REDUCE(mind, 0xFFFFFFFFu, wr_min); FGX_HALF_REDUCE(sumd, 0u, wr_add); FGX_HALF_REDUCE(sume, 0u, wr_add);
  {   // (lane 31 / lane 63 hold the halves' results; every lane reads both)
    const uint32_t mx0 = rlane(maxd, 31), mx1 = rlane(maxd, 63), mn0 = rlane(mind, 31), mn1 = rlane(mind, 63);
    const uint32_t sd0 = rlane(sumd, 31), sd1 = rlane(sumd, 63), se0 = rlane(sume, 31), se1 = rlane(sume, 63);
    maxd = hb ? mx1 : mx0; mind = hb ? mn1 : mn0; sumd = hb ? sd1 : sd0; sume = hb ? se1 : se0;
  }
  const float ce_rate = sumd > 0u ? (float)sume / (float)sumd : 0.0f;
  const uint32_t n_cd = 3u + int_tag_width(maxd), n_cm = 3u + int_tag_width(mind);
  // ---- where the fields of the half's record lie (offsets from record R1's first byte) ----------------------------------------------------
  const uint32_t seq_bytes = (Lc + 1u) >> 1;
  const uint32_t o_seq = dq + 36u + name_len + 1u, o_qual = o_seq + seq_bytes, o_rg = o_qual + Lc, o_t3 = o_rg + 3u + rg_len + 1u;
  const uint32_t n3 = n_cd + n_cm + 7u, nh = P.per_base_tags ? 8u : 0u;
  const uint32_t o_cd = o_t3 + n3 + 8u, o_ceh = o_cd + 2u * Lc, o_ce = o_ceh + 8u;
  const uint32_t o_mi = P.per_base_tags ? o_ce + 2u * Lc : o_t3 + n3;
  const uint32_t o_cb = o_mi + 3u + mi_len + 1u, o_rx = o_cb + (hcb ? 3u + cb_len + 1u : 0u);
  uint8_t* const q = P.out + (oo1 - P.out_base);
  const uint32_t l3 = l < 3u ? l : 3u, sh3 = 8u * l3;                                   // (a 24-bit header word >> sh3: its byte for lanes 0 - 2 of the half, 0 from lane 3 on)
  auto ztag = [&](uint32_t c3, uint32_t len, uint32_t body) -> uint32_t { const uint32_t u = (l - 3u < len) ? body : 0u; return (c3 >> sh3) | u; };   // byte l of  XY:Z:<len bytes> NUL
  // ---- stores ---------------------------------------------------------------------------------------------------------------------------------
  {   // block_size + fixed core: ref_id -1, pos -1, l_read_name, mapq 0, bin 4680, n_cigar_op 0, flag, l_seq, next_ref -1, next_pos -1, tlen 0
    uint32_t flag = bam::F_UNMAPPED;
    if (d_type == 1u) flag |= bam::F_PAIRED | bam::F_FIRST | bam::F_MATE_UNMAPPED;
    else if (d_type == 2u) flag |= bam::F_PAIRED | bam::F_LAST | bam::F_MATE_UNMAPPED;
    uint32_t v = 0xFFFFFFFFu;
    if (l == 0u) v = rec_size;
    if (l == 3u) v = (name_len + 1u) | (4680u << 16);
    if (l == 4u) v = flag << 16;
    if (l == 5u) v = Lc;
    if (l == 8u) v = 0u;
    if (l < 9u) gst32u(q + (dq + 4u * l), v);
  }
  if (l < name_len + 1u) {
    const uint8_t colon_or_mi = l == P.prefix_len ? (uint8_t)':' : nmb;                 // (nmb is the tag's NUL from lane name_len on)
    q[dq + 36u + l] = l < P.prefix_len ? pfx : colon_or_mi;
  }
  if (pay) {
    // eight columns -> four bytes, high nibble first; a column past the end packs as 0 (only column cs + 7 can be: Lc odd)
    uint32_t lo4 = cw.x, hi4 = cw.y;
    if (cs + 7u >= Lc) hi4 &= 0x00FFFFFFu;
    const uint32_t t = (lo4 << 4) | (lo4 >> 8), u = (hi4 << 4) | (hi4 >> 8);            // bytes 0 and 2: (code << 4) | next code
    gst32u(q + (o_seq + (cs >> 1)), __builtin_amdgcn_perm(u, t, 0x06040200u));
    __builtin_memcpy(q + (o_qual + c0), &qw, 8);
  }
  {
    const uint32_t b = ztag('R' | ('G' << 8) | ('Z' << 16), rg_len, rgb);
    if (l < 3u + rg_len + 1u) q[o_rg + l] = (uint8_t)b;
  }
  {   // cD cM cE and, when asked for, the header of the cd array right behind them: one store
    auto int_word = [](uint32_t a, uint32_t b, uint32_t v) -> unsigned long long {
      const uint32_t ty = v <= 127u ? (uint32_t)'c' : v <= 255u ? (uint32_t)'C' : (uint32_t)'S';
      return (unsigned long long)(a | (b << 8) | (ty << 16)) | ((unsigned long long)v << 24);
    };
    const unsigned long long w_cd = int_word('c', 'D', maxd), w_cm = int_word('c', 'M', mind);
    const unsigned long long w_ce = (unsigned long long)('c' | ('E' << 8) | ('f' << 16)) | ((unsigned long long)__float_as_uint(ce_rate) << 24);
    const unsigned long long w_hd = (unsigned long long)('c' | ('d' << 8) | ('B' << 16) | ('s' << 24)) | ((unsigned long long)Lc << 32);
    unsigned long long w = w_hd;
    uint32_t k = l - n3;
    if (l < n3) { w = w_ce; k = l - n_cd - n_cm; }
    if (l < n_cd + n_cm) { w = w_cm; k = l - n_cd; }
    if (l < n_cd) { w = w_cd; k = l; }
    const uint32_t b = (uint32_t)(w >> (8u * (k & 7u)));
    if (l < n3 + nh) q[o_t3 + l] = (uint8_t)b;
  }
  if (P.per_base_tags) {
    if (pay) __builtin_memcpy(q + (o_cd + 2u * c0), &dv, 16);
    if (l < 2u) gst32u(q + (o_ceh + 4u * l), l == 0u ? ('c' | ('e' << 8) | ('B' << 16) | ('s' << 24)) : Lc);
    if (pay) __builtin_memcpy(q + (o_ce + 2u * c0), &ev, 16);
  }
  {
    const uint32_t b = ztag((uint32_t)(uint8_t)P.tag0 | ((uint32_t)(uint8_t)P.tag1 << 8) | ('Z' << 16), mi_len, mib);
    if (l < 3u + mi_len + 1u) q[o_mi + l] = (uint8_t)b;
  }
  if (hcb1 || hcb2) {
    const uint32_t b = ztag((uint32_t)(uint8_t)P.cell0 | ((uint32_t)(uint8_t)P.cell1 << 8) | ('Z' << 16), cb_len, cbb);
    if (hcb && l < 3u + cb_len + 1u) q[o_cb + l] = (uint8_t)b;
  }
  if (hrx1 || hrx2) {
    const uint32_t b = ztag('R' | ('X' << 8) | ('Z' << 16), rx_len, rxb);
    if (hrx && l < 3u + rx_len + 1u) q[o_rx + l] = (uint8_t)b;
  }
  return true;
}
#ifndef FGX_EMIT_OCC
#define FGX_EMIT_OCC 7   /* wavefronts per SIMD the register allocation of k_emit aims at */
#endif
// One wavefront per FAMILY: its (up to three) records.  A third of the slots is empty on paired data (the fragment slot), and a
// wavefront that only finds `valid == 0` still costs a launch and a memory round trip; the descriptor carries blob OFFSETS, so the
// record's strings are one dependent load away instead of two.
// (Assembling the record through LDS — whole-record image with byte writes, or dword-staged column arrays with dword payload
// copies — was measured three times, rounds 1 and 2: 3.4 – 4.0 ms against 2.2 ms per 2 M records; registers-only streaming it is.)
__global__ __launch_bounds__(256, FGX_EMIT_OCC) void k_emit(EmitParams P) {
  // the family's (up to) three descriptors, copied once with 16-byte loads: every field read below is an LDS read — as global
  // loads, the valid flags and then each record's fields were dependent memory round trips of their own
  __shared__ __align__(16) EndDesc sD[4][3];
  static_assert(sizeof(EndDesc) == 96, "EndDesc is copied as six 16-byte pieces");
#if FGX_EMIT_PAIR
  __shared__ __align__(16) uint8_t sPatch[4][EMIT_PATCH_BYTES];   // emit_pair: where k_call_full's answers meet the family's columns
#endif
  uint32_t fam = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  const uint32_t lane = threadIdx.x & 63, wv = (threadIdx.x >> 6) & 3;
  if (P.fam_list) {   // the merge of a direct-records batch: only the families that left the split pipeline have descriptors
    if (fam >= P.n_fam) return;
    fam = (uint32_t)__builtin_amdgcn_readfirstlane((int)P.fam_list[fam]);
  }
  const uint32_t s0 = P.slot0 + 3 * fam;
  if (s0 >= P.slot_end) return;
  // (every kernel argument the records need is asked for here, in one batch: fetched where first used they were five separate
  // scalar-load round trips along the way)
#if defined(FGX_WAVEMU)
#define K_EMIT_PIN(x) ((void)(x))
#else
#define K_EMIT_PIN(x) asm volatile("" :: "s"(x))
#endif
  K_EMIT_PIN(P.blob); K_EMIT_PIN(P.out); K_EMIT_PIN(P.out_base); K_EMIT_PIN(P.col_code); K_EMIT_PIN(P.col_qual); K_EMIT_PIN(P.col_depth);
  K_EMIT_PIN(P.col_err); K_EMIT_PIN(P.prefix); K_EMIT_PIN(P.prefix_len); K_EMIT_PIN(P.rg); K_EMIT_PIN(P.rg_len);
#undef K_EMIT_PIN
  const uint32_t ns = P.slot_end - s0 < 3 ? P.slot_end - s0 : 3;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4 piece = ((const u32x4*)&P.ends[s0])[lane < 6 * ns ? lane : 0u];
  const uint64_t oo = P.out_off[s0 + (lane < ns ? lane : 0u)];   // (both loads leave before either is waited for)
#if FGX_EMIT_PAIR
  const uint32_t fr_flag = (P.full_flag && !P.fam_list) ? (uint32_t)P.full_flag[fam] : 0u;   // ... and this one: does the pair writer apply k_call_full's answers for the family?
#endif
  if (lane < 6 * ns) ((u32x4*)&sD[wv][0])[lane] = piece;
  wave_sync();
  const bool v0 = uni(sD[wv][0].valid) != 0, v1 = ns > 1 && uni(sD[wv][1].valid) != 0, v2 = ns > 2 && uni(sD[wv][2].valid) != 0;
  // (the record's output offset as a SCALAR: with it in a vector register every store of the record formed a 64-bit vector
  // address of its own — a third of the kernel's vector instructions were address adds and register moves)
  auto off_of = [&](int k) -> uint64_t {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(oo >> 32), k) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)oo, k);
  };
  if (v0) { EmitLoads R0; emit_load(P, sD[wv][0], off_of(0), lane, R0); emit_store(P, sD[wv][0], lane, R0); }   // a fragment record: families of single reads
#if FGX_EMIT_PAIR
  {
    // the family's range of results: the word the packed build left in the fragment slot's descriptor (fastpath.h: full_range_word)
    const uint64_t fr_word = uniform_u64(sD[wv][0].col_off);
    const uint32_t fr_cnt = uni(fr_flag) ? (uint32_t)(fr_word >> 32) & 0xFFFFu : 0u;
    if (!v0 && v1 && v2 && emit_pair(P, &sD[wv][0], off_of(1), off_of(2), lane, &sPatch[wv][0], (uint32_t)fr_word, fr_cnt <= FULL_RESULT_MAX_ITEMS ? fr_cnt : 0u)) return;
  }   // (round 6) the usual pair family: both records side by side in the halves of the wavefront
#endif
  // the two records of a pair family: both records' loads, then both records' stores
  EmitLoads R1, R2;
  if (v1) emit_load(P, sD[wv][1], off_of(1), lane, R1);
  if (v2) emit_load(P, sD[wv][2], off_of(2), lane, R2);
  if (v1) emit_store(P, sD[wv][1], lane, R1);
  if (v2) emit_store(P, sD[wv][2], lane, R2);
}

// -----------------------------------------------------------------------------------------------------
// k_emit_duplex — one wavefront per duplex consensus record: the A/B strand combine of duplex_consensus
// (duplex_caller.rs:931-1108) over the two single-strand column segments, then the record of duplex_read_into
// (:1118-1405): tags MI [CB] RG aD aE aM [ac ad ae aq] bD bE bM [bc bd be bq] cD cE cM RX.
// -----------------------------------------------------------------------------------------------------
// records the fast writers (k_emit_duplex_fast / k_emit_codec_fast, below) take; the per-field kernels skip them
constexpr uint32_t DUP_SLOTS = 2;     // duplex: up to 256 positions

__device__ __forceinline__ bool small_tags(uint32_t name_len, uint32_t mi_len, uint32_t cb_len, uint32_t rg_len, uint32_t rx_len) {
  return name_len + 1 <= 64 && mi_len + 4 <= 64 && cb_len + 4 <= 64 && rg_len + 4 <= 64 && rx_len + 4 <= 64;
}
__device__ __forceinline__ bool fast_ok(const DuplexDesc& D, uint32_t prefix_len, uint32_t rg_len) {
  return D.len <= 128 * DUP_SLOTS && small_tags(prefix_len + 1 + D.mi_len, D.mi_len, D.has_cb ? D.cb_len : 0, rg_len, D.has_rx ? D.rx_len : 0);
}
__device__ __forceinline__ bool fast_ok(const CodecDesc& D, uint32_t prefix_len, uint32_t rg_len) {
  return small_tags(prefix_len + 1 + D.mi_len, D.mi_len, D.has_cb ? D.cb_len : 0, rg_len, D.has_rx ? D.rx_len : 0);     // any length: written in windows of 256 positions
}

__device__ __forceinline__ uint32_t obs_sum(uint32_t o) { return (o & 0xFF) + ((o >> 8) & 0xFF) + ((o >> 16) & 0xFF) + (o >> 24); }
__device__ __forceinline__ uint32_t obs_of_code(uint32_t o, uint32_t code) {   // count of the base with 4-bit code 1/2/4/8
  return code == 1 ? (o & 0xFF) : code == 2 ? ((o >> 8) & 0xFF) : code == 4 ? ((o >> 16) & 0xFF) : code == 8 ? (o >> 24) : 0u;
}
__device__ __forceinline__ uint32_t cap_q(int32_t v) { return v < 2 ? 2u : v > 93 ? 93u : (uint32_t)v; }
// The raw duplex call of one position from the two single-strand calls (duplex_consensus, duplex_caller.rs:979-1020), bases as 4-bit codes.
// METH 1, the methylation-aware mode's conversion-artifact rule (:988-1005): a C / T or G / A disagreement at a column that either strand's
// annotation flags as a reference cytosine (`ref_c`) is a conversion event — the unconverted base, the qualities added, and no error counted
// (`artifact`).
template <int METH>
__device__ __forceinline__ void duplex_combine(uint32_t ca, uint32_t qa, uint32_t cb, uint32_t qb, bool ref_c, uint32_t& rb, uint32_t& rq, bool& artifact) {
  artifact = false;
  if constexpr (METH != 0) {
    const uint32_t both = ca | cb;                                    // {C, T} = 2 | 8, {G, A} = 4 | 1 (an N, 15, makes neither)
    artifact = ref_c && ca != cb && (both == 10u || both == 5u);
    if (artifact) { rb = both == 10u ? 2u : 4u; rq = cap_q((int32_t)qa + (int32_t)qb); return; }
  }
  if (ca == cb) { rb = ca; rq = cap_q((int32_t)qa + (int32_t)qb); }
  else if (qa > qb) { rb = ca; rq = cap_q((int32_t)qa - (int32_t)qb); }
  else if (qb > qa) { rb = cb; rq = cap_q((int32_t)qb - (int32_t)qa); }
  else { rb = ca; rq = FGX_MIN_PHRED; }
}
// The duplex call of a position where both strands have a call: the raw call (`rb`, `artifact`), and what the record shows (`oc`, `oq`) — no call
// where either strand has none or the raw quality is the minimum.  The record writers (through duplex_column) and the methylation tag kernels of
// duplex_meth.inc (MM is built from the duplex bases) share it.
struct DCall { uint32_t rb, oc, oq; bool artifact; };
template <int METH>
__device__ __forceinline__ DCall duplex_call(uint32_t ca, uint32_t qa, uint32_t cb, uint32_t qb, bool ref_c) {
  DCall r;
  uint32_t rq;
  duplex_combine<METH>(ca, qa, cb, qb, ref_c, r.rb, rq, r.artifact);
  const bool nocall = ca == 15 || cb == 15 || rq == FGX_MIN_PHRED;
  r.oc = nocall ? 15u : r.rb; r.oq = nocall ? (uint32_t)FGX_MIN_PHRED : rq;
  return r;
}
// The errors of a position with a duplex call: source reads of both strands that disagree with the raw duplex base (N never counts; a conversion event is
// no error), out of the observation counts `xa` / `xb` — the scoring reads' (col_obs), or every source read's (col_obs_all) for a record a per-strand cap
// bit — and their `total`.
__device__ __forceinline__ uint32_t duplex_errors(const DCall& d, uint32_t total, uint32_t xa, uint32_t xb) {
  return (d.rb == 15 || d.artifact) ? 0u : total - (obs_of_code(xa, d.rb) + obs_of_code(xb, d.rb));
}
// One position of a duplex record from values in registers: strand A's call (base code, quality, errors, the observation counts of the scoring reads:
// depth), strand B's likewise where the record has one (`has_ba`; its fields read as no call, depth 0 otherwise), the duplex call and its errors out of
// `xa` / `xb`.  (k_emit_duplex_fast spells the has_ba arm out around the same duplex_call / duplex_errors: through this function its builds <0>, <1>,
// <0, 1> came out at 71 / 71 / 74 VGPRs and 67 SGPRs against 71 / 73 / 74 and 68 — no worse, but its form stays the one its speed was measured with,
// profiles/record_writers_refactor.md.)
struct DCol { uint32_t ca, qa, ea, da, cb, qb, eb, db, oc, oq, oe; };
template <int METH>
__device__ __forceinline__ DCol duplex_column(uint32_t ca, uint32_t qa, uint32_t ea, uint32_t oa, bool has_ba, uint32_t cb, uint32_t qb, uint32_t eb, uint32_t ob,
                                              uint32_t xa, uint32_t xb, bool ref_c) {
  DCol c;
  c.ca = ca; c.qa = qa; c.ea = ea; c.da = obs_sum(oa);
  c.cb = 15; c.qb = 0; c.eb = 0; c.db = 0; c.oc = ca; c.oq = qa; c.oe = ea;
  if (has_ba) {
    c.cb = cb; c.qb = qb; c.eb = eb; c.db = obs_sum(ob);
    const DCall d = duplex_call<METH>(ca, qa, cb, qb, ref_c);
    c.oc = d.oc; c.oq = d.oq;
    c.oe = duplex_errors(d, obs_sum(xa) + obs_sum(xb), xa, xb);
  }
  return c;
}

// CAP 1: the writers of a caller with --max-reads-per-strand — a record with DuplexDesc::capped takes the counts of the error recount (cE / ce) from
// col_obs_all (every source read); depths (aD bD cD, ad bd) stay col_obs's (the scoring reads).  CAP 0: the writers without any of it.
template <int METH, int CAP = 0>     // METH 1: the methylation-aware mode (the conversion-artifact rule in the strand combine)
__global__ __launch_bounds__(256) void k_emit_duplex(DuplexEmitParams P) {
  const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)(P.slot0 + ((blockIdx.x * blockDim.x + threadIdx.x) >> 6)));
  const uint32_t lane = threadIdx.x & 63;
  if (slot >= P.slot_end) return;
  const DuplexDesc& D = P.ends[slot];
  if (!D.valid || fast_ok(D, P.prefix_len, P.rg_len)) return;     // k_emit_duplex_fast writes those
  const uint32_t L = D.len;
  const bool has_ba = D.has_ba != 0;
  const uint64_t a_off = D.a_off, b_off = D.b_off;
  const uint8_t* mi = P.blob + P.rec_off[D.first_rec] + D.mi_off;
  const uint32_t mi_len = D.mi_len, name_len = P.prefix_len + 1 + mi_len;
  const uint32_t flag = bam::F_UNMAPPED | bam::F_PAIRED | bam::F_MATE_UNMAPPED | (D.type == 1 ? bam::F_FIRST : bam::F_LAST);
  // one position of the record: both strands' single-strand calls and the duplex call
  auto col = [&](uint32_t i) {
    const uint64_t ia = a_off + i, ib = b_off + i;
    const uint32_t oa = P.col_obs[ia];
    uint32_t cb = 15, qb = 0, eb = 0, ob = 0, xa = oa, xb = 0;
    bool ref_c = false;
    if (has_ba) {
      cb = P.col_code[ib]; qb = P.col_qual[ib]; eb = P.col_err[ib]; ob = P.col_obs[ib]; xb = ob;
      if constexpr (METH != 0) ref_c = (P.meth_flag[ia] | P.meth_flag[ib]) != 0;
      if constexpr (CAP != 0) { if (D.capped) { xa = P.col_obs_all[ia]; xb = P.col_obs_all[ib]; } }
    }
    return duplex_column<METH>(P.col_code[ia], P.col_qual[ia], P.col_err[ia], oa, has_ba, cb, qb, eb, ob, xa, xb, ref_c);
  };
  // ---- reductions for aD aM aE / bD bM bE / cD cM cE -------------------------------------------------------------------------
  StrandStats A, B, AB;
  for (uint32_t i = lane; i < L; i += 64) { const DCol c = col(i); A.add(c.da, c.ea); B.add(c.db, c.eb); AB.add(c.da + c.db, c.oe); }
  reduce_stats(A, B, AB, L);
  // ---- the record: block_size + core, name, bases, quals, then the tags in the reference's order ------------------------------------
  FieldWriterNested W{P.out + P.out_off[slot], lane};
  auto strand = [&](char s, const StrandStats& T, bool per_base, bool b_side) {   // <s>D <s>E <s>M, and a strand's per-base tags: bases, depths, errors, quals
    W.scalars(s, false, T.dmax, T.dmin, T.rate());
    if (!per_base) return;
    W.string_any(s, 'c', L, [&](uint32_t i) { const DCol c = col(i); return bam::code_to_ascii((uint8_t)(b_side ? c.cb : c.ca)); });
    W.i16_any(s, 'd', L, [&](uint32_t i) { const DCol c = col(i); return b_side ? c.db : c.da; });
    W.i16_any(s, 'e', L, [&](uint32_t i) { const DCol c = col(i); return b_side ? c.eb : c.ea; });
    W.string_any(s, 'q', L, [&](uint32_t i) { const DCol c = col(i); const uint32_t qq = (b_side ? c.qb : c.qa) + 33; return qq > 255 ? 255u : qq; });
  };
  W.core(D.rec_size, name_len, flag, L);
  W.name(P.prefix, P.prefix_len, mi, name_len);
  W.seq_qual_any(L, [&](uint32_t i) { return col(i).oc; }, [&](uint32_t i) { return col(i).oq; });
  W.z_any('M', 'I', mi, mi_len);
  if (D.has_cb) W.z_any(P.cell0, P.cell1, P.blob + P.rec_off[D.cb_rec] + D.cb_off, D.cb_len);
  W.z_any('R', 'G', (const uint8_t*)P.rg, P.rg_len);
  strand('a', A, P.per_base_tags, false);
  strand('b', B, P.per_base_tags && has_ba, true);
  strand('c', AB, false, false);
  if (D.has_rx) W.z_any('R', 'X', (const uint8_t*)D.rx, D.rx_len);
}

// -----------------------------------------------------------------------------------------------------
// k_emit_codec — one wavefront per CODEC molecule: orient and pad the two single-strand consensi
// (codec_caller.rs:955-968, 1272-1314), combine them position by position (:1331-1512), apply the quality
// masks (:1526-1561), turn the result into R1's orientation and write the fragment record (:1590-1757):
// tags RG MI cD cM cE aD aM aE bD bM bE [ad bd ae be ac bc aq bq] [CB] RX.
// -----------------------------------------------------------------------------------------------------
// Strand geometry of a CODEC molecule in reference orientation.  Both strands are brought to reference orientation (the reverse strand's consensus
// reverse-complemented), the negative-strand one right-aligned by padding on the left, combined, and the whole thing reverse-complemented again when R1
// is the negative strand: strand 1 is reverse-complemented and right-aligned when R1 is the negative read, strand 2 is reverse-complemented when R1 is
// NOT negative and right-aligned when R2 is.
struct CodecGeom {
  uint32_t C, l1, l2, sh1, sh2, neg;     // neg: CodecDesc::flags (kept as the word it is: with bool members k_emit_codec_fast took two more registers, 79 -> 81)
  __device__ __forceinline__ CodecGeom(const CodecDesc& D) : C(D.cons_len), l1(D.l1), l2(D.l2), neg(D.flags) {
    sh1 = (neg & 1) ? C - l1 : 0; sh2 = (neg & 2) ? C - l2 : 0;
  }
  __device__ __forceinline__ bool r1_neg() const { return (neg & 1) != 0; }
  __device__ __forceinline__ bool rc1() const { return r1_neg(); }
  __device__ __forceinline__ bool rc2() const { return !r1_neg(); }
  // position f of the record (R1's orientation) -> the reference-orientation index i (0 for an f past the record), and per strand: whether i is padding
  // there, and the column of its consensus segment to read (0 where it is padding: the loads need no condition)
  __device__ __forceinline__ void locate(uint32_t f, uint32_t& i, uint32_t& k1, uint32_t& k2, bool& pad1, bool& pad2) const {
    i = f < C ? (r1_neg() ? C - 1 - f : f) : 0;
    pad1 = i < sh1 || i - sh1 >= l1; pad2 = i < sh2 || i - sh2 >= l2;
    const uint32_t j1 = pad1 ? 0 : i - sh1, j2 = pad2 ? 0 : i - sh2;
    k1 = l1 ? (rc1() ? l1 - 1 - j1 : j1) : 0; k2 = l2 ? (rc2() ? l2 - 1 - j2 : j2) : 0;
  }
};
// One position of a CODEC record from values in registers: the strands' calls as loaded at locate()'s columns (base code, quality, depth, errors;
// whatever was loaded for a padding position is dropped here), oriented and padded (codec_caller.rs:955-968, 1272-1314), combined (:1331-1512), the
// quality masks applied on the reference-orientation index — outer bases first, then single-strand stretches (:1526-1561) — and everything turned into
// R1's orientation.
struct CCol { uint32_t b1, q1, d1, e1, b2, q2, d2, e2, ob, oq, oe; bool pad1, pad2, dup, dis; };   // bases as 4-bit codes; padN = lower-case 'n' padding
__device__ __forceinline__ CCol codec_column(const CodecGeom& G, uint32_t i, uint32_t b1, uint32_t q1, uint32_t d1, uint32_t e1, bool pad1,
                                             uint32_t b2, uint32_t q2, uint32_t d2, uint32_t e2, bool pad2, const CodecEmitParams& P /* the masks */) {
  if (G.rc1()) b1 = comp_code((uint8_t)b1);
  if (G.rc2()) b2 = comp_code((uint8_t)b2);
  if (pad1) { b1 = 15; q1 = 0; d1 = 0; e1 = 0; }
  if (pad2) { b2 = 15; q2 = 0; d2 = 0; e2 = 0; }
  const bool ha = !pad1 && b1 != 15, hb = !pad2 && b2 != 15;
  bool dis = false;
  uint32_t fb, fq, err;
  auto sat = [](uint32_t de) { return de < 32767u ? de : 32767u; };     // the error count of a position is an int16
  if (ha && hb) {
    uint32_t rb, rq;
    if (b1 == b2) { rb = b1; const uint32_t sm = q1 + q2; rq = sm < 93 ? sm : 93; }
    else if (q1 > q2) { dis = true; rb = b1; rq = q1 - q2; if (rq < FGX_MIN_PHRED) rq = FGX_MIN_PHRED; }
    else if (q2 > q1) { dis = true; rb = b2; rq = q2 - q1; if (rq < FGX_MIN_PHRED) rq = FGX_MIN_PHRED; }
    else { dis = true; rb = b1; rq = FGX_MIN_PHRED; }
    if (rq == FGX_MIN_PHRED) { fb = 15; fq = FGX_MIN_PHRED; } else { fb = rb; fq = rq; }
    err = sat(b1 == b2 ? e1 + e2 : b1 == rb ? e1 + (d2 > e2 ? d2 - e2 : 0) : e2 + (d1 > e1 ? d1 - e1 : 0));
  } else if (ha) { if (q1 == FGX_MIN_PHRED) { fb = 15; fq = FGX_MIN_PHRED; } else { fb = b1; fq = q1; } err = e1; }
  else if (hb) { if (q2 == FGX_MIN_PHRED) { fb = 15; fq = FGX_MIN_PHRED; } else { fb = b2; fq = q2; } err = e2; }
  else { fb = 15; fq = FGX_MIN_PHRED; err = sat(e1 + e2); }
  if ((!pad1 && b1 == 15) || (!pad2 && b2 == 15)) { fb = 15; fq = FGX_MIN_PHRED; }     // an upper-case N on either strand
  if (P.has_outer && P.outer_len > 0 && (i < P.outer_len || G.C - 1 - i < P.outer_len)) fq = P.outer_qual;
  if (P.has_ss && (!ha || !hb)) fq = P.ss_qual;
  if (G.r1_neg()) { fb = comp_code((uint8_t)fb); b1 = comp_code((uint8_t)b1); b2 = comp_code((uint8_t)b2); }
  CCol c;
  c.b1 = b1; c.q1 = q1; c.d1 = d1; c.e1 = e1; c.b2 = b2; c.q2 = q2; c.d2 = d2; c.e2 = e2;
  c.ob = fb; c.oq = fq; c.oe = err; c.pad1 = pad1; c.pad2 = pad2; c.dup = ha && hb; c.dis = dis;
  return c;
}
// the CODEC-only counters of a record: consensus bases, duplex bases, duplex disagreements (n_dup / n_dis summed over the wavefront already)
__device__ __forceinline__ void codec_count(const CodecEmitParams& P, uint32_t lane, uint32_t C, uint32_t n_dup, uint32_t n_dis) {
  if (lane == 0) {
    unsigned long long* st = P.stats + (size_t)(blockIdx.x & (STAT_SLOTS - 1)) * 32;
    atomicAdd(&st[24], (unsigned long long)C);
    if (n_dup) atomicAdd(&st[25], (unsigned long long)n_dup);
    if (n_dis) atomicAdd(&st[26], (unsigned long long)n_dis);
  }
}

__global__ __launch_bounds__(256) void k_emit_codec(CodecEmitParams P) {
  const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)(P.slot0 + ((blockIdx.x * blockDim.x + threadIdx.x) >> 6)));
  const uint32_t lane = threadIdx.x & 63;
  if (slot >= P.slot_end) return;
  const CodecDesc& D = P.ends[slot];
  if (!D.valid || fast_ok(D, P.prefix_len, P.rg_len)) return;      // k_emit_codec_fast writes those
  const CodecGeom G(D);
  const uint32_t C = G.C;
  const uint64_t s1 = D.s1_off, s2 = D.s2_off;
  const uint8_t* mi = P.blob + P.rec_off[D.first_rec] + D.mi_off;
  const uint32_t mi_len = D.mi_len, name_len = P.prefix_len + 1 + mi_len;
  auto col = [&](uint32_t f) {       // position f of the record (R1's orientation)
    uint32_t i, k1, k2;
    bool pad1, pad2;
    G.locate(f, i, k1, k2, pad1, pad2);
    uint32_t b1 = 15, q1 = 0, d1 = 0, e1 = 0, b2 = 15, q2 = 0, d2 = 0, e2 = 0;     // (no load for a padding position)
    if (!pad1) { b1 = P.col_code[s1 + k1]; q1 = P.col_qual[s1 + k1]; d1 = P.col_depth[s1 + k1]; e1 = P.col_err[s1 + k1]; }
    if (!pad2) { b2 = P.col_code[s2 + k2]; q2 = P.col_qual[s2 + k2]; d2 = P.col_depth[s2 + k2]; e2 = P.col_err[s2 + k2]; }
    return codec_column(G, i, b1, q1, d1, e1, pad1, b2, q2, d2, e2, pad2, P);
  };
  // ---- reductions: cD cM cE / aD aM aE / bD bM bE, and the duplex counters -----------------------------------------------------
  StrandStats A, B, AB;
  uint32_t n_dup = 0, n_dis = 0;
  for (uint32_t f = lane; f < C; f += 64) {
    const CCol c = col(f);
    A.add(c.d1, c.e1); B.add(c.d2, c.e2); AB.add(c.d1 + c.d2, c.oe);
    n_dup += c.dup ? 1 : 0; n_dis += c.dis ? 1 : 0;
  }
  reduce_stats(A, B, AB, C);
  codec_count(P, lane, C, wave_sum(n_dup), wave_sum(n_dis));
  // ---- the record (flag: unmapped fragment): block_size + core, name, bases, quals, then the tags in the reference's order ------------
  FieldWriterNested W{P.out + P.out_off[slot], lane};
  W.core(D.rec_size, name_len, (uint32_t)bam::F_UNMAPPED, C);
  W.name(P.prefix, P.prefix_len, mi, name_len);
  W.seq_qual_any(C, [&](uint32_t f) { return col(f).ob; }, [&](uint32_t f) { return col(f).oq; });
  W.z_any('R', 'G', (const uint8_t*)P.rg, P.rg_len);
  W.z_any('M', 'I', mi, mi_len);
  W.scalars('c', true, AB.dmax, AB.dmin, AB.rate());
  W.scalars('a', true, A.dmax, A.dmin, A.rate());
  W.scalars('b', true, B.dmax, B.dmin, B.rate());
  if (P.per_base_tags) {
    W.i16_any('a', 'd', C, [&](uint32_t f) { return col(f).d1; });
    W.i16_any('b', 'd', C, [&](uint32_t f) { return col(f).d2; });
    W.i16_any('a', 'e', C, [&](uint32_t f) { return col(f).e1; });
    W.i16_any('b', 'e', C, [&](uint32_t f) { return col(f).e2; });
    W.string_any('a', 'c', C, [&](uint32_t f) { const CCol c = col(f); return c.pad1 ? (uint8_t)'n' : bam::code_to_ascii((uint8_t)c.b1); });
    W.string_any('b', 'c', C, [&](uint32_t f) { const CCol c = col(f); return c.pad2 ? (uint8_t)'n' : bam::code_to_ascii((uint8_t)c.b2); });
    W.string_any('a', 'q', C, [&](uint32_t f) { const uint32_t qq = col(f).q1 + 33; return qq > 255 ? 255u : qq; });
    W.string_any('b', 'q', C, [&](uint32_t f) { const uint32_t qq = col(f).q2 + 33; return qq > 255 ? 255u : qq; });
  }
  if (D.has_cb) W.z_any(P.cell0, P.cell1, P.blob + P.rec_off[D.cb_rec] + D.cb_off, D.cb_len);
  if (D.has_rx) W.z_any('R', 'X', (const uint8_t*)D.rx, D.rx_len);
}

// -----------------------------------------------------------------------------------------------------
// Fast record writers for duplex and CODEC.  The per-field writers above wait on a memory round trip for every
// 64 bytes they produce and re-evaluate the strand combine for every field; here each lane owns PAIRS of
// positions (2·lane, 2·lane+1, then +128 per slot), loads all of them in one sweep, evaluates the combine once
// per position into three packed registers, and then only stores: a string field is two byte stores per slot, an
// int16 array four, packed bases one — no cross-lane traffic, no waits.  Records that do not fit the register
// budget (or have unusually long names / tags) are left to the per-field kernels, which skip what is done here.
// -----------------------------------------------------------------------------------------------------
// shared field writers (q advances; every lane calls them)
// (The small fields are written as straight-line code — uniform words built by the scalar unit, a lane's byte taken with one shift,
// one-level selects —: nested conditionals over the lane number compile into nested exec-mask regions, and the record writers were bound by
// scalar instructions, profiles/r04_experiments.md.)
struct FieldWriterFlat {
  uint8_t* q; uint32_t lane;
  __device__ __forceinline__ uint32_t sh3() const { return 8u * (lane < 3u ? lane : 3u); }   // (a 24-bit header word >> sh3: its byte for lanes 0 - 2, 0 from lane 3 on)
  // one store: bytes [0, n) with n <= 64, byte i = f(i)
  template <class F> __device__ __forceinline__ void small(uint32_t n, F f) { const uint8_t b = f(lane); if (lane < n) q[lane] = b; q += n; }
  __device__ __forceinline__ void z_small(char t0, char t1, const uint8_t* src, uint32_t n) {       // Z tag, n + 4 <= 64
    const uint32_t k = lane >= 3 ? lane - 3 : 0;
    const uint32_t b = src[k < n ? k : (n ? n - 1 : 0)];
    const uint32_t c3 = (uint32_t)(uint8_t)t0 | ((uint32_t)(uint8_t)t1 << 8) | ((uint32_t)'Z' << 16);
    const uint32_t u = (lane - 3u < n) ? b : 0u;                                                      // (unsigned: false for lanes 0 - 2)
    const uint32_t v = (c3 >> sh3()) | u;
    if (lane < 3 + n + 1) q[lane] = (uint8_t)v;
    q += 3 + n + 1;
  }
  __device__ __forceinline__ void scalars(char s, bool m_second, uint32_t dmax, uint32_t dmin, float rate) {   // <s>D <s>E <s>M (duplex) or <s>D <s>M <s>E (CODEC)
    // three uniform words: an integer tag here is `<s>D` + its type + ONE value byte (4 bytes), the rate `<s>Ef` + its four bytes (7)
    auto int_word = [&](uint32_t b, uint32_t v) -> unsigned long long {
      const uint32_t ty = v <= 127 ? (uint32_t)'c' : v <= 255 ? (uint32_t)'C' : (uint32_t)'S';
      return (unsigned long long)((uint32_t)(uint8_t)s | (b << 8) | (ty << 16) | ((v & 0xFFu) << 24));
    };
    const unsigned long long wD = int_word('D', dmax), wM = int_word('M', dmin);
    const unsigned long long wE = (unsigned long long)((uint32_t)(uint8_t)s | ((uint32_t)'E' << 8) | ((uint32_t)'f' << 16)) | ((unsigned long long)__float_as_uint(rate) << 24);
    const unsigned long long w2 = m_second ? wM : wE, w3 = m_second ? wE : wM;
    const uint32_t n2 = m_second ? 4u : 7u;
    unsigned long long w = wD;
    uint32_t k = lane;
    if (lane >= 4u) { w = w2; k = lane - 4u; }
    if (lane >= 4u + n2) { w = w3; k = lane - 4u - n2; }
    const uint32_t v = (uint32_t)(w >> (8u * (k & 7u)));
    if (lane < 15) q[lane] = (uint8_t)v;
    q += 15;
  }
  __device__ __forceinline__ void header3(char t0, char t1) {                                        // `xyZ`
    const uint32_t c3 = (uint32_t)(uint8_t)t0 | ((uint32_t)(uint8_t)t1 << 8) | ((uint32_t)'Z' << 16);
    const uint32_t v = c3 >> sh3();
    if (lane < 3) q[lane] = (uint8_t)v;
    q += 3;
  }
  __device__ __forceinline__ void header8(char t0, char t1, uint32_t L) {                            // `xyBs` + the count
    const unsigned long long w = (unsigned long long)((uint32_t)(uint8_t)t0 | ((uint32_t)(uint8_t)t1 << 8) | ((uint32_t)'B' << 16) | ((uint32_t)'s' << 24)) | ((unsigned long long)L << 32);
    const uint32_t v = (uint32_t)(w >> (8u * (lane & 7u)));
    if (lane < 8) q[lane] = (uint8_t)v;
    q += 8;
  }
  __device__ __forceinline__ void core(uint32_t rec_size, uint32_t name_len, uint32_t flag, uint32_t L) {
    uint32_t v = 0xFFFFFFFFu;
    if (lane == 0) v = rec_size;
    if (lane == 3) v = (name_len + 1) | (4680u << 16);
    if (lane == 4) v = flag << 16;
    if (lane == 5) v = L;
    if (lane == 8) v = 0u;
    if (lane < 9) gst32u(q + 4 * lane, v);
    q += 36;
  }
};

template <uint32_t SLOTS, class FW, class B>      // string field of L bytes after a 3-byte `xyZ` header and before a NUL
__device__ __forceinline__ void put_string(FW& W, char t0, char t1, uint32_t L, B byte_of) {
  W.header3(t0, t1);
  // a lane's two positions are neighbours in the record: ONE 16-bit store (gfx950 takes them unaligned) instead of two byte stores
#pragma unroll
  for (uint32_t t = 0; t < SLOTS; t++) {
    const uint32_t p = 128 * t + 2 * W.lane;
    if (p + 1 < L) gst16u(W.q + p, (uint32_t)(uint8_t)byte_of(t, 0) | ((uint32_t)(uint8_t)byte_of(t, 1) << 8));
    else if (p < L) W.q[p] = byte_of(t, 0);
  }
  if (W.lane == 0) W.q[L] = 0;
  W.q += L + 1;
}
template <uint32_t SLOTS, class FW, class V>      // B:s array of L int16 values
__device__ __forceinline__ void put_i16(FW& W, char t0, char t1, uint32_t L, V val_of) {
  W.header8(t0, t1, L);
  // a lane's two int16 values are four consecutive bytes: one (unaligned) dword store instead of four byte stores
#pragma unroll
  for (uint32_t t = 0; t < SLOTS; t++) {
    const uint32_t p = 128 * t + 2 * W.lane;
    if (p + 1 < L) gst32u(W.q + 2 * p, ((uint32_t)val_of(t, 0) & 0xFFFFu) | ((uint32_t)val_of(t, 1) << 16));
    else if (p < L) gst16u(W.q + 2 * p, (uint32_t)val_of(t, 0));
  }
  W.q += 2 * L;
}
template <uint32_t SLOTS, class FW, class C, class Q>   // 4-bit packed bases, then qualities
__device__ __forceinline__ void put_seq_qual(FW& W, uint32_t L, C code_of, Q qual_of) {
#pragma unroll
  for (uint32_t t = 0; t < SLOTS; t++) {
    const uint32_t p = 128 * t + 2 * W.lane;
    if (p < L) W.q[p >> 1] = (uint8_t)((code_of(t, 0) << 4) | (p + 1 < L ? code_of(t, 1) : 0u));
  }
  W.q += (L + 1) / 2;
#pragma unroll
  for (uint32_t t = 0; t < SLOTS; t++) {
    const uint32_t p = 128 * t + 2 * W.lane;
    if (p + 1 < L) gst16u(W.q + p, ((uint32_t)qual_of(t, 0) & 0xFFu) | (((uint32_t)qual_of(t, 1) & 0xFFu) << 8));
    else if (p < L) W.q[p] = (uint8_t)qual_of(t, 0);
  }
  W.q += L;
}

// (round 6) how many valid records the fast writers refuse — a thread per slot, one atomic per wavefront: the per-field writers (k_emit_duplex / k_emit_codec)
// are launched only when the count is not 0.  (Counting inside the fast writers cost them a wavefront per SIMD: 71 -> 73 / 79 -> 89 VGPRs.)
template <class Desc>     // DuplexDesc or CodecDesc (fast_ok is overloaded for the two)
__global__ __launch_bounds__(256) void k_count_slow(const Desc* __restrict__ ends, uint32_t slot0, uint32_t slot_end, uint32_t prefix_len, uint32_t rg_len, uint32_t* __restrict__ n_slow) {
  const uint32_t slot = slot0 + blockIdx.x * blockDim.x + threadIdx.x;
  bool slow = false;
  if (slot < slot_end) { const Desc& D = ends[slot]; slow = D.valid && !fast_ok(D, prefix_len, rg_len); }
  const unsigned long long m = __ballot(slow);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(n_slow, (uint32_t)__popcll(m));
}
template <int METH, int CAP = 0>     // METH 1: the methylation-aware mode (the conversion-artifact rule in the strand combine); CAP: see k_emit_duplex
__global__ __launch_bounds__(256) void k_emit_duplex_fast(DuplexEmitParams P) {
  const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)(P.slot0 + ((blockIdx.x * blockDim.x + threadIdx.x) >> 6)));
  const uint32_t lane = threadIdx.x & 63;
  if (slot >= P.slot_end) return;
  const DuplexDesc& D = P.ends[slot];
  if (!D.valid || !fast_ok(D, P.prefix_len, P.rg_len)) return;
  const uint32_t L = D.len, lastp = L ? L - 1 : 0;
  const bool has_ba = D.has_ba != 0;
  const uint64_t a_off = D.a_off, b_off = has_ba ? D.b_off : D.a_off;
  const uint8_t* first = P.blob + P.rec_off[D.first_rec];
  const uint32_t mi_len = D.mi_len, mi_off = D.mi_off, name_len = P.prefix_len + 1 + mi_len;
  const bool has_cb = D.has_cb != 0, has_rx = D.has_rx != 0;
  const uint32_t cb_len = has_cb ? D.cb_len : 0, rx_len = has_rx ? D.rx_len : 0;
  const uint32_t flag = bam::F_UNMAPPED | bam::F_PAIRED | bam::F_MATE_UNMAPPED | (D.type == 1 ? bam::F_FIRST : bam::F_LAST);
  // ---- every load of the record (indices clamped into the record's own segments, so unconditional) -----------------------
  uint32_t ca[DUP_SLOTS][2], qa[DUP_SLOTS][2], ea[DUP_SLOTS][2], oa[DUP_SLOTS][2], cb[DUP_SLOTS][2], qb[DUP_SLOTS][2], eb[DUP_SLOTS][2], ob[DUP_SLOTS][2];
  uint32_t rc[DUP_SLOTS];           // methylation-aware mode: either strand flags a reference cytosine, a byte per position of the pair
  uint32_t na[DUP_SLOTS][2], nb[DUP_SLOTS][2];     // CAP: the recount's counts (every source read) of a capped record
  const bool capped = CAP != 0 && D.capped != 0;
#pragma unroll
  for (uint32_t t = 0; t < DUP_SLOTS; t++) {
    // (round 6) a lane's two neighbouring positions with ONE load per array and strand (2 + 2 + 4 + 8 bytes) instead of one per position: 16 vector memory
    // instructions per lane where there were 32.  The pair's first position is clamped into the record; its second may lie one column past the end
    // (the scratch arrays carry slack) — such a position is masked out of the statistics and written by no field writer.
    const uint32_t pb = 128 * t + 2 * lane, pc = pb < lastp ? pb : lastp;
    auto ld2 = [&](uint64_t off, uint32_t* c2, uint32_t* q2, uint32_t* e2, uint32_t* o2) {
      uint16_t cw, qw; uint32_t ew; unsigned long long ow;
      __builtin_memcpy(&cw, P.col_code + off, 2); __builtin_memcpy(&qw, P.col_qual + off, 2);
      __builtin_memcpy(&ew, (const uint8_t*)P.col_err + 2 * off, 4); __builtin_memcpy(&ow, (const uint8_t*)P.col_obs + 4 * off, 8);
      c2[0] = cw & 0xFFu; c2[1] = cw >> 8; q2[0] = qw & 0xFFu; q2[1] = qw >> 8; e2[0] = ew & 0xFFFFu; e2[1] = ew >> 16; o2[0] = (uint32_t)ow; o2[1] = (uint32_t)(ow >> 32);
    };
    ld2(a_off + pc, ca[t], qa[t], ea[t], oa[t]);
    ld2(b_off + pc, cb[t], qb[t], eb[t], ob[t]);
    if constexpr (CAP != 0) {
      na[t][0] = oa[t][0]; na[t][1] = oa[t][1]; nb[t][0] = ob[t][0]; nb[t][1] = ob[t][1];
      if (capped) {
        unsigned long long wa, wb;
        __builtin_memcpy(&wa, (const uint8_t*)P.col_obs_all + 4 * (a_off + pc), 8); __builtin_memcpy(&wb, (const uint8_t*)P.col_obs_all + 4 * (b_off + pc), 8);
        na[t][0] = (uint32_t)wa; na[t][1] = (uint32_t)(wa >> 32); nb[t][0] = (uint32_t)wb; nb[t][1] = (uint32_t)(wb >> 32);
      }
    }
    rc[t] = 0;
    if constexpr (METH != 0) { uint16_t fa, fb; __builtin_memcpy(&fa, P.meth_flag + a_off + pc, 2); __builtin_memcpy(&fb, P.meth_flag + b_off + pc, 2); rc[t] = (uint32_t)(fa | fb); }
  }
  const uint32_t k3 = lane >= 3 ? lane - 3 : 0, ni = lane > P.prefix_len ? lane - P.prefix_len - 1 : 0;
  const uint8_t pfx = (uint8_t)P.prefix[lane < P.prefix_len ? lane : 0], nmb = first[mi_off + (ni < mi_len ? ni : mi_len)];
  // ---- the duplex call of each position, packed: w0 = ca | cb<<4 | oc<<8 | qa<<16 | qb<<24 ; w1 = da | db<<8 | ea<<16 | eb<<24 ; w2 = oq | oe<<8
  uint32_t w0[DUP_SLOTS][2], w1[DUP_SLOTS][2], w2[DUP_SLOTS][2];
  StrandStats A, B, AB;
#pragma unroll
  for (uint32_t t = 0; t < DUP_SLOTS; t++)
#pragma unroll
    for (uint32_t k = 0; k < 2; k++) {
      const uint32_t da = obs_sum(oa[t][k]);
      uint32_t db = 0, xcb = 15, xqb = 0, xeb = 0, oc = ca[t][k], oq = qa[t][k], oe = ea[t][k];
      if (has_ba) {      // (duplex_column's rule, spelled out: see there)
        db = obs_sum(ob[t][k]); xcb = cb[t][k]; xqb = qb[t][k]; xeb = eb[t][k];
        const DCall d = duplex_call<METH>(ca[t][k], qa[t][k], xcb, xqb, ((rc[t] >> (8 * k)) & 0xFFu) != 0);
        oc = d.oc; oq = d.oq;
        if constexpr (CAP != 0) oe = duplex_errors(d, obs_sum(na[t][k]) + obs_sum(nb[t][k]), na[t][k], nb[t][k]);
        else oe = duplex_errors(d, da + db, oa[t][k], ob[t][k]);
      }
      w0[t][k] = ca[t][k] | (xcb << 4) | (oc << 8) | (qa[t][k] << 16) | (xqb << 24);
      w1[t][k] = da | (db << 8) | (ea[t][k] << 16) | (xeb << 24);
      w2[t][k] = oq | (oe << 8);
      if (128 * t + 2 * lane + k < L) { A.add(da, ea[t][k]); B.add(db, xeb); AB.add(da + db, oe); }
    }
  reduce_stats(A, B, AB, L);
  const float a_rate = A.rate(), b_rate = B.rate(), c_rate = AB.rate();
  // ---- stores ------------------------------------------------------------------------------------------------------------------
  FieldWriterFlat W{P.out + P.out_off[slot], lane};
  W.core(D.rec_size, name_len, flag, L);
  W.small(name_len + 1, [&](uint32_t i) { const uint8_t x = i == P.prefix_len ? (uint8_t)':' : nmb, y = i < P.prefix_len ? pfx : x; return i < name_len ? y : (uint8_t)0; });   // (three one-level selects)
  put_seq_qual<DUP_SLOTS>(W, L, [&](uint32_t t, uint32_t k) { return (w0[t][k] >> 8) & 15; }, [&](uint32_t t, uint32_t k) { return w2[t][k] & 0xFF; });
  W.z_small('M', 'I', first + mi_off, mi_len);
  if (has_cb) W.z_small(P.cell0, P.cell1, P.blob + P.rec_off[D.cb_rec] + D.cb_off, cb_len);
  W.z_small('R', 'G', (const uint8_t*)P.rg, P.rg_len);
  W.scalars('a', false, A.dmax, A.dmin, a_rate);
  if (P.per_base_tags) {
    put_string<DUP_SLOTS>(W, 'a', 'c', L, [&](uint32_t t, uint32_t k) { return bam::code_to_ascii((uint8_t)(w0[t][k] & 15)); });
    put_i16<DUP_SLOTS>(W, 'a', 'd', L, [&](uint32_t t, uint32_t k) { return w1[t][k] & 0xFF; });
    put_i16<DUP_SLOTS>(W, 'a', 'e', L, [&](uint32_t t, uint32_t k) { return (w1[t][k] >> 16) & 0xFF; });
    put_string<DUP_SLOTS>(W, 'a', 'q', L, [&](uint32_t t, uint32_t k) { return (uint8_t)(((w0[t][k] >> 16) & 0xFF) + 33); });
  }
  W.scalars('b', false, B.dmax, B.dmin, b_rate);
  if (P.per_base_tags && has_ba) {
    put_string<DUP_SLOTS>(W, 'b', 'c', L, [&](uint32_t t, uint32_t k) { return bam::code_to_ascii((uint8_t)((w0[t][k] >> 4) & 15)); });
    put_i16<DUP_SLOTS>(W, 'b', 'd', L, [&](uint32_t t, uint32_t k) { return (w1[t][k] >> 8) & 0xFF; });
    put_i16<DUP_SLOTS>(W, 'b', 'e', L, [&](uint32_t t, uint32_t k) { return w1[t][k] >> 24; });
    put_string<DUP_SLOTS>(W, 'b', 'q', L, [&](uint32_t t, uint32_t k) { return (uint8_t)((w0[t][k] >> 24) + 33); });
  }
  W.scalars('c', false, AB.dmax, AB.dmin, c_rate);
  if (has_rx) W.z_small('R', 'X', (const uint8_t*)D.rx, rx_len);
}

__global__ __launch_bounds__(256) void k_emit_codec_fast(CodecEmitParams P) {
  const uint32_t slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)(P.slot0 + ((blockIdx.x * blockDim.x + threadIdx.x) >> 6)));
  const uint32_t lane = threadIdx.x & 63;
  if (slot >= P.slot_end) return;
  const CodecDesc& D = P.ends[slot];
  if (!D.valid || !fast_ok(D, P.prefix_len, P.rg_len)) return;
  const CodecGeom G(D);
  const uint32_t C = G.C;
  const uint64_t s1 = D.s1_off, s2 = D.s2_off;
  const uint8_t* first = P.blob + P.rec_off[D.first_rec];
  const uint32_t mi_len = D.mi_len, mi_off = D.mi_off, name_len = P.prefix_len + 1 + mi_len;
  const bool has_cb = D.has_cb != 0, has_rx = D.has_rx != 0;
  const uint32_t cb_len = has_cb ? D.cb_len : 0, rx_len = has_rx ? D.rx_len : 0;
  const uint32_t ni = lane > P.prefix_len ? lane - P.prefix_len - 1 : 0;
  const uint8_t pfx = (uint8_t)P.prefix[lane < P.prefix_len ? lane : 0], nmb = first[mi_off + (ni < mi_len ? ni : mi_len)];
  // field layout of the record (every offset is known up front, so the position-indexed fields can be written window by window)
  uint8_t* const rec = P.out + P.out_off[slot];
  uint8_t* const q_seq = rec + 36 + name_len + 1;
  uint8_t* const q_qual = q_seq + (C + 1) / 2;
  uint8_t* const q_rg = q_qual + C;
  uint8_t* const q_scal = q_rg + (3 + P.rg_len + 1) + (3 + mi_len + 1);
  uint8_t* const q_arr = q_scal + 45;                       // ad bd ae be: 8 + 2C each
  uint8_t* const q_str = q_arr + 4 * (8 + 2 * C);           // ac bc aq bq: 3 + C + 1 each
  uint8_t* const q_tail = P.per_base_tags ? q_str + 4 * (3 + C + 1) : q_arr;
  StrandStats A, B, AB;
  uint32_t n_dup = 0, n_dis = 0;
  for (uint32_t win = 0; win < C; win += 256) {             // 256 positions per sweep: 4 per lane, all loads of the sweep in flight together
    uint32_t vb1[4], vq1[4], vd1[4], ve1[4], vb2[4], vq2[4], vd2[4], ve2[4];
    bool vp1[4], vp2[4];
    uint32_t vi[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
      uint32_t k1, k2;
      G.locate(win + 128 * (u >> 1) + 2 * lane + (u & 1), vi[u], k1, k2, vp1[u], vp2[u]);
      vb1[u] = P.col_code[s1 + k1]; vq1[u] = P.col_qual[s1 + k1]; vd1[u] = P.col_depth[s1 + k1]; ve1[u] = P.col_err[s1 + k1];
      vb2[u] = P.col_code[s2 + k2]; vq2[u] = P.col_qual[s2 + k2]; vd2[u] = P.col_depth[s2 + k2]; ve2[u] = P.col_err[s2 + k2];
    }
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
      const uint32_t f = win + 128 * (u >> 1) + 2 * lane + (u & 1);
      const CCol c = codec_column(G, vi[u], vb1[u], vq1[u], vd1[u], ve1[u], vp1[u], vb2[u], vq2[u], vd2[u], ve2[u], vp2[u], P);
      if (f < C) {
        A.add(c.d1, c.e1); B.add(c.d2, c.e2); AB.add(c.d1 + c.d2, c.oe);
        n_dup += c.dup ? 1 : 0; n_dis += c.dis ? 1 : 0;
        q_qual[f] = (uint8_t)c.oq;
        if (P.per_base_tags) {
          uint8_t* a = q_arr + 8 + 2 * f;
          a[0] = (uint8_t)c.d1; a[1] = 0;
          a += 8 + 2 * C; a[0] = (uint8_t)c.d2; a[1] = 0;
          a += 8 + 2 * C; a[0] = (uint8_t)c.e1; a[1] = 0;
          a += 8 + 2 * C; a[0] = (uint8_t)c.e2; a[1] = 0;
          uint8_t* z = q_str + 3 + f;
          z[0] = c.pad1 ? (uint8_t)'n' : bam::code_to_ascii((uint8_t)c.b1);
          z += 3 + C + 1; z[0] = c.pad2 ? (uint8_t)'n' : bam::code_to_ascii((uint8_t)c.b2);
          z += 3 + C + 1; z[0] = (uint8_t)(c.q1 + 33);
          z += 3 + C + 1; z[0] = (uint8_t)(c.q2 + 33);
        }
      }
      vb1[u] = c.ob;     // keep the duplex base for the nibble packing below
    }
#pragma unroll
    for (uint32_t h = 0; h < 2; h++) {   // packed bases: this lane's two positions of each half-window share one byte
      const uint32_t f = win + 128 * h + 2 * lane;
      if (f < C) q_seq[f >> 1] = (uint8_t)((vb1[2 * h] << 4) | (f + 1 < C ? vb1[2 * h + 1] : 0u));
    }
  }
  reduce_stats(A, B, AB, C);
  codec_count(P, lane, C, wave_sum(n_dup), wave_sum(n_dis));
  // ---- the fields that are not indexed by position ----------------------------------------------------------------------------
  FieldWriterNested W{rec, lane};
  W.core(D.rec_size, name_len, (uint32_t)bam::F_UNMAPPED, C);
  W.small(name_len + 1, [&](uint32_t i) { return i < P.prefix_len ? pfx : i == P.prefix_len ? (uint8_t)':' : i < name_len ? nmb : (uint8_t)0; });
  W.q = q_rg;
  W.z_small('R', 'G', (const uint8_t*)P.rg, P.rg_len);
  W.z_small('M', 'I', first + mi_off, mi_len);
  W.scalars('c', true, AB.dmax, AB.dmin, AB.rate());
  W.scalars('a', true, A.dmax, A.dmin, A.rate());
  W.scalars('b', true, B.dmax, B.dmin, B.rate());
  if (P.per_base_tags) {
    if (lane < 32) {          // the four array headers and the four string headers + terminators
      const uint32_t r = lane >> 3, i = lane & 7;
      const char t0 = (r & 1) ? 'b' : 'a', t1 = r < 2 ? 'd' : 'e';
      q_arr[(size_t)r * (8 + 2 * C) + i] = i == 0 ? (uint8_t)t0 : i == 1 ? (uint8_t)t1 : i == 2 ? (uint8_t)'B' : i == 3 ? (uint8_t)'s' : (uint8_t)(C >> (8 * ((i - 4) & 3)));
    } else if (lane < 48) {
      const uint32_t r = (lane - 32) >> 2, i = (lane - 32) & 3;
      const char t0 = (r & 1) ? 'b' : 'a', t1 = r < 2 ? 'c' : 'q';
      uint8_t* z = q_str + (size_t)r * (3 + C + 1);
      if (i < 3) z[i] = i == 0 ? (uint8_t)t0 : i == 1 ? (uint8_t)t1 : (uint8_t)'Z'; else z[3 + C] = 0;
    }
  }
  W.q = q_tail;
  if (has_cb) W.z_small(P.cell0, P.cell1, P.blob + P.rec_off[D.cb_rec] + D.cb_off, cb_len);
  if (has_rx) W.z_small('R', 'X', (const uint8_t*)D.rx, rx_len);
}
