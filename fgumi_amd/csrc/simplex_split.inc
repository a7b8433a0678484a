// simplex_split.inc — the split simplex pipeline: k_split_parse (record kernel) + k_split_cols (column kernel).
// Included by fastpath.hip inside `namespace fgx { namespace {` after simplex_wave2.inc (uni, kahan2, GateTables, unanimous_call_lds).
//
// Why: k_simplex_wave2 spends half of its vector instructions in phases where lane = record — header parse, aux walk, mate
// clip, name hash, pairing, UMI comparison — with n of 64 lanes busy (16 at depth 8), and its column loop pays ~20 vector
// instructions per member step for 8 useful f64 operations (per-member descriptor broadcast, two address adds, clamp, and a
// cold block that the whole wavefront walks whenever ONE lane has seen a second base).  Here the work is cut at the record /
// column boundary:
//
//   k_split_parse   a wavefront takes a run of consecutive families, 64 records per round, lane = record: everything that needs
//                   only the record header and its tags, straight from global memory (no LDS staging) — shape checks, aux walk
//                   (MC / MI / RX / cell tag), closed-form mate clip, name hash, mate pairing inside the family (rotation over
//                   the hash, names verified), the shared reference span of each pair, UMI equality, and the row of each read in
//                   the family's LDS tile.  Leaves a 32-byte SplitRec per record, a 32-byte SplitFam per family, and (in place of
//                   k_col_bound) the family's scratch-column bound and byte-span descriptor.
//   k_split_cols    one wavefront per family: stages ONLY sequence + qualities (225 of 330 bytes) into a row-per-read tile with
//                   fixed row strides, end A's rows first; overlap correction in LDS; clip / fill; final lengths; gates; then the
//                   column loop over a flat column space of both ends (lane = column, 64 per pass; a 2 x 150 family = 5 passes):
//                   every member step is two byte reads at `lane address + row * stride` (no descriptor broadcast, no clamp:
//                   256-entry pair table), the allow-mask test and 8 f64 operations.  A column that shows a second base leaves
//                   the loop for good: its observations (<= 16 rows) travel to k_call_full, which runs the four-lane Kahan sum —
//                   the hot loop never executes the cold block.
//
// Shape taken by k_split_cols (decided in k_split_parse; everything else goes, untouched, to k_simplex_wave2 and from there down
// the usual chain): k_simplex_wave2's record shape (simplex_wave2.inc) and, in addition, per end one strand (reverse ends: one
// read length), no family with fragments AND pairs, record counts within --max-reads, UMIs all equal (or absent), at most 16
// rows per end when a column disagrees.
//
// Reference semantics restated: the same as k_simplex_wave2 (vanilla_caller.rs:1080-1296, 1304-1422, 1454-1646, 1652-1755;
// overlapping.rs:236-336, 627-684; raw-bam/overlap.rs:181-357; simple_umi.rs:46-117).

#ifndef FGX_S2_OCC
#define FGX_S2_OCC 6
#endif
#ifndef FGX_S2_OCC_PACKED
#define FGX_S2_OCC_PACKED 7   /* the packed build: 46 VGPRs (eight wavefronts per SIMD by registers), 5632-byte slices and 368 bytes of tables — seven workgroups of four wavefronts in a CU's 160 KB; at a bound of 8 the compiler caps the kernel at 78 scalar registers and its uniforms spill again */
#endif
#ifndef FGX_S2_PAIRS
#define FGX_S2_PAIRS 256   /* rows of the {correct, error} table: 256 = indexed by the raw quality byte (no clamp in the loop) */
#endif

#ifndef FGX_S2_F32
#define FGX_S2_F32 1   /* 1: k_split_cols sums a column's single-base observations in f32 (two adds per observation) and lets only the columns
                          an error-inflated gate cannot decide go to k_call_full, which recomputes them exactly (see unanimous_call_approx);
                          0: two f64 Kahan chains per observation (rounds 2 - 3), for measurements */
#endif
#ifndef FGX_S2_FMASEL
#define FGX_S2_FMASEL 1   /* f32 sums: an observation is added as acc = pair * {sel, sel} + acc with sel = 1.0 / 0.0 (one select + one packed fma,
                             the count of observations as a third f32 sum) instead of one packed add + two selects + a 0 / 1 select and its add */
#endif
#ifndef FGX_S2_NOSUM
#define FGX_S2_NOSUM 1    /* round 5: ends of at least unanimous_cap_depth() rows run the sum-free observation step (S2_OBSERVE_FAST); 0: measurements */
#endif
#ifndef FGX_S2_PREGATE
#define FGX_S2_PREGATE 1  /* f32 sums: the answer "the cap" — what a clean column of a deep family gets — is decided in seven f32 instructions
                             (s2_cap_pregate); only the lanes it does not cover run the f64 gate */
#endif
struct S2Lds {
  GateTables g;
  uint8_t t1[96];                              // (round 5) the consensus quality of a column that holds ONE observation, by its quality (0xFF: not a table answer)
  alignas(16) float pairf[FGX_S2_PAIRS][2];    // {correct, error_per_alt} rounded to f32: k_split_cols's hot loop (it copies the image up to here)
  alignas(16) double pair[FGX_S2_PAIRS][2];    // the f64 pairs: k_deep_cols
};
// what lies in device memory (FastParams::s2_image): the LDS image, then (round 6) the consensus quality of a column that holds TWO observations of one
// base, by their qualities in file order (0xFF: not a table answer) — 8.8 KB the packed build reads from global memory (no kernel copies it into LDS)
struct S2Image {
  S2Lds lds;
  alignas(16) uint8_t t2[(pk::T2_BYTES + 15u) & ~15u];
};
static_assert(offsetof(S2Image, lds) == 0, "kernels read FastParams::s2_image as an S2Lds");
struct S2Tiny {             // what the packed build of k_split_cols (COLS 1) keeps: the cap and the one-observation table — 3.8 KB less LDS per
  struct { uint32_t cap; } g;   // workgroup than S2Head, which is a seventh workgroup per CU
  uint8_t t1[96];
};
struct S2Head {             // what k_split_cols keeps in LDS with f32 sums: the image up to the f64 pairs
  GateTables g;
  uint8_t t1[96];
  alignas(16) float pairf[FGX_S2_PAIRS][2];
};
constexpr uint32_t S2_HEAD_BYTES = (uint32_t)(offsetof(S2Lds, pair));
static_assert(sizeof(S2Head) == S2_HEAD_BYTES, "S2Head is the head of S2Lds");
static_assert(S2_HEAD_BYTES % 16 == 0, "the head of S2Lds is copied in 16-byte pieces");
static_assert(sizeof(S2Lds) % 16 == 0, "S2Lds is copied in 16-byte pieces");
inline void build_s2_image(S2Image& I, const ConsensusTables& t) {
  memset(&I, 0, sizeof(I));
  S2Lds& L = I.lds;
  fill_gate_tables(L.g, t);
  for (uint32_t i = 0; i < FGX_S2_PAIRS; i++) {
    const uint32_t q = i < 93 ? i : 93;
    L.pair[i][0] = t.correct[q]; L.pair[i][1] = t.error_per_alt[q];
  }
  fill_pairs_f32(L.pairf, FGX_S2_PAIRS, t);      // (gate_core.h: rounding and the finite stand-in for ln 0)
  pk::fill_t1(L.t1, t);                          // (packed_core.h: the call of a column that holds ONE observation, by its quality)
  pk::fill_t2(I.t2, t);                          // (... TWO observations of one base)
}

// a * b for a, b < 2^24 (the low 32 bits of the product): v_mul_u32_u24 is a full-rate instruction, v_mul_lo_u32 takes four times as long; the
// compiler picks the 24-bit form only when it can prove both ranges
#if defined(FGX_WAVEMU)
__device__ __forceinline__ uint32_t s2_mul24(uint32_t a, uint32_t b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
#else
__device__ __forceinline__ uint32_t s2_mul24(uint32_t a, uint32_t b) { uint32_t r; asm("v_mul_u32_u24_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
#endif
__device__ __forceinline__ uint32_t mbcnt64(unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }   // bits of m below this lane

// -----------------------------------------------------------------------------------------------------------------------------
// k_split_parse — lane = record, 64 records (a run of whole families) per round
// -----------------------------------------------------------------------------------------------------------------------------
// Every lane keeps two windows of its record in LDS: SP_HEAD bytes behind the fixed header (name, CIGAR) and the first SP_AUX bytes
// of the tag block — two memory round trips (five and four 16-byte loads per lane, all in flight together) instead of a dependent
// chain of ~15 small loads through the name and the tag entries.  A tag block longer than its window is walked in global memory.
constexpr uint32_t SP_HEAD = 48, SP_AUX = 64, SP_LANE = SP_HEAD + SP_AUX;   // head window: bytes [32, 80) of the record (name, CIGAR)
constexpr uint32_t SP_WAVE_LDS = 64 * SP_LANE + 16;   // (+ slack: the string scan reads whole 8-byte words)
// Families [g_begin, n_grp) — the host launches it chunk by chunk on a second stream, so that the record kernel of chunk i + 1 (waiting
// on memory most of its time) runs under the column kernel of chunk i (bound by vector-instruction issue).  `bound` / `fam_desc`
// may be null: k_col_bound has written them (the chunked schedule needs the scan of ALL bounds before the first column kernel).
// The body of the record kernel for ONE wavefront: families g0 .. g0 + nf - 1 (nf <= 32), round after round of up to 64 records; `Wv` = SP_WAVE_LDS
// bytes of LDS for the wavefront's windows, `sTagCls` the aux type classes (fill_tag_classes).  `after_round(fa, fb)` runs when the descriptors
// of the round's families g0 + fa .. g0 + fb - 1 have been written (round 6: the experiment k_split_fused decided the families' columns right there —
// slower than two kernels on two streams, removed, profiles/r06_experiments.md; k_split_parse passes a hook that does nothing).
template <class AfterRound>
__device__ __forceinline__ void s2_parse_wave(const FastParams& P, const uint32_t g0, const uint32_t nf, uint8_t* const Wv, const uint8_t* const sTagCls,
                                              uint64_t* __restrict__ bound, const uint32_t max_ends, uint4* __restrict__ fam_desc, AfterRound&& after_round) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const uint32_t lane = threadIdx.x & 63;
  uint8_t* const Wh = Wv + lane * SP_LANE;                             // this lane's head window; its tag window follows
  uint8_t* const Wa = Wh + SP_HEAD;
  const uint32_t gf = P.grp_first[g0 + (lane < nf ? lane : nf)];       // lane i <= nf: the record index where family g0 + i starts
  const unsigned long long below = (1ull << lane) - 1ull;
  SplitRec* const out_rec = P.split_rec;
  SplitFam* const out_fam = P.split_fam;

  uint32_t fa = 0;
  while (fa < nf) {
    // ---- the round: families fa .. fb - 1, as many as fit 64 lanes (one at least) -------------------------------------------
    const uint32_t ra = rlane(gf, fa);
    uint32_t fb = fa + 1;
    while (fb < nf) {
      const uint32_t nx = rlane(gf, fb + 1), cur = rlane(gf, fb);
      if (nx < cur || nx - ra > 64u) break;
      fb++;
    }
    const uint32_t rb = rlane(gf, fb);
    const uint32_t nrec = rb >= ra ? rb - ra : 0u;
    if (nrec > 64u) {
      // ---- one family of more than 64 records (fb == fa + 1): k_family's; only its column bound and byte-span descriptor -------
      const uint32_t g = g0 + fa;
      uint32_t mx = 0;
      for (uint32_t i = lane; i < nrec; i += 64) { const uint32_t l = P.rec_len[ra + i]; mx = l > mx ? l : mx; }
      mx = uni(wave_max(mx));
      if (lane == 0) {
        const uint32_t lb = mx > 33 ? (mx - 33) * 2 / 3 + 1 : 1;
        const uint32_t ends = nrec < max_ends ? nrec : max_ends;
        if (bound) {
          bound[g] = (uint64_t)ends * lb + COL_BOUND_PAD;
          const uint64_t lo = P.rec_off[ra], hi = P.rec_off[rb - 1] + P.rec_len[rb - 1];
          const uint32_t span = (hi >= lo && hi - lo < 0xFFFFFFFFull) ? (uint32_t)(hi - lo) : 0xFFFFFFFFu;
          fam_desc[g] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), span, nrec);
        }
        SplitFam F;
        memset(&F, 0, sizeof(F));
        out_fam[g] = F;
      }
    } else {   // (one call site of after_round below)
    const bool act = lane < nrec;
    const uint32_t r = ra + (act ? lane : 0u);
    // the family of this lane: fa + the number of boundaries at or below its record
    uint32_t fl = fa;
    for (uint32_t j = fa + 1; j < fb; j++) { const uint32_t gj = rlane(gf, j); fl += (act && r >= gj) ? 1u : 0u; }   // (the cross-lane read outside the short circuit: every lane takes part — tests/wavemu)
    const uint32_t seg_first = (uint32_t)__shfl((int)gf, (int)fl), seg_next = (uint32_t)__shfl((int)gf, (int)(fl + 1));
    const uint32_t seg_lo = act ? seg_first - ra : 0u;                  // first lane of the family
    const uint32_t n = act ? seg_next - seg_first : 0u;                 // its records (1 .. 64)
    const uint32_t sl = lane - seg_lo;                                  // this record's index in its family
    const uint32_t g = g0 + fl;
    const unsigned long long nmask = n >= 64u ? ~0ull : ((1ull << n) - 1ull);
    auto fbal = [&](bool p) -> unsigned long long { return (__ballot(p) >> seg_lo) & nmask; };   // the family's part of a ballot, bit i = its record i
    auto fbc = [&](uint32_t v, uint32_t s) -> uint32_t { return (uint32_t)__shfl((int)v, (int)(seg_lo + s)); };   // value of the family's record s

    // ---- parse (the record rules: record_core.h; the bytes come through the two LDS windows) -------------------------------------
    const unsigned long long off = act ? P.rec_off[r] : 0ull;
    const uint32_t len = act ? P.rec_len[r] : 0u;
    bool odd = false;
    if (act && (len < 36u || len > 0xFFFFu || off > P.blob_len || (unsigned long long)len > P.blob_len - off)) odd = true;
    const bool live = act && !odd;
    const uint8_t* const rec = P.blob + (live ? off : 0ull);
    u32x4 hp[2 + SP_HEAD / 16];                                  // [0], [1]: the fixed header (registers only); the rest goes to the head window
#pragma unroll
    for (uint32_t u = 0; u < 2 + SP_HEAD / 16; u++) { u32x4 x = {0, 0, 0, 0}; if (live && 16u * u < len) __builtin_memcpy(&x, rec + 16 * u, 16); hp[u] = x; }
#pragma unroll
    for (uint32_t u = 0; u < SP_HEAD / 16; u++) *(u32x4*)(Wh + 16 * u) = hp[2 + u];
    uint32_t flags = 0, l_seq = 0, seq_rel = 0, name_len = 0, clip = 0, hash = 0;
    int32_t pos = 0, ref_id = 0;
    uint32_t mi_rel = 0, mi_len = 0, rx_rel = 0, rx_len = 0, cb_rel = 0, cb_len = 0;
    bool has_mi = false, has_rx = false, has_cb = false;
    // the fixed header, from the registers (a record that is not live: zeros)
    const record::FixedHeader H = record::decode_header(hp[0].x, hp[0].y, hp[0].z, hp[0].w, hp[1].x);
    const record::MateFields M = record::decode_mate(hp[1].y, hp[1].z);
    const uint32_t l_name = H.l_name;
    const bool unm = live && (H.flags & bam::F_UNMAPPED);   // an unmapped record: a read without a CIGAR — l_seq query bases, ref_id / pos unused
    uint32_t aux_rel = 0, aux_len = 0;
    if (live) {
      l_seq = H.l_seq; flags = H.flags;
      const record::Layout lay = record::layout(H, len);
      if (lay.odd || record::streaming_header_odd(H, 1u, true, SP_HEAD)) odd = true;   // (a name beyond the head window: rare, k_simplex_wave2's)
      else { aux_rel = lay.aux_off; aux_len = len - aux_rel; seq_rel = lay.seq_off; name_len = l_name - 1; }
    }
    const bool parse = live && !odd;
    const bool aux_in_lds = aux_len <= SP_AUX;
    {   // the tag window (a block that does not fit is walked in global memory below)
      u32x4 ap[SP_AUX / 16];
#pragma unroll
      for (uint32_t u = 0; u < SP_AUX / 16; u++) { u32x4 x = {0, 0, 0, 0}; if (parse && aux_in_lds && 16u * u < aux_len) __builtin_memcpy(&x, rec + aux_rel + 16 * u, 16); ap[u] = x; }
#pragma unroll
      for (uint32_t u = 0; u < SP_AUX / 16; u++) *(u32x4*)(Wa + 16 * u) = ap[u];
    }
    wave_sync();
    if (parse) {
      ref_id = unm ? unmapped_ref_key(lane) : H.ref_id; pos = H.pos;   // (no shared span with an unmapped member: `ov_cnt` stays 0 below)
      if (record::streaming_flags_odd(H, true)) odd = true;
      if (!unm && !record::single_block_op(ld32u(Wh, l_name), l_seq)) odd = true;
      // aux walk (tags.rs:13-34): first occurrence of MC / <tag> / RX / <cell tag>; value offsets relative to the tag block
      AuxTags ax;
      if (aux_in_lds) aux_walk(Wa, sTagCls, 0u, aux_len, P, ax);
      else aux_walk(rec + aux_rel, sTagCls, 0u, aux_len, P, ax);
      if (ax.oddw) odd = true;
      const record::TagFields tg = record::unpack_tags(ax);
      has_mi = tg.has_mi; mi_rel = aux_rel + tg.mi_lo; mi_len = tg.mi_len;
      has_rx = tg.has_rx; rx_rel = aux_rel + tg.rx_lo; rx_len = tg.rx_len;
      has_cb = tg.has_cb; cb_rel = aux_rel + tg.cb_lo; cb_len = tg.cb_len;
      if (!odd && tg.has_mc && !(flags & (bam::F_UNMAPPED | bam::F_MATE_UNMAPPED))) {   // (either of them: no clip, whatever MC says)
        // this read and its mate are both one M op, the mate in [0, 2^30): the closed form; anything else is not this kernel's
        const uint32_t ML = record::mc_single_m(tg.mc_len, [&]() { return aux_in_lds ? ld64u(Wa, tg.mc_lo) : gld64(rec + aux_rel + tg.mc_lo); });
        if (ML == 0 || !record::mate_in_range(M)) odd = true;
        else clip = record::single_m_mate_clip(H, ref_id, M, (int32_t)ML);        // <= l_seq <= 65535
      }
      if (!odd) hash = record::name_hash30(name_len, [&](uint32_t o) { return ld32u(Wh, o); }, [&](uint32_t o) { return ld64u(Wh, o); });
    }
    if (act && sl == 0 && !odd && record::first_record_odd(has_mi, mi_len, P.prefix_len)) odd = true;
    if (act && !odd && (mi_len > 255 || rx_len > 255 || cb_len > 255)) odd = true;
    const bool rev = (flags & bam::F_REVERSE) != 0;
    const uint32_t ty = (!act || odd) ? 0u : (flags & bam::F_FIRST) ? 1u : (flags & bam::F_LAST) ? 2u : 0u;
    const uint32_t cls = ty == 2u ? 1u : 0u;                            // end A (fragments or R1s) / end B (R2s)
    // the family's first record: its offset (body offsets of the family are kept relative to it) and its RX value
    const uint32_t off_lo = (uint32_t)off, off_hi = (uint32_t)(off >> 32);
    const unsigned long long off0 = (unsigned long long)fbc(off_lo, 0) | ((unsigned long long)fbc(off_hi, 0) << 32);
    if (act && !odd && (off < off0 || off - off0 > 0x7FFF0000ull)) odd = true;

    // ---- one rotation over the family: mate candidates by name hash, and what the family's records have in common ------------
    const uint32_t kh = (hash << 2) | ty;
    const uint32_t inf = l_seq | (cls << 16) | ((rev ? 1u : 0u) << 17);
    const uint32_t nmax = uni(wave_max(n));
    int cmate = -1, clater = -1;
    uint32_t max_a = cls == 0u ? l_seq : 0u, max_b = cls == 1u ? l_seq : 0u, max_len = len;
    bool irregular = false;
    for (uint32_t k = 1; k < nmax; k++) {
      const uint32_t up = sl + k;
      const bool wrap = up >= n, inrange = k < n;
      const uint32_t s = wrap ? up - n : up;
      const uint32_t src = seg_lo + (inrange ? s : sl);
      const uint32_t okh = (uint32_t)__shfl((int)kh, (int)src), oinf = (uint32_t)__shfl((int)inf, (int)src), olen = (uint32_t)__shfl((int)len, (int)src);
      const uint32_t d = okh ^ kh;
      const int as_later = (d == 0 && !wrap && inrange) ? (int)s : -1;   // a later R1 of this name
      const int as_mate = (d == 3 && inrange) ? (int)s : -1;
      clater = as_later > clater ? as_later : clater;
      cmate = as_mate > cmate ? as_mate : cmate;
      const uint32_t ol = oinf & 0xFFFF, ocls = (oinf >> 16) & 1u, orev = (oinf >> 17) & 1u;
      if (inrange) {
        if (ocls == 0u) max_a = ol > max_a ? ol : max_a; else max_b = ol > max_b ? ol : max_b;
        max_len = olen > max_len ? olen : max_len;
        if (ocls == cls && (orev != (rev ? 1u : 0u) || (rev && ol != l_seq))) irregular = true;   // an end is one strand; a reverse end one length
      }
    }
    if (ty != 1u || !P.overlap) { cmate = -1; clater = -1; }
    int mate = -1;
    bool collide = false;
    {
      const int other = clater >= 0 ? clater : cmate;
      const uint32_t osl = other >= 0 ? (uint32_t)other : sl;
      const uint32_t onl = fbc(name_len, osl);
      if (other >= 0) {
        bool same = onl == name_len;
        const uint8_t* const Wo = Wv + (seg_lo + osl) * SP_LANE;     // the other record's head window
        for (uint32_t i = 0; i < name_len && same; i += 8) {
          unsigned long long wa = ld64u(Wo, i), wb = ld64u(Wh, i);
          if (i + 8 > name_len) { const unsigned long long mk = (1ULL << (8 * (name_len - i))) - 1; wa &= mk; wb &= mk; }
          if (wa != wb) same = false;
        }
        if (!same) collide = true;                            // equal hashes, different names: the exact rules live in k_family_wave<0>
        else if (clater < 0) mate = cmate;
      }
    }
    // shared reference span of each pair, owned by its R1 lane (both reads are one M op: reference offsets are query offsets)
    const uint32_t msrc = mate >= 0 ? (uint32_t)mate : sl;
    const int32_t pos_b = (int32_t)fbc((uint32_t)pos, msrc), ref_b = (int32_t)fbc((uint32_t)ref_id, msrc);
    const uint32_t len_b = fbc(l_seq, msrc);
    uint32_t ov_cnt = 0, ov_off1 = 0, ov_off2 = 0;
    if (mate >= 0 && ref_id == ref_b) {
      const int32_t s1 = pos + 1, e1 = pos + (int32_t)l_seq, s2 = pos_b + 1, e2 = pos_b + (int32_t)len_b;
      const int32_t lox = s1 > s2 ? s1 : s2, hix = e1 < e2 ? e1 : e2;
      if (hix >= lox) { ov_cnt = (uint32_t)(hix - lox + 1); ov_off1 = (uint32_t)(lox - s1); ov_off2 = (uint32_t)(lox - s2); }
    }
    // do all pairs of the family share ONE geometry (count and offsets of the shared bases)?  k_split_cols then walks pairs x bases as one index space
    bool ov_uniform;
    {
      const unsigned long long ovm = fbal(act && ov_cnt != 0);
      const uint32_t fp = ovm ? (uint32_t)__builtin_ctzll(ovm) : 0u;
      const uint32_t key = ov_cnt | (ov_off1 << 16);
      const uint32_t k0 = fbc(key, fp), k1 = fbc(ov_off2, fp);
      const unsigned long long other_geometry = fbal(act && ov_cnt != 0 && (key != k0 || ov_off2 != k1));   // (every lane takes part in the ballot: families differ in `ovm`)
      ov_uniform = ovm != 0 && other_geometry == 0;
    }
    // ---- rows: end A's records first, then end B's, file order inside an end ---------------------------------------------------
    const unsigned long long in_a = fbal(act && cls == 0u), in_b = fbal(act && cls == 1u);
    const uint32_t m_a = (uint32_t)__popcll(in_a), m_b = (uint32_t)__popcll(in_b);
    const unsigned long long mine_below = (cls ? in_b : in_a) & ((1ull << sl) - 1ull);
    const uint32_t slot = (uint32_t)__popcll(mine_below) + (cls ? m_a : 0u);
    const uint32_t mate_slot = fbc(slot, msrc);
    // ---- UMIs: every record carries the same value, or none carries one --------------------------------------------------------
    const unsigned long long with_rx = fbal(act && has_rx);
    const uint32_t rx0_rel = fbc(rx_rel, 0), rx0_len = fbc(rx_len, 0);
    const uint32_t rx0_win = fbc((aux_in_lds ? 1u : 0u) | (aux_rel << 1), 0);    // the first record's tag block: in its window? where?
    bool rx_diff = false;
    if (act && !odd && has_rx && sl != 0) {
      if (rx_len != rx0_len) rx_diff = true;
      else if (aux_in_lds && (rx0_win & 1u)) {
        const uint8_t* const W0 = Wv + seg_lo * SP_LANE + SP_HEAD;     // the first record's tag window
        const uint32_t o0 = rx0_rel - (rx0_win >> 1), o1 = rx_rel - aux_rel;
        for (uint32_t i = 0; i < rx_len && !rx_diff; i += 8) {
          unsigned long long wa = ld64u(W0, o0 + i), wb = ld64u(Wa, o1 + i);
          if (i + 8 > rx_len) { const unsigned long long mk = (1ULL << (8 * (rx_len - i))) - 1; wa &= mk; wb &= mk; }
          if (wa != wb) rx_diff = true;
        }
      } else {
        const uint8_t* const r0p = P.blob + off0 + rx0_rel;
        const uint8_t* const rp = rec + rx_rel;
        for (uint32_t i = 0; i < rx_len && !rx_diff; i += 8) {
          unsigned long long wa = gld64(r0p + i), wb = gld64(rp + i);
          if (i + 8 > rx_len) { const unsigned long long mk = (1ULL << (8 * (rx_len - i))) - 1; wa &= mk; wb &= mk; }
          if (wa != wb) rx_diff = true;
        }
      }
    }
    // ---- family verdict -----------------------------------------------------------------------------------------------------------
    const bool f_odd = fbal(odd) != 0, f_coll = fbal(collide) != 0, f_irr = fbal(irregular) != 0, f_rxd = fbal(rx_diff) != 0;
    const bool f_frag = fbal(act && ty == 0u) != 0, f_pair = fbal(act && ty != 0u) != 0;
    const bool f_mix = mixed_unmapped_end(act, flags, fbal);   // drop_unmapped_if_any_mapped needs the final lengths: k_family_wave<0>'s
    const bool rx_all = with_rx == nmask, rx_none = with_rx == 0;
    const uint32_t maxl = max_a > max_b ? max_a : max_b;
    // row strides of the family's LDS tile: reads up to 160 bases share ONE pair of strides (k_split_cols has a build with them as
    // immediates), longer reads get their own
    const uint32_t qs = maxl <= 160u ? 160u : (maxl + 15u) & ~15u, ss = maxl <= 160u ? 80u : ((maxl + 1u) / 2u + 15u) & ~15u;
    const uint32_t qc = qs >> 4, sc = ss >> 4;
    const uint32_t need = n * (qs + ss);
    bool take = !f_odd && !f_coll && !f_irr && !f_rxd && !f_mix && !(f_frag && f_pair) && (rx_all || rx_none) && n >= 1u && maxl >= 1u;
    if (rx_all && rx0_len > (uint32_t)FAST_RX_CAP) take = false;
    if (P.max_reads >= 0 && ((long long)m_a > P.max_reads || (long long)m_b > P.max_reads)) take = false;   // --max-reads may bite: k_family_wave<0>
    if (need > 60000u || maxl > 4000u) take = false;
    // an end of more than 16 rows: a column of it that shows a second base travels to k_call_full as ceil(rows / 16) consecutive
    // observation items (FULL_ITEM_CONT, fastpath.h) — every family of up to 64 records in this shape stays here.  (Round 3 handed such
    // families to k_simplex_wave2: LDS for their whole records, three launches over growing slices, 0.9 ns per read on long-tail sizes.)
    if (P.dir_size && (m_a > 16u || m_b > 16u)) take = false;   // (direct records keep the limit: their packed depth sums are 16 bits per end)

    // ---- direct records: the exact bytes of the family's consensus records, BEFORE the column kernel runs (its lanes then write the
    //      records where they belong).  What decides a record's size beyond the tag lengths is the consensus length, i.e. the reads'
    //      final lengths — k_split_cols phases 2 - 4 (overlap pre-correction, mate clip, trailing-N / low-quality strip) restated for
    //      the 3' end of each read alone: lane = record walks back from the clip point until a base survives, looking at its mate's
    //      base where the position is shared.  k_split_cols checks its own sizes against these (dir_flags[0]).
    if (P.dir_size) {
      uint8_t* const Wm = Wv;                                 // 64 bytes of the (no longer needed) windows: R2 record -> 1 + its R1
      Wm[lane] = 0;
      wave_sync();                                            // (lanes talk through LDS here: without the fences the compiler may forward a lane's own 0)
      if (act && mate >= 0) Wm[seg_lo + (uint32_t)mate] = (uint8_t)(sl + 1u);
      wave_sync();
      const uint32_t pm = Wm[lane];
      const int partner = mate >= 0 ? mate : (int)pm - 1;
      const uint32_t psl = partner >= 0 ? (uint32_t)partner : sl;
      const uint32_t p_cnt = fbc(ov_cnt, psl), p_o1 = fbc(ov_off1, psl), p_o2 = fbc(ov_off2, psl);
      const uint32_t p_seq = fbc(seq_rel, psl), p_lseq = fbc(l_seq, psl), p_lo = fbc(off_lo, psl), p_hi = fbc(off_hi, psl);
      uint32_t wo = 0, mo = 0, wc = 0;                        // shared bases: first one in this read / in the mate, how many
      if (partner >= 0) { if (mate >= 0) { wo = ov_off1; mo = ov_off2; wc = ov_cnt; } else { wo = p_o2; mo = p_o1; wc = p_cnt; } }
      uint32_t fin = 0;
      if (act && take) {
        const uint8_t* const prec = P.blob + (((unsigned long long)p_hi << 32) | p_lo);
        const uint32_t qrel = seq_rel + ((l_seq + 1u) >> 1), pqrel = p_seq + ((p_lseq + 1u) >> 1);
        const uint32_t min_bq = P.min_input_bq & 0xFFu;
        uint32_t flr = l_seq > clip ? l_seq - clip : 0u;
        while (flr > 0) {
          const uint32_t idx = rev ? l_seq - flr : flr - 1u;
          uint32_t cc = ((uint32_t)rec[seq_rel + (idx >> 1)] >> ((~idx & 1u) << 2)) & 15u, qq = rec[qrel + idx];
          if (idx - wo < wc) {                                // a shared base: what the pre-correction leaves there (overlapping.rs:236-336)
            const uint32_t j = mo + (idx - wo);
            const uint32_t c2 = ((uint32_t)prec[p_seq + (j >> 1)] >> ((~j & 1u) << 2)) & 15u, q2 = prec[pqrel + j];
            if (cc != 15u && c2 != 15u) {
              if (cc == c2) { const uint32_t sm = qq + q2; qq = sm < 93u ? sm : 93u; }
              else {
                const int32_t d = (int32_t)qq - (int32_t)q2;
                const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
                cc = d == 0 ? 15u : d > 0 ? cc : c2;
                qq = ad < (uint32_t)FGX_MIN_PHRED ? (uint32_t)FGX_MIN_PHRED : ad;
              }
            }
          }
          if (cc != 15u && qq >= min_bq) break;
          flr--;
        }
        fin = flr;
      }
      // consensus length per end type (k_split_cols phase 5) and the record of each consensus read (k_split_finish's size formula)
      uint32_t clen[3] = {0, 0, 0}, rem_e[3] = {0, 0, 0}, fk_e[3] = {0, 0, 0};
      bool ok_e[3] = {false, false, false};
#pragma unroll
      for (uint32_t e = 0; e < 3; e++) {
        const bool mine = act && take && ty == e;
        const unsigned long long in_e = fbal(mine), kept = fbal(mine && fin > 0);
        const uint32_t cnt = (uint32_t)__popcll(in_e), rem = (uint32_t)__popcll(kept);
        const uint32_t fk = kept ? (uint32_t)__builtin_ctzll(kept) : 0u;
        const uint32_t f0 = fbc(fin, fk);
        const bool good = cnt != 0 && cnt >= P.min_reads && rem != 0 && rem >= P.min_reads;
        const unsigned long long other_len = fbal(mine && fin > 0 && fin != f0);
        const bool differs = good && other_len != 0;
        uint32_t cl = f0;
        if (__any(differs)) {                               // reads of one end with different final lengths (rare): a uniform walk over the family
          const uint32_t val = (mine && fin > 0) ? fin : 0u;
          uint32_t ge = 0, mx = 0;
          for (uint32_t k = 0; k < nmax; k++) {
            const uint32_t vk = fbc(val, k < n ? k : 0u);
            if (k < n && vk) { ge += vk >= fin ? 1u : 0u; mx = vk > mx ? vk : mx; }
          }
          if (P.min_reads == 1) { if (differs) cl = mx; }
          else {
            const uint32_t cand = (val && ge >= P.min_reads) ? fin : 0u;
            uint32_t mc = 0;
            for (uint32_t k = 0; k < nmax; k++) { const uint32_t vk = fbc(cand, k < n ? k : 0u); if (k < n) mc = vk > mc ? vk : mc; }
            if (differs) cl = mc;
          }
        }
        ok_e[e] = good; clen[e] = good ? cl : 0u; rem_e[e] = rem; fk_e[e] = fk;
      }
      const bool has_frag = ok_e[0], has_pair = ok_e[1] && ok_e[2];
      const uint32_t mi0 = fbc(mi_len, 0);
      auto rec_bytes = [&](uint32_t Lc, uint32_t fk, uint32_t kept_n) -> uint32_t {
        const bool hcb = P.cell0 && fbc(has_cb ? 1u : 0u, fk) != 0;
        const uint32_t cbl = fbc(cb_len, fk);
        const uint32_t nm = P.prefix_len + 1u + mi0;
        return 4u + 32u + nm + 1u + (Lc + 1u) / 2u + Lc + (3u + P.rg_len + 1u) + 4u + 4u + 7u + (P.per_base_tags ? 2u * (8u + 2u * Lc) : 0u) +
               (3u + mi0 + 1u) + (hcb ? 3u + cbl + 1u : 0u) + ((rx_all && kept_n) ? 3u + rx0_len + 1u : 0u);
      };
      const uint32_t sz_f = rec_bytes(clen[0], fk_e[0], rem_e[0]), sz_1 = rec_bytes(clen[1], fk_e[1], rem_e[1]), sz_2 = rec_bytes(clen[2], fk_e[2], rem_e[2]);
      const uint32_t dsize = !take ? 0u : has_frag ? sz_f : has_pair ? sz_1 + sz_2 : 0u;
      if (act && sl == 0) P.dir_size[g] = dsize;
    }

    if (act) {
      SplitRec R;
      R.body_off = (uint32_t)(off - off0);
      R.seq_rel = (uint16_t)seq_rel; R.l_seq = (uint16_t)l_seq; R.clip = (uint16_t)clip;
      R.ov_off1 = (uint16_t)ov_off1; R.ov_off2 = (uint16_t)ov_off2; R.ov_cnt = (uint16_t)ov_cnt;
      R.slot = (uint8_t)slot; R.mate_slot = (uint8_t)mate_slot;
      R.bits = (uint8_t)(ty | ((rev ? 1u : 0u) << 2) | ((has_cb ? 1u : 0u) << 3));
      R.cb_len = (uint8_t)cb_len; R.cb_rel = (uint16_t)cb_rel; R.mi_rel = (uint16_t)mi_rel;
      R.mi_len = (uint8_t)mi_len; R.rx_len = (uint8_t)rx_len; R.rx_rel = (uint16_t)rx_rel;
      R._pad = 0;
      out_rec[r] = R;
    }
    if (bound && act && sl == 0) {
      // column bound and byte-span descriptor, exactly k_col_bound's
      const uint32_t lb = max_len > 33 ? (max_len - 33) * 2 / 3 + 1 : 1;
      const uint32_t ends = n < max_ends ? n : max_ends;
      bound[g] = (uint64_t)ends * lb + COL_BOUND_PAD;
    }
    {
      const uint32_t last = n ? n - 1 : 0;
      const unsigned long long end = off + len;
      const unsigned long long hi = (unsigned long long)fbc((uint32_t)end, last) | ((unsigned long long)fbc((uint32_t)(end >> 32), last) << 32);
      // the strands of the two ends, from their first records (a regular end has one)
      const uint32_t fa_l = in_a ? (uint32_t)__builtin_ctzll(in_a) : 0u, fb_l = in_b ? (uint32_t)__builtin_ctzll(in_b) : 0u;
      const uint32_t ra_v = fbc(rev ? 1u : 0u, fa_l), rb_v = fbc(rev ? 1u : 0u, fb_l);
      if (act && sl == 0) {
        const uint32_t span = (hi >= off && hi - off < 0xFFFFFFFFull) ? (uint32_t)(hi - off) : 0xFFFFFFFFu;
        if (bound) fam_desc[g] = make_uint4((uint32_t)off, (uint32_t)(off >> 32), span, n);
        SplitFam F;
        F.flags = take ? 1u : 0u;
        F.need_bytes = need;
        F.qs = (uint16_t)qs; F.ss = (uint16_t)ss;
        F.n = (uint8_t)n; F.m_a = (uint8_t)m_a; F.m_b = (uint8_t)m_b; F.type_a = (uint8_t)((f_frag ? 0u : 1u) | (ov_uniform ? 2u : 0u));
        F.rev_a = (uint8_t)(in_a ? ra_v : 0u); F.rev_b = (uint8_t)(in_b ? rb_v : 0u);
        F.rx_len = (uint8_t)(rx_all ? rx0_len : 0u); F.rx_all = (uint8_t)(rx_all ? 1u : 0u);
        F.len_a = (uint16_t)(max_a < 65535u ? max_a : 65535u); F.len_b = (uint16_t)(max_b < 65535u ? max_b : 65535u);
        const uint32_t cpr = qc + sc;
        F.inv_cpr = cpr ? (16777216u + cpr - 1u) / cpr : 0u;
        F.qc = (uint16_t)qc; F.sc = (uint16_t)sc;
        out_fam[g] = F;
      }
    }
    // empty families of the round (no lane belongs to them): lane j stands for family fa + j
    {
      const uint32_t fj = fa + lane;
      const uint32_t a0 = (uint32_t)__shfl((int)gf, (int)(fj < nf ? fj : nf)), a1 = (uint32_t)__shfl((int)gf, (int)(fj + 1 <= nf ? fj + 1 : nf));
      if (fj < fb && a1 <= a0) {
        const uint32_t ge = g0 + fj;
        if (bound) { bound[ge] = 0; fam_desc[ge] = make_uint4(0u, 0u, 0xFFFFFFFFu, a1 == a0 ? 0u : a1 - a0); }
        SplitFam F;
        memset(&F, 0, sizeof(F));
        out_fam[ge] = F;
      }
    }
    }
    after_round(fa, fb);
    fa = fb;
  }
}
__global__ __launch_bounds__(128) void k_split_parse(FastParams P, uint32_t g_begin, uint32_t n_grp, uint32_t fpw, uint64_t* __restrict__ bound, uint32_t max_ends,
                                                     uint4* __restrict__ fam_desc) {
  __shared__ __align__(16) uint8_t sTagCls[256];
  __shared__ __align__(16) uint8_t sWin[2 * SP_WAVE_LDS];
  fill_tag_classes(sTagCls);
  __syncthreads();
  const uint32_t wave = uni((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const unsigned long long g0l = (unsigned long long)g_begin + (unsigned long long)wave * fpw;
  if (g0l >= n_grp) return;
  const uint32_t g0 = (uint32_t)g0l;
  const uint32_t nf = uni(n_grp - g0 < fpw ? n_grp - g0 : fpw);        // families of this wavefront (fpw <= 32: boundaries in lanes 0 .. nf)
  s2_parse_wave(P, g0, nf, sWin + (threadIdx.x >> 6) * SP_WAVE_LDS, sTagCls, bound, max_ends, fam_desc, [](uint32_t, uint32_t) {});
}

// -----------------------------------------------------------------------------------------------------------------------------
// k_split_cols — one wavefront per family, lane = record for the short record phases, lane = column for the rest
// -----------------------------------------------------------------------------------------------------------------------------
#if FGX_S2_PAIRS >= 256
#define S2_PAIR_OFF(q) ((q) << 4)
#else
#define S2_PAIR_OFF(q) (((q) < 93u ? (q) : 93u) << 4)
#endif
#ifndef FGX_S2_ABLATE
#define FGX_S2_ABLATE 0   /* profiling builds only: k_split_cols returns after phase FGX_S2_ABLATE (what the phase left is folded into one store,
                             so that it is not optimised away): the PMC instruction counts of two builds differ by one phase (tools/ablate_split.sh) */
#endif
#define S2_ABLATE_AFTER(k, sink) if (FGX_S2_ABLATE == (k)) { P.rec_sizes[slot0 + (lane & 1)] = (uint64_t)(sink); return; }
#ifndef FGX_S2_MIN_ITEMS
#define FGX_S2_MIN_ITEMS 8   /* room (FullItems) a family must find behind its tile in the wave's LDS slice */
#endif

// One observation of a lane's column (the names are k_split_cols's column-loop variables).  Hot: the lane has seen nothing yet or
// this very base only — one bit extract of the allow mask.  An observation of good quality that is not hot (a second distinct
// base; also an N or IUPAC code of good quality, which is no observation at all) marks the lane in the scalar mask `suspect`
// (two scalar instructions, no branch): such a column leaves for k_call_full with its observations, whatever the loop goes on
// to add to it.
#if FGX_S2_F32 && FGX_S2_FMASEL
#define S2_OBSERVE(q_, sb_, pr_) do { \
    const uint32_t w_q = (q_), w_c = ((uint32_t)(sb_) >> ish) & 15u; \
    const unsigned long long qm = __builtin_amdgcn_uicmp(w_q, min_bq, 35 /* uge */); \
    const unsigned long long bm = __builtin_amdgcn_uicmp(__builtin_amdgcn_ubfe(allow, w_c, 1u), 0u, 33 /* ne */); \
    suspect |= qm & ~bm; \
    const bool w_hit = __builtin_amdgcn_inverse_ballot_w64(qm & bm); \
    allow = w_hit ? 1u << w_c : allow; \
    const float w_sel = w_hit ? 1.0f : 0.0f; \
    const s2_f32x2 w_sel2 = {w_sel, w_sel}; \
    acc2 = __builtin_elementwise_fma((pr_), w_sel2, acc2);   /* pair * 1 + acc = the add, rounded once; pair * 0 + acc = acc (the table is finite) */ \
    cntf += w_sel; \
  } while (0)
#else
#define S2_OBSERVE(q_, sb_, pr_) do { \
    const uint32_t w_q = (q_), w_c = ((uint32_t)(sb_) >> ish) & 15u; \
    const unsigned long long qm = __builtin_amdgcn_uicmp(w_q, min_bq, 35 /* uge */); \
    const unsigned long long bm = __builtin_amdgcn_uicmp(__builtin_amdgcn_ubfe(allow, w_c, 1u), 0u, 33 /* ne */); \
    suspect |= qm & ~bm; \
    if (__builtin_amdgcn_inverse_ballot_w64(qm & bm)) { allow = 1u << w_c; n1++; S2_ADD(pr_); } \
  } while (0)
#endif
#if FGX_S2_F32
#define S2_ADD(pr_) do { acc2 += (pr_); } while (0)     /* one v_pk_add_f32: {w~, l~} += {correct, error_per_alt} */
#else
#define S2_ADD(pr_) do { kahan2(s1, c1, (pr_).x); kahan2(sR, cR, (pr_).y); } while (0)
#endif
// the table entries of a batch of qualities, loaded ahead of the observations that use them (the empty asm keeps the loads where
// they are written: sunk into the predicated blocks they would be waited for there, one by one)
#if FGX_S2_F32
typedef float s2_f32x2 __attribute__((ext_vector_type(2)));
#define S2_PAIR(pr_, q_) s2_f32x2 pr_ = *(const s2_f32x2*)(pairs + ((q_) << 3))
#else
#define S2_PAIR(pr_, q_) double2 pr_ = *(const double2*)(pairs + S2_PAIR_OFF(q_))
#endif
#define S2_PIN4(a_, b_, c_, d_) FGX_PIN("+v"(a_.x), "+v"(a_.y), "+v"(b_.x), "+v"(b_.y), "+v"(c_.x), "+v"(c_.y), "+v"(d_.x), "+v"(d_.y))
#define S2_PIN1(a_) FGX_PIN("+v"(a_.x), "+v"(a_.y))
// Round 5 — an observation WITHOUT sums, for an end of at least P.s2_nsafe rows (unanimous_cap_depth, gate_core.h: that many agreeing
// observations of any qualities at or above the floor are the cap).  The lane keeps the OR of the accepted base codes, their sum and their
// number: one base only  <=>  the OR is a single bit and the sum is count x OR (a code 0 of good quality — '=' — adds nothing to the OR
// and breaks the product: such a column leaves for k_call_full like one that shows a second base or an N / IUPAC code).  Six vector
// instructions and no scalar one, against twelve and three of S2_OBSERVE.
#define S2_OBSERVE_FAST(q_, sb_) do { \
    const uint32_t w_c = __builtin_amdgcn_ubfe((uint32_t)(sb_), ish, 4u); \
    const bool w_g = (uint32_t)(q_) >= min_bq; \
    const uint32_t w_t = w_g ? w_c : 0u; \
    f_or |= w_t; f_sum += w_t; f_cnt += w_g ? 1u : 0u; \
  } while (0)

// 16-bit halves: the per-end depth statistics of the direct records travel two to a register
typedef unsigned short s2_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t s2_pkmax(uint32_t a, uint32_t b) { s2_u16x2 x, y; __builtin_memcpy(&x, &a, 4); __builtin_memcpy(&y, &b, 4); x = __builtin_elementwise_max(x, y); uint32_t r; __builtin_memcpy(&r, &x, 4); return r; }
__device__ __forceinline__ uint32_t s2_pkmin(uint32_t a, uint32_t b) { s2_u16x2 x, y; __builtin_memcpy(&x, &a, 4); __builtin_memcpy(&y, &b, 4); x = __builtin_elementwise_min(x, y); uint32_t r; __builtin_memcpy(&r, &x, 4); return r; }
__device__ __forceinline__ void s2_st16(uint8_t* p, uint32_t v) { const uint16_t w = (uint16_t)v; __builtin_memcpy(p, &w, 2); }
// one consensus record written in place (DIRECT): offsets from the family's first output byte
struct S2DirRec { uint32_t base, Lc, type, fk, kept, o_seq, o_qual, o_rg, o_t3, o_cd, o_ce, o_mi, o_cb, o_rx, size, hcb, cbl; };

// (development) what the packed pass met, counted when FGX_S2_DEBUG=1: [0] runs tried, [1] runs it finished, [2] columns it sent to k_call_full,
// [3] runs without room for their items, [42] runs whose shape it does not take
__device__ uint32_t g_s2_dbg[64];
// The families the packed column pass takes (round 5: a kernel of its own, COLS = 1 below): every end of two or more rows has between
// nsafe (unanimous_cap_depth) and 16 rows (one k_call_full item holds a column's observations), and the eight-position groups of both ends fit the 64 lanes (reads of up to 256 bases).
constexpr uint32_t S2_PACKED_MAX_ROWS = 31;   // rows of an end the packed pass takes: its byte counters add 8 per observation (round 5: 16 — one k_call_full item per flagged column; round 6: two)
__device__ __forceinline__ bool s2_packed_shape(uint32_t m_a, uint32_t m_b, uint32_t len_a, uint32_t len_b, uint32_t nsafe) {
  const bool oa = m_a < 2u || (m_a >= nsafe && m_a <= S2_PACKED_MAX_ROWS), ob = m_b < 2u || (m_b >= nsafe && m_b <= S2_PACKED_MAX_ROWS);
  return oa && ob && ((len_a + 7u) >> 3) + ((len_b + 7u) >> 3) <= 64u;
}

// the packed build's scratch layout (see offA / offB in k_split_cols): end A behind S2_PAD_FRONT columns, end B sixteen columns behind end A's last group
constexpr uint32_t S2_PAD_FRONT = 8;
__host__ __device__ __forceinline__ uint32_t s2_padded_b(uint32_t lc_a) { return S2_PAD_FRONT + ((lc_a + 7u) & ~7u) + 16u; }
static_assert(COL_BOUND_PAD >= S2_PAD_FRONT + 7 + 16 + 7 + 8, "the column bound's padding covers the packed build's layout: 8 + r8(lc_a) + 16 + r8(lc_b) + 8 <= 2 lc + 2 + COL_BOUND_PAD");
// which tables a build keeps in LDS (f32 sums: the packed build the cap and t1 only, the classic builds the image up to the f64 pairs)
template <int COLS> struct S2SharedOf {
#if FGX_S2_F32
  typedef typename std::conditional<COLS == 1, S2Tiny, S2Head>::type type;
#else
  typedef S2Lds type;
#endif
};
typedef uint32_t s2_u32x4 __attribute__((ext_vector_type(4)));
// The kernel's FastParams read AGAIN from the kernarg segment, at the place of use (the packed build only).  The compiler loads every field of the
// by-value argument it needs anywhere in one go and keeps them live: ~40 scalar registers of pointers that the record and result phases use
// once each, which is what pushed the family's own uniforms into spill lanes (v_writelane / v_readlane on the vector pipe, the one this kernel
// is short of).  A scalar load where the field is used costs the scalar cache's latency, not a vector slot.  The pin keeps the compiler from
// merging the reads back into the one at the top.  k_split_cols's first argument IS the FastParams: offset 0 of the segment.
template <bool AGAIN> struct S2Args { static __device__ __forceinline__ const FastParams& of(const FastParams& P) { return P; } };
#if !defined(FGX_WAVEMU)
template <> struct S2Args<true> {
  static __device__ __forceinline__ const FGX_CONST_AS FastParams& of(const FastParams&) {
    const FGX_CONST_AS FastParams* k = (const FGX_CONST_AS FastParams*)__builtin_amdgcn_kernarg_segment_ptr();
    FGX_PIN("+s"(k));
    return *k;
  }
};
#endif
// ONE family through the column kernel (round 6: a function of its own; FUSED — the tables are in LDS already, nothing of the workgroup is waited
// for — served the experiment k_split_fused, a wavefront that parsed a round of records and then decided the round's families: profiles/r06_experiments.md).
template <int QS_T, int SS_T, int DIRECT, int COLS, bool FUSED>   // row strides of the quality / sequence tiles (0, 0: the family's own, from its descriptor); DIRECT 1: the
                                            // family's consensus records are written here, at the offsets k_split_parse's sizes gave (fastpath.h).
                                            // COLS 0: every family, 64 columns per pass (run_cols); COLS 1: the families of s2_packed_shape, the packed
                                            // pass only; COLS 2: run_cols for every OTHER family (the two are launched over the same families, each
                                            // leaves the other's alone: the packed pass in a kernel of its own keeps its registers, and run_cols its)
__device__ __forceinline__ void s2_cols_family(const FastParams& P, const uint32_t g, bool bail, const uint32_t tiny_w, const s2_u32x4* const im, uint8_t* const W,
                                               typename S2SharedOf<COLS>::type& sL, const uint32_t lane, const uint32_t my_list) {
  typedef typename S2SharedOf<COLS>::type S2Shared;
  typedef s2_u32x4 u32x4;
  auto& sT = sL.g;
  constexpr bool TINY = FGX_S2_F32 && COLS == 1;          // the packed build reads the cap and S2Lds::t1 only
  constexpr uint32_t IMG_V = TINY ? 0u : (uint32_t)((FGX_S2_F32 ? S2_HEAD_BYTES : (uint32_t)sizeof(S2Lds)) / 16);   // (f32 sums: the gate tables and the f32 pairs only)
  const unsigned long long below = (1ull << lane) - 1ull;
  (void)sT; (void)IMG_V; (void)tiny_w; (void)im; (void)below;
  typedef S2Args<COLS == 1 && !FUSED> KA;     // KA::of(P).field: the packed build reads the field from the kernarg segment right there

  const uint4 fd = P.fam_desc[g];
  const u32x4 f0 = ((const u32x4*)&P.split_fam[g])[0], f1 = ((const u32x4*)&P.split_fam[g])[1];
  const uint64_t col_base_early = DIRECT ? 0ull : P.col_base[g];
  const uint64_t dir_off_ld = DIRECT ? P.dir_off[g] : 0ull;
  const uint32_t dir_size_ld = DIRECT ? P.dir_size[g] : 0u;
  const uint32_t r0 = P.grp_first[g], n = uni(fd.w);
  const uint32_t slot0 = 3 * g;
  // what this wavefront leaves for k_split_finish: one 32-byte result (status 0 = the family is another kernel's)
  auto leave = [&](uint32_t status, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t w5, uint32_t w6) {
    if (lane == 0) {
      u32x4* o = (u32x4*)&KA::of(P).split_out[g];
      const u32x4 a = {status | w1, w2, w3, w4}, b = {w5, w6, 0u, 0u};
      o[0] = a; o[1] = b;
    }
  };
  const uint64_t dir_off_early = uniform_u64(dir_off_ld);      // (the same in every lane: scalars from here on)
  const uint32_t dir_size_early = uni(dir_size_ld);
  // DIRECT: the family's three slots in the offset / size tables (what the scan of the record sizes gives the scratch path)
  auto dir_tables = [&](uint32_t s0, uint32_t s1, uint32_t s2) {
    if (lane < 3) {
      const uint32_t sz = lane == 0 ? s0 : lane == 1 ? s1 : s2, before = lane == 0 ? 0u : lane == 1 ? s0 : s0 + s1;
      P.out_off[slot0 + lane] = dir_off_early + before; P.rec_sizes[slot0 + lane] = sz;
    }
  };
  if (!bail && n < P.min_reads) { leave(2u, 0, n << 24, 0, 0, 0, 0); if (DIRECT) dir_tables(0, 0, 0); bail = true; }   // simplex.rs:673-683: counted by k_split_finish
  // not this kernel's: k_simplex_wave2 decides (and hands on what is not its shape either)
  auto to_route = [&]() { leave(0u, 0, 0, 0, 0, 0, 0); if (lane == 0) { uint32_t k = atomicAdd(KA::of(P).n_route, 1u); KA::of(P).route[k] = g; } };
  // fits the shape but not this launch's LDS slice: the next launch of this kernel (bigger slices)
  auto to_retry = [&]() { if (!KA::of(P).retry) { to_route(); return; } leave(0u, 0, 0, 0, 0, 0, 0); if (lane == 0) { uint32_t k = atomicAdd(KA::of(P).n_retry, 1u); KA::of(P).retry[k] = g; } };
  // SplitFam: flags | need_bytes | qs, ss | n, m_a, m_b, type_a || rev_a, rev_b, rx_len, rx_all | len_a, len_b | inv_cpr | qc, sc
  const uint32_t f_flags = uni(f0.x), need = uni(f0.y);
  const uint32_t QS = QS_T ? (uint32_t)QS_T : uni(f0.z & 0xFFFF), SS = SS_T ? (uint32_t)SS_T : uni(f0.z >> 16);
  const uint32_t m_a = uni((f0.w >> 8) & 0xFF), m_b = uni((f0.w >> 16) & 0xFF);
  const bool ov_uniform = (uni(f0.w >> 24) & 2u) != 0;        // every pair of the family shares one overlap geometry
  const uint32_t rev_a = uni(f1.x & 0xFF), rev_b = uni((f1.x >> 8) & 0xFF), rx_ulen = uni((f1.x >> 16) & 0xFF), rx_all = uni(f1.x >> 24);
  const uint32_t len_a = uni(f1.y & 0xFFFF), len_b = uni(f1.y >> 16), inv_cpr = uni(f1.z), qc = uni(f1.w & 0xFFFF), sc = uni(f1.w >> 16);
  if constexpr (COLS != 0) {   // (before anything is written: the family is the partner launch's)
    const bool mine = s2_packed_shape(m_a, m_b, len_a, len_b, P.s2_nsafe) == (COLS == 1);
    if (!bail && !mine) { if (COLS == 1 && !P.s2_partner) to_retry(); bail = true; }   // (no partner launch — the batch's sample showed this shape only —: the next launch takes it)
  }
  if (!bail && n > 64u && KA::of(P).big) { leave(0u, 0, 0, 0, 0, 0, 0); if (lane == 0) { uint32_t k = atomicAdd(KA::of(P).n_big, 1u); KA::of(P).big[k] = g; } bail = true; }   // k_family's, directly
  if (!bail && (!(f_flags & 1u) || n > 64u)) { to_route(); bail = true; }
  if (!bail && QS_T && ((f0.z & 0xFFFF) != (uint32_t)QS_T || (f0.z >> 16) != (uint32_t)SS_T)) { to_retry(); bail = true; }   // other strides: the generic build
  const uint32_t ibase = need + 16;
  const uint32_t tmp_bytes = 8u * n, min_tail = tmp_bytes > FGX_S2_MIN_ITEMS * (uint32_t)sizeof(FullItem) ? tmp_bytes : FGX_S2_MIN_ITEMS * (uint32_t)sizeof(FullItem);
  if (!bail && ibase + min_tail > P.lds_wave_bytes) { to_retry(); bail = true; }
  const uint32_t icap = uni(bail ? 0u : (P.lds_wave_bytes - ibase) / (uint32_t)sizeof(FullItem));
  uint32_t icnt = 0;
  static_assert(sizeof(FullItem) == 48, "FullItem is moved as three 16-byte pieces");

#if FGX_PHASE_TIMING
  unsigned long long _t = __builtin_amdgcn_s_memtime();
#endif
  // ---- 1. the records' descriptors (lane = record) and the family's bytes -----------------------------------------------------
  const bool act = !bail && lane < n;
  u32x4 d0 = {0, 0, 0, 0}, d1 = {0, 0, 0, 0};
  if (act) { const u32x4* rp = (const u32x4*)&P.split_rec[r0 + lane]; d0 = rp[0]; d1 = rp[1]; }
  if constexpr (!FUSED) {   // (the fused kernel has its tables in LDS before the first family)
    if constexpr (TINY) {
      if (threadIdx.x < 24u) ((uint32_t*)&sL.t1[0])[threadIdx.x] = tiny_w;
      else if (threadIdx.x == 24u) sL.g.cap = tiny_w;
    } else {
      u32x4* const img_dst = (u32x4*)&sL;
#pragma unroll
      for (int u = 0; u < 6; u++) { const uint32_t ii = threadIdx.x + u * blockDim.x; if (ii < IMG_V) img_dst[ii] = im[u]; }
    }
  }
  // SplitRec: body_off | seq_rel, l_seq | clip, ov_off1 | ov_off2, ov_cnt || slot, mate_slot, bits, cb_len | cb_rel, mi_rel | mi_len, rx_len, rx_rel | pad
  const uint32_t body_off = d0.x, seq_rel = d0.y & 0xFFFF, l_seq = d0.y >> 16, clip = d0.z & 0xFFFF, ov_off1 = d0.z >> 16;
  const uint32_t ov_off2 = d0.w & 0xFFFF, ov_cnt = d0.w >> 16;
  const uint32_t slot = d1.x & 0xFF, mate_slot = (d1.x >> 8) & 0xFF, bits = (d1.x >> 16) & 0xFF, cb_len = d1.x >> 24;
  const uint32_t cb_rel = d1.y & 0xFFFF, mi_rel = d1.y >> 16, mi_len = d1.z & 0xFF, rx_rel = d1.z >> 16;
  const uint32_t ty = bits & 3u;
  const bool rev = (bits & 4u) != 0, has_cb = (bits & 8u) != 0;
  const unsigned long long lo_off = uniform_u64((unsigned long long)fd.x | ((unsigned long long)fd.y << 32));
  const uint8_t* const fbase = P.blob + lo_off;
  // tile: quality rows [0, n * QS), sequence rows [S0, S0 + n * SS); behind it (from ibase) first the row table of the staging
  // loop, later the FullItems of the columns that need k_call_full
  const uint32_t S0 = n * QS;
  if (act) *(uint2*)(W + ibase + 8u * slot) = make_uint2(body_off + seq_rel, l_seq);
  if constexpr (FUSED) wave_sync(); else __syncthreads();     // the tables (workgroup); the row table (this wavefront)
  if (bail) return;
  {
    const uint32_t cpr = qc + sc, total = n * cpr;
    for (uint32_t t0 = 0; t0 < total; t0 += 256) {
      u32x4 v[4];
      uint32_t dst[4];
      bool on[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint32_t t = t0 + 64u * u + lane;
        const bool in = t < total;
        const uint32_t tt = in ? t : 0u;
        const uint32_t row = s2_mul24(tt, inv_cpr) >> 24;        // (tt < 64 rows x chunks per row, inv_cpr <= 2^23: the 24-bit multiply is a full-rate instruction)
        const uint32_t ch = tt - s2_mul24(row, cpr);
        const uint2 e = *(const uint2*)(W + ibase + 8u * row);   // {SEQ offset from the family's first body, l_seq}
        const bool isq = ch < qc;
        const uint32_t c = isq ? ch : ch - qc;
        const uint32_t sbytes = (e.y + 1u) >> 1;
        const uint32_t src = e.x + (isq ? sbytes : 0u) + 16u * c;
        dst[u] = (isq ? row * QS : S0 + row * SS) + 16u * c;
        on[u] = in;
        const bool need_ld = in && 16u * c < (isq ? e.y : sbytes);      // (rows are as wide as the longest read; a chunk past this read is zeros)
        u32x4 x = {0, 0, 0, 0};
        if (need_ld) __builtin_memcpy(&x, fbase + src, 16);
        v[u] = x;
      }
#pragma unroll
      for (int u = 0; u < 4; u++) if (on[u]) *(u32x4*)(W + dst[u]) = v[u];
    }
  }
  wave_sync();
  PH(1)
  const uint32_t my_q = slot * QS, my_s = S0 + slot * SS;           // this record's rows
  if (__any(act && W[my_q] == 0xFF)) { to_route(); return; }        // absent qualities (vanilla_caller.rs:1119-1124): the general rules live further down the chain
  S2_ABLATE_AFTER(1, W[my_s])
  const uint32_t min_bq = uni((uint32_t)P.min_input_bq & 0xFFu);

  // ---- 1b. (packed build, round 7) CLEAN rows: is every raw quality of the family, at the positions below its read's own length, at or
  //          above --min-input-base-quality?  Then every sub-floor quality the column pass meets was written by the overlap step below,
  //          together with code 0 (`drop`), and the pass needs no quality at all (packed_core.h, acc_row_seq).  The layout is the column
  //          pass's: a lane takes group k of its end, over ALL rows of both ends (known from SplitFam before the gates).  What lies at or
  //          past l_seq is never looked at: the last 16-byte chunk of a quality row carries tag text, NULs included.
  uint32_t dirty_v = 1u;          // per lane: its group holds a raw quality below the floor (or the test did not run).  A VECTOR register on purpose:
                                  // the one bit is needed again in phase 6, and the scalar file is what this kernel is short of (its uniforms spill)
  if constexpr (COLS == 1) {
    if ((P.s2_packed & 4u) && min_bq <= 128u) {
      const uint32_t ga = m_a ? (len_a + 7u) >> 3 : 0u, gb = m_b ? (len_b + 7u) >> 3 : 0u;      // (ga + gb <= 64: s2_packed_shape)
      const bool inl = lane < ga + gb, in_b = inl && lane >= ga;
      const uint32_t k = inl ? (in_b ? lane - ga : lane) : 0u;
      const uint32_t rowE = in_b ? m_a : 0u, rows = inl ? (in_b ? m_b : m_a) : 0u;
      const uint32_t m_lo = !m_b ? m_a : !m_a ? m_b : (m_a < m_b ? m_a : m_b), m_hi = m_a > m_b ? m_a : m_b;
      const uint32_t mb4 = min_bq * 0x01010101u;
      uint32_t qj = s2_mul24(rowE, QS) + 8u * k, j = 0;
      pk::Below Z;
      pk::below_reset(Z);
      bool dirty;
      if (__all(!act || l_seq == (ty == 2u ? len_b : len_a))) {
        // every read as long as its end's rows (the usual family): the length masks once, behind the last row
        for (; j + 4 <= m_lo; j += 4, qj += 4 * QS) {
          const uint2 q0 = *(const uint2*)(W + qj), q1 = *(const uint2*)(W + qj + QS), q2 = *(const uint2*)(W + qj + 2 * QS), q3 = *(const uint2*)(W + qj + 3 * QS);
          pk::below_row(Z, q0.x, q0.y, mb4); pk::below_row(Z, q1.x, q1.y, mb4); pk::below_row(Z, q2.x, q2.y, mb4); pk::below_row(Z, q3.x, q3.y, mb4);
        }
        for (; j < m_hi; j++, qj += QS) if (j < rows) { const uint2 q0 = *(const uint2*)(W + qj); pk::below_row(Z, q0.x, q0.y, mb4); }
        uint32_t nfl, nfh;
        pk::count_masks(in_b ? len_b : len_a, k, &nfl, &nfh);
        dirty = pk::below_any(Z, nfl, nfh);
      } else {
        // reads of several lengths: each row with its own (the row table of the staging loop still stands)
        for (; j < m_hi; j++, qj += QS)
          if (j < rows) { const uint2 q0 = *(const uint2*)(W + qj); pk::below_row_len(Z, q0.x, q0.y, mb4, *(const uint32_t*)(W + ibase + 8u * (rowE + j) + 4u), k); }
        dirty = pk::below_any(Z, pk::H, pk::H);
      }
      dirty_v = (inl && dirty) ? 1u : 0u;
    }
    FGX_PIN("+v"(dirty_v));
  }

  // ---- 2. overlapping-bases pre-correction in LDS (overlapping.rs:236-336, 627-684) -------------------------------------------
  uint32_t ov_agree = 0, ov_dis = 0, ov_corr = 0;             // (wave-uniform: counted with ballots byte by byte, summed over the wavefront once by the packed step)
  {
    // one shared base of a pair: o1 / o2 = sequence bytes, sh1 / sh2 = nibble shifts, q1 / q2 = quality bytes of the two reads.
    // Agreement: both qualities become min(qa + qb, 93).  Disagreement: the higher quality's base wins with the difference (at
    // least 2); a tie masks both (N, 2).  A changed base is ONE 32-bit LDS atomic — XOR with the (old ^ new) nibble: neighbouring
    // lanes own the other nibble of the same byte.
    auto shared_base = [&](const bool in, const uint32_t o1, const uint32_t o2, const uint32_t q1, const uint32_t q2, const uint32_t sh1, const uint32_t sh2) {
      // (every address is inside the tile also for a lane past the end of the index space — it computes position 0 —: the loads and the
      // arithmetic run unconditionally, only the stores are predicated; the three counts come from compare masks)
      const uint32_t c1 = ((uint32_t)W[o1] >> sh1) & 15, c2 = ((uint32_t)W[o2] >> sh2) & 15;
      const uint32_t qa = W[q1], qb = W[q2];
      const bool valid = in && (c1 > c2 ? c1 : c2) != 15;      // neither is N
      const bool agree = c1 == c2;
      const uint32_t sm = qa + qb, nq = sm < 93 ? sm : 93;
      const int32_t d = (int32_t)qa - (int32_t)qb;
      const uint32_t ad = (uint32_t)(d < 0 ? -d : d), dq = ad < FGX_MIN_PHRED ? (uint32_t)FGX_MIN_PHRED : ad;
      const uint32_t cb = d == 0 ? 15u : d > 0 ? c1 : c2;
      const uint32_t newq = agree ? nq : dq;
      // (round 5) a corrected base whose new quality is below --min-input-base-quality is no observation for anything that follows (every
      // reader of the tile tests the quality first; k_call_full skips such observations): its code becomes 0, so that the packed column
      // pass, which clears the codes of sub-floor qualities before it looks at them, finds nothing to clear in the usual family (a
      // disagreement of two mates leaves both with the DIFFERENCE of their qualities — below the floor nearly always)
      const bool drop = newq < min_bq;
      const uint32_t x1 = drop ? c1 : agree ? 0u : (c1 ^ cb), x2 = drop ? c2 : agree ? 0u : (c2 ^ cb);
      const bool changed = nq != qa || nq != qb;
      if (valid) {
        atomicXor((uint32_t*)(W + (o1 & ~3u)), x1 << (8 * (o1 & 3) + sh1));
        atomicXor((uint32_t*)(W + (o2 & ~3u)), x2 << (8 * (o2 & 3) + sh2));
        W[q1] = (uint8_t)newq; W[q2] = (uint8_t)newq;
      }
      const uint32_t na = (uint32_t)__popcll(__ballot(valid && agree)), nd = (uint32_t)__popcll(__ballot(valid && !agree));
      ov_agree += na; ov_dis += nd;
      ov_corr += (uint32_t)__popcll(__ballot(valid && agree && changed)) + 2u * nd;
    };
    const unsigned long long om = __ballot(act && ov_cnt != 0);
    if (om) {
      const uint32_t np = (uint32_t)__popcll(om), fp = (uint32_t)__builtin_ctzll(om);
      const uint32_t cn0 = rlane(ov_cnt, fp);
      bool ov_packed = false, ov_guard = false;
      if constexpr (COLS == 1) {
        // ---- 2a. (round 8) EIGHT shared bases per lane on packed words (packed_core.h, ov_step): pairs x groups of eight as one index space, 64
        //      per step — 8 pairs x 40 bases in one step, 8 x 150 in three.  For families of one geometry and two or more overlapping pairs (one
        //      pair of a few bases is cheaper byte by byte).  The groups are aligned to the mate whose offset is 0 (one of the two always is: the
        //      overlap starts at the later of the two starts) — its words are the lane's own and are stored as they are; the other mate's words
        //      are shared with the neighbouring group and get XOR deltas of the lane's own positions (LDS atomics: they compose in any order, and
        //      a lane that loads after a neighbour's delta finds its own positions untouched — no order between lanes or steps is needed).
        //      A quality of 128 or more at a shared position would carry between bytes: such a family is voted out BEFORE the first store (a
        //      family of several steps: in a pass over the qualities of its own) and takes the byte-wise steps below.
        const uint32_t oo1 = rlane(ov_off1, fp), oo2 = rlane(ov_off2, fp);
        if ((KA::of(P).s2_packed & 8u) && ov_uniform && np > 1u && (oo1 == 0u || oo2 == 0u) && ((QS & 7u) | (SS & 3u)) == 0u && min_bq <= 128u) {
          if (act && ov_cnt != 0) *(uint16_t*)(W + ibase + 2u * (uint32_t)__popcll(om & below)) = (uint16_t)(slot | (mate_slot << 8));   // pair -> its two rows
          wave_sync();
          const bool a_is_1 = oo1 == 0u;                         // the aligned mate ("A") is the pair's first row
          const uint32_t off = oo1 | oo2, sq = off & 3u, sn = off & 7u;   // the other mate ("B") starts here
          const uint32_t ng = (cn0 + 7u) >> 3, total = np * ng;  // (at most 31 pairs x 32 groups: s2_packed_shape)
          const uint32_t inv = uni((uint32_t)(1048576.0f / (float)ng) + 2u);    // (t * inv) >> 20 == t / ng for t < 32 * 64, as below
          const uint32_t mb4 = min_bq * 0x01010101u;
          // one lane's item: the addresses of A's words and of B's first aligned words, the in-range masks, the eight positions of both mates.
          // B's second sequence word and third quality dword may lie past its row — in the next row, or in the 16 bytes between the tile and
          // the pair table —: every position in them then lies past the read, is masked out of the arithmetic and gets a delta of 0.
          struct OvLane { uint32_t aq, as, bq, bs, ml, mh, qax, qay, caw, qbx, qby, cbp; };
          auto ov_load = [&](const uint32_t t0, OvLane& L) {
            const uint32_t t = t0 + lane;
            const bool in = t < total;
            const uint32_t tt = in ? t : 0u;                     // (a lane past the index space computes item 0 under empty masks and stores nothing)
            const uint32_t pi = s2_mul24(tt, inv) >> 20, k = tt - s2_mul24(pi, ng);
            const uint32_t rows = *(const uint16_t*)(W + ibase + 2u * pi), r1 = rows & 0xFF, r2 = rows >> 8;
            const uint32_t rA = a_is_1 ? r1 : r2, rB = a_is_1 ? r2 : r1;
            L.aq = rA * QS + 8u * k; L.as = S0 + rA * SS + 4u * k;
            L.bq = rB * QS + 4u * ((off >> 2) + 2u * k); L.bs = S0 + rB * SS + 4u * ((off >> 3) + k);
            pk::ov_in_masks(in ? cn0 : 0u, k, &L.ml, &L.mh);
            const uint2 qa = *(const uint2*)(W + L.aq);
            L.qax = qa.x; L.qay = qa.y; L.caw = *(const uint32_t*)(W + L.as);
            pk::ov_gather_q(*(const uint32_t*)(W + L.bq), *(const uint32_t*)(W + L.bq + 4u), *(const uint32_t*)(W + L.bq + 8u), sq, &L.qbx, &L.qby);
            L.cbp = pk::ov_gather_c(*(const uint32_t*)(W + L.bs), *(const uint32_t*)(W + L.bs + 4u), sn);
          };
          if (total > 64u) {
            uint32_t hi_v = 0;
            for (uint32_t t0 = 0; t0 < total; t0 += 64) { OvLane L; ov_load(t0, L); hi_v |= pk::ov_high(L.qax, L.qay, L.qbx, L.qby, L.ml, L.mh) ? 1u : 0u; }
            ov_guard = __any(hi_v != 0u);
          }
          if (!ov_guard) {
            uint32_t n_ad = 0, n_chg = 0;                        // per lane: agreements | disagreements << 16 (a family has fewer than 2^13 shared bases), changed agreements
            for (uint32_t t0 = 0; t0 < total; t0 += 64) {
              OvLane L;
              ov_load(t0, L);
              if (total <= 64u && __any(pk::ov_high(L.qax, L.qay, L.qbx, L.qby, L.ml, L.mh))) { ov_guard = true; break; }   // (the only step: nothing stored yet)
              pk::OvStep R;
              pk::ov_step(L.qax, L.qay, L.caw, L.qbx, L.qby, L.cbp, L.ml, L.mh, mb4, R);
              uint32_t e[3], f[2];
              pk::ov_scatter_q(R.dq[0], R.dq[1], sq, e); pk::ov_scatter_c(R.dc, sn, f);
              if (t0 + lane < total) {
                *(uint2*)(W + L.aq) = make_uint2(R.qa[0], R.qa[1]); *(uint32_t*)(W + L.as) = R.ca;
                atomicXor((uint32_t*)(W + L.bq), e[0]); atomicXor((uint32_t*)(W + L.bq + 4u), e[1]); atomicXor((uint32_t*)(W + L.bq + 8u), e[2]);
                atomicXor((uint32_t*)(W + L.bs), f[0]); atomicXor((uint32_t*)(W + L.bs + 4u), f[1]);
              }
              n_ad += R.n_ad; n_chg += R.n_chg;
            }
            if (!ov_guard) {
              const uint32_t t_ad = wave_sum(n_ad), t_chg = wave_sum(n_chg);
              ov_agree = t_ad & 0xFFFFu; ov_dis = t_ad >> 16; ov_corr = t_chg + 2u * ov_dis;
              ov_packed = true;
            }
          }
        }
      }
      if (ov_packed) {
        // (corrected above)
      } else if (ov_uniform && np > 1u && cn0 < 64u) {
        // ONE geometry for every pair: pairs x shared bases as one index space, 64 per step (8 pairs x 40 bases = 5 steps, not 8)
        const uint32_t oo1 = rlane(ov_off1, fp), oo2 = rlane(ov_off2, fp);
        if (act && ov_cnt != 0) *(uint16_t*)(W + ibase + 2u * (uint32_t)__popcll(om & below)) = (uint16_t)(slot | (mate_slot << 8));   // pair -> its two rows
        wave_sync();
        const uint32_t inv = uni((uint32_t)(1048576.0f / (float)cn0) + 2u);    // > 2^20 / cn0 by at most 2: (t * inv) >> 20 == t / cn0 for t < 32 * 64 (24-bit multiplies: full rate)
        const uint32_t total = np * cn0;
        for (uint32_t t0 = 0; t0 < total; t0 += 64) {
          const uint32_t t = t0 + lane;
          const bool in = t < total;
          const uint32_t tt = in ? t : 0u;
          const uint32_t pk = s2_mul24(tt, inv) >> 20, w = tt - s2_mul24(pk, cn0);
          const uint32_t rows = *(const uint16_t*)(W + ibase + 2u * pk), r1 = rows & 0xFF, r2 = rows >> 8;
          const uint32_t i1 = oo1 + w, i2 = oo2 + w;
          shared_base(in, S0 + r1 * SS + (i1 >> 1), S0 + r2 * SS + (i2 >> 1), r1 * QS + i1, r2 * QS + i2, (~i1 & 1) << 2, (~i2 & 1) << 2);
        }
      } else {
        // pair after pair, 64 shared bases per step
        const uint32_t mt_q = mate_slot * QS, mt_s = S0 + mate_slot * SS;
        const uint32_t my_q0 = slot * QS, my_s0 = S0 + slot * SS;
        for (unsigned long long pm = om; pm; pm &= pm - 1) {
          const uint32_t a = (uint32_t)__builtin_ctzll(pm);
          const uint32_t sa = rlane(my_s0, a), qa0 = rlane(my_q0, a), sb = rlane(mt_s, a), qb0 = rlane(mt_q, a);
          const uint32_t cn = rlane(ov_cnt, a);
          const uint32_t i1 = rlane(ov_off1, a) + lane, i2 = rlane(ov_off2, a) + lane;
          uint32_t o1 = sa + (i1 >> 1), o2 = sb + (i2 >> 1), q1 = qa0 + i1, q2 = qb0 + i2;
          const uint32_t sh1 = (~i1 & 1) << 2, sh2 = (~i2 & 1) << 2;
          for (uint32_t w0 = 0; w0 < cn; w0 += 64, o1 += 32, o2 += 32, q1 += 64, q2 += 64) shared_base(w0 + lane < cn, o1, o2, q1, q2, sh1, sh2);
        }
      }
      // (packed build) which step corrected the family, for k_split_finish's counters: in the top bits of ov_corr, a uniform that lives to the
      // family's result anyway (fastpath.h, S2_OV_*) — a register of its own would sit in a spill lane across the column pass
      if constexpr (COLS == 1) ov_corr |= ov_packed ? S2_OV_PACKED : ov_guard ? (S2_OV_BYTEWISE | S2_OV_GUARD) : S2_OV_BYTEWISE;
    }
  }
  const uint32_t ov_bases = ov_agree + ov_dis;
  wave_sync();
  PH(3)
  S2_ABLATE_AFTER(3, ov_bases + ov_corr + W[my_s])

  // ---- 3. what is not part of the source read becomes "no observation" (code 0): bases past the mate clip, and the row beyond a
  //         forward read that is shorter than its end's rows ---------------------------------------------------------------------
  const uint32_t fl = l_seq > clip ? l_seq - clip : 0u;      // length up to the mate clip (vanilla_caller.rs:1129-1160; no --trim in this shape)
  if (act) {
    uint32_t z0, z1;
    if (!rev) { z0 = fl; z1 = ty == 2u ? len_b : len_a; } else { z0 = 0; z1 = clip < l_seq ? clip : l_seq; }
    if (z0 < z1) {
      if (z0 & 1u) { W[my_s + (z0 >> 1)] &= 0xF0; z0++; }
      if (z0 < z1 && (z1 & 1u)) { W[my_s + (z1 >> 1)] &= 0x0F; z1--; }
      for (uint32_t b = z0 >> 1; b < (z1 >> 1); b++) W[my_s + b] = 0;
    }
  }
  // ---- 4. final length per read: without its trailing N / masked bases ----------------------------------------------------------
  uint32_t final_len = 0;
  if (act) {
    uint32_t flr = fl;
    while (flr > 0) {
      const uint32_t idx = rev ? l_seq - flr : flr - 1;
      const uint32_t c = ((uint32_t)W[my_s + (idx >> 1)] >> ((~idx & 1u) << 2)) & 15u, q = W[my_q + idx];
      if (c != 15u && q >= min_bq) break;
      flr--;
    }
    final_len = flr;
  }
  wave_sync();
  PH(4)
  S2_ABLATE_AFTER(4, final_len + ov_bases + ov_corr)

  // ---- 5. family gates with ballots (process_group :1329-1422, process_subgroup :1454-1646) -----------------------------------
  uint32_t rej = 0;        // rejected reads by reason, packed: insufficient | zero-length << 8 | orphan << 16 (each <= 64)
  const uint32_t my_end = act ? ty : 255u;
  bool ok[3] = {false, false, false};
  unsigned long long mem[3] = {0, 0, 0};
  uint32_t surv[3] = {0, 0, 0}, clen[3] = {0, 0, 0};
#pragma unroll
  for (uint32_t e = 0; e < 3; e++) {
    const unsigned long long in_e = __ballot(my_end == e);
    const uint32_t cnt = (uint32_t)__popcll(in_e);
    if (cnt == 0) continue;
    if (cnt < P.min_reads) { rej += cnt; continue; }
    const unsigned long long kept = __ballot(my_end == e && final_len > 0);
    const uint32_t rem = (uint32_t)__popcll(kept), zero = cnt - rem;
    rej += zero << 8;
    if (rem < P.min_reads) { rej += rem; continue; }
    if (rem == 0) continue;
    const bool mine = (kept >> lane) & 1;
    const uint32_t f0l = rlane(final_len, (uint32_t)__builtin_ctzll(kept));
    if (__all(!mine || final_len == f0l)) clen[e] = f0l;     // one final length (the usual family): it is the consensus length under either rule
    else if (P.min_reads == 1) clen[e] = uni(wave_max(mine ? final_len : 0));
    else {
      uint32_t ge = 0;
      for (unsigned long long m = kept; m; m &= m - 1) { const uint32_t fj = rlane(final_len, (uint32_t)__builtin_ctzll(m)); ge += (fj >= final_len) ? 1 : 0; }
      clen[e] = uni(wave_max((mine && ge >= P.min_reads) ? final_len : 0));
    }
    mem[e] = kept; surv[e] = rem; ok[e] = true;
  }
  const bool has_frag = ok[0], has_pair = ok[1] && ok[2];
  if (has_frag && (ok[1] || ok[2])) { to_route(); return; }   // (k_split_parse does not flag such a family; belt and braces)
  const uint32_t ne = has_frag ? 1u : has_pair ? 2u : 0u;
  if (!has_pair) { if (ok[1]) rej += surv[1] << 16; else if (ok[2]) rej += surv[2] << 16; }
  // end A = the fragment end or the R1 end (rows 0 .. m_a), end B = the R2 end (rows m_a .. m_a + m_b)
  const uint32_t type_a = has_frag ? 0u : 1u;
  const uint32_t lc_a = uni(ne ? (has_frag ? clen[0] : clen[1]) : 0u), lc_b = uni(ne == 2u ? clen[2] : 0u);
  const unsigned long long mem_a = uniform_u64(ne ? (has_frag ? mem[0] : mem[1]) : 0ull), mem_b = uniform_u64(ne == 2u ? mem[2] : 0ull);
  const uint32_t surv_a = (uint32_t)__popcll(mem_a), surv_b = (uint32_t)__popcll(mem_b);

  const uint32_t fk_a = mem_a ? (uint32_t)__builtin_ctzll(mem_a) : 0u, fk_b = mem_b ? (uint32_t)__builtin_ctzll(mem_b) : 0u;   // first retained read of each end
  // scratch columns of the two ends inside the family's slot.  The classic builds lay them back to back.  The packed build (round 6) leaves
  // room around them — eight columns in front of end A, sixteen between the ends, eight behind end B (the column bound carries COL_BOUND_PAD
  // for it) —: every lane of the packed pass then stores all eight slots of its group with the wide stores, also the group that straddles
  // an end of its end (a reverse end's first columns, any end's last ones: for 150-base reads one lane of each end in EVERY family, which sent
  // every wavefront through the 4 + 2 + 1 store path as well); what it writes beside the end lands in the padding.  SplitOut.status bit 7
  // tells k_split_finish which layout the family's EndDescs point into (bit 6, round 7: the packed pass ran its clean row loop).
  const uint32_t offA = COLS == 1 ? S2_PAD_FRONT : 0u, offB = COLS == 1 ? s2_padded_b(lc_a) : lc_a;
  // ---- 5b. DIRECT: where the family's records go and what they look like (all wave-uniform; vanilla_caller.rs:1767-1881) ---------
  S2DirRec RA, RB;
  __builtin_memset(&RA, 0, sizeof(RA)); __builtin_memset(&RB, 0, sizeof(RB));
  uint8_t* fam_out = nullptr;
  uint32_t d_nm = 0, d_mi0 = 0, d_mirel = 0;
  uint32_t acc_max = 0, acc_min = 0xFFFFFFFFu, acc_sum = 0;   // per-base depths of this lane's columns: end A in the low half, end B in the high half
  if constexpr (DIRECT != 0) {
    d_mi0 = rlane(mi_len, 0); d_mirel = rlane(mi_rel, 0);
    d_nm = P.prefix_len + 1u + d_mi0;
    auto layout = [&](S2DirRec& R, uint32_t base, uint32_t Lc, uint32_t type, uint32_t fk, uint32_t kept) {
      R.base = base; R.Lc = Lc; R.type = type; R.fk = fk; R.kept = kept;
      R.hcb = (P.cell0 && (rlane(bits, fk) & 8u)) ? 1u : 0u; R.cbl = rlane(cb_len, fk);
      R.o_seq = 36u + d_nm + 1u; R.o_qual = R.o_seq + ((Lc + 1u) >> 1); R.o_rg = R.o_qual + Lc; R.o_t3 = R.o_rg + 3u + P.rg_len + 1u;
      R.o_cd = R.o_t3 + 15u + 8u; R.o_ce = R.o_cd + 2u * Lc + 8u;                       // (the DATA of the cd / ce arrays; their 8-byte headers lie in front)
      R.o_mi = P.per_base_tags ? R.o_ce + 2u * Lc : R.o_t3 + 15u;
      R.o_cb = R.o_mi + 3u + d_mi0 + 1u; R.o_rx = R.o_cb + (R.hcb ? 3u + R.cbl + 1u : 0u);
      R.size = R.o_rx + ((rx_all && kept) ? 3u + rx_ulen + 1u : 0u);
    };
    if (ne >= 1u) layout(RA, 0u, lc_a, type_a, fk_a, surv_a);
    if (ne == 2u) layout(RB, RA.size, lc_b, 2u, fk_b, surv_b);
    const uint32_t total = RA.size + RB.size;
    if (total != dir_size_early) {           // k_split_parse predicted other records: nothing may be written (the host runs the batch again through the scratch path)
      if (lane == 0) atomicAdd(&P.dir_flags[0], 1u);
      to_route(); return;
    }
    if (dir_off_early + total > P.out_cap) { if (lane == 0) atomicAdd(&P.dir_flags[1], 1u); to_route(); return; }
    fam_out = P.out + dir_off_early;
  }
  PH(5)
  S2_ABLATE_AFTER(5, lc_a + lc_b + surv_a + surv_b + rej + (uint32_t)mem_a + (uint32_t)mem_b + ov_bases + ov_corr)
  // ---- 6. consensus columns -------------------------------------------------------------------------------------------------------
  const DeviceTables* T = P.T;
  const uint64_t col_base = uniform_u64(col_base_early);
  // the family's part of the four scratch planes (the packed build works them out where it writes them — planes(), from the kernarg segment, see
  // S2Args —: ten scalar registers that were live from here to the end)
  uint8_t* const fam_code = COLS == 1 ? nullptr : P.col_code + col_base;
  uint8_t* const fam_qual = COLS == 1 ? nullptr : P.col_qual + col_base;
  uint16_t* const fam_depth = COLS == 1 ? nullptr : P.col_depth + col_base;
  uint16_t* const fam_err = COLS == 1 ? nullptr : P.col_err + col_base;
  struct Planes { uint8_t* code; uint8_t* qual; uint16_t* depth; uint16_t* err; };
  auto planes = [&]() -> Planes {
    if constexpr (COLS != 1) return Planes{fam_code, fam_qual, fam_depth, fam_err};
    else { const auto& K = KA::of(P); return Planes{K.col_code + col_base, K.col_qual + col_base, K.col_depth + col_base, K.col_err + col_base}; }
  };
  const uint8_t* pairs = nullptr;
  if constexpr (!TINY) {
#if FGX_S2_F32
    pairs = (const uint8_t*)&sL.pairf[0][0];
#else
    pairs = (const uint8_t*)&sL.pair[0][0];
#endif
  }
  // a single-read end: LUT keyed by the unclamped quality (:1677-1708)
  auto single_end = [&](unsigned long long members, uint32_t Lc, uint32_t coff) {
    const Planes PL = planes();
    const uint32_t r = (uint32_t)__builtin_ctzll(members);
    const uint32_t s_r = rlane(my_s, r), q_r = rlane(my_q, r), L_r = rlane(l_seq, r);
    const bool rv_r = (rlane(bits, r) & 4u) != 0;
    for (uint32_t p = lane; p < Lc; p += 64) {
      const uint32_t idx = rv_r ? L_r - 1 - p : p;
      uint32_t code = ((uint32_t)W[s_r + (idx >> 1)] >> ((~idx & 1u) << 2)) & 15u, q = W[q_r + idx];
      if (rv_r) code = comp_code((uint8_t)code);
      if (q < min_bq) { code = 15; q = FGX_MIN_PHRED; }
      const uint8_t adj = q < 94 ? T->single_input_quals[q] : 0;
      uint8_t ob, oq;
      if (adj < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; } else { ob = (uint8_t)code; oq = adj; }
      if constexpr (DIRECT != 0) { (void)coff; }
      else {
        const uint32_t oc = coff + p;
        PL.code[oc] = ob; PL.qual[oc] = oq; PL.depth[oc] = (uint16_t)(code != 15 ? 1 : 0); PL.err[oc] = 0;
      }
    }
  };
  // the same for a record written in place: a pass = 64 columns, two columns to a sequence byte (even lane = high nibble)
  auto single_end_direct = [&](unsigned long long members, const S2DirRec& R, bool is_b) {
    const uint32_t r = (uint32_t)__builtin_ctzll(members);
    const uint32_t s_r = rlane(my_s, r), q_r = rlane(my_q, r), L_r = rlane(l_seq, r);
    const bool rv_r = (rlane(bits, r) & 4u) != 0;
    const uint32_t Lc = R.Lc;
    uint8_t* const q = fam_out + R.base;
    for (uint32_t p0 = 0; p0 < Lc; p0 += 64) {
      const uint32_t p = p0 + lane;
      const bool in = p < Lc;
      const uint32_t idx = in ? (rv_r ? L_r - 1 - p : p) : 0u;
      uint32_t code = ((uint32_t)W[s_r + (idx >> 1)] >> ((~idx & 1u) << 2)) & 15u, qv = W[q_r + idx];
      if (rv_r) code = comp_code((uint8_t)code);
      if (qv < min_bq) { code = 15; qv = FGX_MIN_PHRED; }
      const uint32_t adj = qv < 94 ? T->single_input_quals[qv] : 0u;
      uint32_t ob, oq;
      if (adj < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; } else { ob = code; oq = adj; }
      if (!in) ob = 0;
      const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ob, 0xB1, 0xF, 0xF, false);   // the neighbouring lane's code (quad_perm 1, 0, 3, 2)
      const uint32_t dcol = (in && code != 15u) ? 1u : 0u;
      if (in) {
        if (!(lane & 1u)) q[R.o_seq + (p >> 1)] = (uint8_t)((ob << 4) | nb);
        q[R.o_qual + p] = (uint8_t)oq;
        if (P.per_base_tags) { s2_st16(q + R.o_cd + 2u * p, dcol); s2_st16(q + R.o_ce + 2u * p, 0u); }
        const uint32_t sh = is_b ? 16u : 0u;
        acc_max = s2_pkmax(acc_max, dcol << sh); acc_min = s2_pkmin(acc_min, (dcol << sh) | (is_b ? 0x0000FFFFu : 0xFFFF0000u)); acc_sum += dcol << sh;
      }
    }
  };
  // Multi-read ends: ONE flat column space — cnt_a columns of end A, then cnt_b of end B — 64 columns per pass; a lane's two
  // tile addresses (quality byte, sequence byte of row 0 of its end) are its own, member j is `address + j * stride`.  Both
  // ends share a run when they have equally many rows (the usual pair family: 2 x 150 columns = 5 passes).
  bool gone = false, gone_far = false;                        // the family leaves: no room for its items in this launch's slice / not this kernel's at all
  bool multi_items = false;                                   // some column took more than one item (more than 16 observations): the family's items stay in ONE list
  auto run_cols = [&](const uint32_t cnt_a, const uint32_t cnt_b, const uint32_t m) {
    if constexpr (COLS != 1) {     // (the packed build holds no gate tables: nothing of this body exists there)
    // DIRECT: end B starts at an EVEN flat column, so that the two columns of a sequence byte always sit in neighbouring lanes of one pass
    const uint32_t cb0 = DIRECT ? (cnt_a + 1u) & ~1u : cnt_a;   // first flat column of end B
    const uint32_t tot = cb0 + cnt_b;
    // index of column c in a member read of its end: forward c' , reverse L - 1 - c' (c' = c, or c - cb0 in end B) = (c ^ xm) + xk
    const uint32_t xm_a = rev_a ? ~0u : 0u, xk_a = rev_a ? len_a : 0u;
    const uint32_t xm_b = rev_b ? ~0u : 0u, xk_b = rev_b ? len_b + cb0 : 0u - cb0;
    const uint32_t qb_b = m_a * QS, sb_a = S0, sb_b = S0 + m_a * SS;
    const uint32_t oc_base = cnt_a ? 0u : lc_a;               // scratch column of flat column 0: end A's columns come first
    // DIRECT: a lane's four store offsets are `field start of its end + its column`: end B's starts with the flat offset folded in
    const uint32_t fA_seq = RA.base + RA.o_seq, fA_qual = RA.base + RA.o_qual, fA_cd = RA.base + RA.o_cd, fA_ce = RA.base + RA.o_ce;
    const uint32_t fB_seq = RB.base + RB.o_seq - (cb0 >> 1), fB_qual = RB.base + RB.o_qual - cb0, fB_cd = RB.base + RB.o_cd - 2u * cb0, fB_ce = RB.base + RB.o_ce - 2u * cb0;
    const uint32_t dq_seq = fB_seq - fA_seq, dq_qual = fB_qual - fA_qual, dq_cd = fB_cd - fA_cd, dq_ce = fB_ce - fA_ce;   // end B's fields from end A's
#if FGX_S2_F32 && FGX_S2_PREGATE
    const S2PreGate pre = s2_pregate_consts(sT, m);
#endif
    const uint32_t nsafe = P.s2_nsafe;
    const bool fast_m = FGX_S2_F32 && FGX_S2_PREGATE && FGX_S2_NOSUM && m >= nsafe;   // (FGX_NEVER_CAP: no end is that deep)
    for (uint32_t c0 = 0; c0 < tot && !gone; c0 += 64) {
      const uint32_t c = uni(c0) + lane;
      const bool in_b = c >= cb0, incol = in_b ? c < tot : c < cnt_a;
      const uint32_t xm = in_b ? xm_b : xm_a, xk = in_b ? xk_b : xk_a;
      const bool lane_rev = xm != 0;
      const uint32_t ix = incol ? (c ^ xm) + xk : 0u;                      // (column < consensus length <= read length)
      const uint32_t ish = (~ix & 1u) << 2;
      const uint32_t qa = (in_b ? qb_b : 0u) + ix, sa = (in_b ? sb_b : sb_a) + (ix >> 1);
      const uint32_t oc = oc_base + c;
      if constexpr (DIRECT == 0) if (fast_m) {
        // ---- round 5: the sum-free pass.  An end of at least nsafe rows (unanimous_cap_depth, gate_core.h): a column whose accepted
        //      observations show ONE base, nsafe times or more, is (base, cap) whatever their qualities — the OR of the codes, their sum
        //      and their number decide, no table and no sum.  A pass in which some lane's single-base column holds FEWER observations than
        //      that (ragged read ends) falls through to the pass with the f32 sums below; a column with a second base / an N / IUPAC code /
        //      a '=' of good quality travels to k_call_full with its observations, written by one lane per row.
        uint32_t f_or = 0, f_sum = 0, f_cnt = 0;
        {
          uint32_t qj = qa, sj = sa, j = 0;
          for (; j + 4 <= m; j += 4, qj += 4 * QS, sj += 4 * SS) {
            const uint32_t q0 = W[qj], b0 = W[sj], q1 = W[qj + QS], b1_ = W[sj + SS], q2 = W[qj + 2 * QS], b2_ = W[sj + 2 * SS], q3 = W[qj + 3 * QS], b3_ = W[sj + 3 * SS];
            S2_OBSERVE_FAST(q0, b0); S2_OBSERVE_FAST(q1, b1_); S2_OBSERVE_FAST(q2, b2_); S2_OBSERVE_FAST(q3, b3_);
          }
          for (; j < m; j++, qj += QS, sj += SS) { const uint32_t q0 = W[qj], b0 = W[sj]; S2_OBSERVE_FAST(q0, b0); }
        }
        const bool one = incol && ((0x116u >> f_or) & 1u) != 0 && f_sum == s2_mul24(f_cnt, f_or);   // one base, ACGT, every accepted code is it
        const bool capnow = one && f_cnt >= nsafe;
        if (!__any(one && !capnow)) {
          const bool coldf = incol && !capnow && f_cnt != 0u;
          const unsigned long long cm_ = __ballot(coldf);
          if (cm_) {
            // the columns for k_call_full: ceil(m / 16) consecutive items each; observation j (row j of the end) is written by lane j
            const uint32_t per_cold = (m + 15u) >> 4, ncold = (uint32_t)__popcll(cm_);
            const uint32_t cnt = per_cold * ncold;
            if (icnt + cnt > icap) { gone = true; break; }
            if (per_cold > 1u) multi_items = true;
            uint32_t k = 0;
            for (unsigned long long w = cm_; w; w &= w - 1, k++) {
              const uint32_t l = (uint32_t)__builtin_ctzll(w);
              const uint32_t qa_l = rlane(qa, l), sa_l = rlane(sa, l), ish_l = rlane(ish, l), oc_l = rlane(oc, l), rv_l = rlane(lane_rev ? 1u : 0u, l);
              uint8_t* const it = W + ibase + s2_mul24(icnt + per_cold * k, (uint32_t)sizeof(FullItem));
              if (lane < m) {
                uint32_t cc = __builtin_amdgcn_ubfe((uint32_t)W[sa_l + s2_mul24(lane, SS)], ish_l, 4u);
                if (rv_l) cc = __builtin_bitreverse32(cc) >> 28;
                const uint32_t qv = W[qa_l + s2_mul24(lane, QS)];
                *(uint16_t*)(it + (lane >> 4) * (uint32_t)sizeof(FullItem) + 8 + 2 * (lane & 15u)) = (uint16_t)((cc << 8) | qv);
              }
              if (lane < per_cold) {
                uint8_t* const hd = it + lane * (uint32_t)sizeof(FullItem);
                if (lane == 0) *(uint64_t*)hd = col_base + oc_l;
                *(uint32_t*)(hd + 40) = 0; *(uint32_t*)(hd + 44) = lane == 0 ? (FULL_ITEM_OBS | m) : FULL_ITEM_CONT;
              }
            }
            icnt = uni(icnt + cnt);
          }
          if (incol && !coldf) {
            const uint32_t n1f = capnow ? f_cnt : 0u;
            uint32_t cb = f_or;
            if (lane_rev) cb = __builtin_bitreverse32(cb) >> 28;
            uint32_t ob, oq;
            if (n1f < P.min_reads) { ob = 15; oq = 0; }
            else if (n1f == 0u || sT.cap < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; }
            else { ob = cb; oq = sT.cap; }
            fam_depth[oc] = (uint16_t)n1f;
            fam_code[oc] = (uint8_t)ob; fam_qual[oc] = (uint8_t)oq; fam_err[oc] = 0;
          }
          continue;
        }
      }
#if FGX_S2_F32
      s2_f32x2 acc2 = {0.0f, 0.0f};                           // {w~, l~}: sums of the one base seen / of "any other base" (unanimous_call_approx)
      float cntf = 0.0f;                                      // (FGX_S2_FMASEL: the number of observations added, as a sum of 1.0s)
#else
      double s1 = 0.0, c1 = 0.0, sR = 0.0, cR = 0.0;
#endif
      uint32_t allow = incol ? 0x116u : 0u, n1 = 0;
      unsigned long long suspect = 0;
      {
        uint32_t qj = qa, sj = sa, j = 0;
        for (; j + 4 <= m; j += 4, qj += 4 * QS, sj += 4 * SS) {
          const uint32_t q0 = W[qj], b0 = W[sj], q1 = W[qj + QS], q2 = W[qj + 2 * QS], q3 = W[qj + 3 * QS];
          uint32_t b1 = W[sj + SS], b2 = W[sj + 2 * SS], b3 = W[sj + 3 * SS];
          S2_PAIR(p0, q0); S2_PAIR(p1, q1); S2_PAIR(p2, q2); S2_PAIR(p3, q3);
          S2_PIN4(p0, p1, p2, p3);
          FGX_PIN("+v"(b1), "+v"(b2), "+v"(b3));   // (zero-extended where they were loaded: sunk into the blocks below, the extension is redone there)
          S2_OBSERVE(q0, b0, p0); S2_OBSERVE(q1, b1, p1); S2_OBSERVE(q2, b2, p2); S2_OBSERVE(q3, b3, p3);
        }
        for (; j < m; j++, qj += QS, sj += SS) { const uint32_t q0 = W[qj], b0 = W[sj]; S2_PAIR(p0, q0); S2_PIN1(p0); S2_OBSERVE(q0, b0, p0); }
      }
#if FGX_S2_F32 && FGX_S2_FMASEL
      n1 = (uint32_t)cntf;
#elif FGX_S2_F32
      (void)cntf;
#endif
      uint32_t b1 = (uint32_t)__builtin_ctz(allow | 0x80000000u);          // the one base seen = index of the set bit (nothing seen: a value nobody reads)
      if (lane_rev) b1 = __builtin_bitreverse32(b1) >> 28;                 // complement = bit reversal of the code
      uint32_t cold = (incol && ((suspect >> lane) & 1ull)) ? 1u : 0u;
      // ---- call ----
      bool need_full = false, resolved = true;
      uint32_t q_call = FGX_MIN_PHRED, code_call = 15;
      if (incol && !cold) {
        if (n1 != 0) {
          uint32_t qq = 0;
          CallConst KC;
          KC.cap = sT.cap; KC.cap_threshold = sT.cap_threshold; KC.half_cerr_at_cap = sT.half_cerr_at_cap;
#if FGX_S2_F32 && FGX_S2_PREGATE
          if (s2_cap_pregate(pre, acc2.x, acc2.y)) { resolved = true; qq = KC.cap; }
          else resolved = unanimous_call_approx(sT, KC, acc2.x, acc2.y, n1, &qq);
#elif FGX_S2_F32
          resolved = unanimous_call_approx(sT, KC, acc2.x, acc2.y, n1, &qq);
#else
          resolved = unanimous_call_lds(sT, P.T->t.cerr_min, KC, s1, sR, &qq);
#endif
          if (resolved) { q_call = qq; code_call = b1; }
        }                                                    // else: no observation → ('N', 2), depth 0
        need_full = !resolved;
        if constexpr (DIRECT == 0) fam_depth[oc] = (uint16_t)n1;   // (at most 64 member reads: no saturation to apply)
      }
#if FGX_S2_F32
      // the approximate sums are no input for k_call_full: a column the gate cannot decide travels with its observations, like one that
      // showed a second base (k_call_full sums them as the reference does)
      if (need_full) { cold = 1u; need_full = false; }
#endif
      // columns for k_call_full: the chains of a single-base column the gate could not decide, the observations of a column
      // that showed a second base
      uint32_t dcold = 0;
      const unsigned long long im_ = __ballot(need_full || cold);
      if (im_) {
        // a cold column takes ceil(m / 16) consecutive items (m is the same for the whole run), every other one item
        const unsigned long long cm_ = __ballot(cold != 0);
        const uint32_t per_cold = (m + 15u) >> 4;
        const uint32_t cnt = (uint32_t)__popcll(im_) + (per_cold - 1u) * (uint32_t)__popcll(cm_);
        if (icnt + cnt > icap) { gone = true; break; }
        if (per_cold > 1u && cm_) multi_items = true;
        if (need_full || cold) {
          uint8_t* const it = W + ibase + s2_mul24(icnt + (uint32_t)__popcll(im_ & below) + (per_cold - 1u) * (uint32_t)__popcll(cm_ & below), (uint32_t)sizeof(FullItem));
          if constexpr (DIRECT != 0) *(uint64_t*)it = FULL_DEST_DIRECT | ((uint64_t)(slot0 + (in_b ? 2u : type_a)) << 16) | (uint64_t)(c - (in_b ? cb0 : 0u));
          else *(uint64_t*)it = col_base + oc;
          if (cold) {
            uint32_t qj = qa, sj = sa;
            for (uint32_t j = 0; j < m; j++, qj += QS, sj += SS) {
              uint32_t cc = __builtin_amdgcn_ubfe((uint32_t)W[sj], ish, 4u);
              if (lane_rev) cc = __builtin_bitreverse32(cc) >> 28;
              const uint32_t qv = W[qj];
              *(uint16_t*)(it + (j >> 4) * (uint32_t)sizeof(FullItem) + 8 + 2 * (j & 15u)) = (uint16_t)((cc << 8) | qv);   // observation j: item j / 16 of the column
              if constexpr (DIRECT != 0) dcold += (qv >= min_bq && ((0x116u >> cc) & 1u)) ? 1u : 0u;   // the depth k_call_full will count (ACGT of good quality)
            }
            *(uint32_t*)(it + 40) = 0; *(uint32_t*)(it + 44) = FULL_ITEM_OBS | m;
            for (uint32_t k = 1; k < per_cold; k++) { *(uint32_t*)(it + k * (uint32_t)sizeof(FullItem) + 40) = 0; *(uint32_t*)(it + k * (uint32_t)sizeof(FullItem) + 44) = FULL_ITEM_CONT; }
          } else {
#if !FGX_S2_F32
            *(double*)(it + 8) = s1; *(double*)(it + 16) = 0.0; *(double*)(it + 24) = 0.0; *(double*)(it + 32) = sR;
            *(uint32_t*)(it + 40) = n1; *(uint32_t*)(it + 44) = b1;
#endif
          }
        }
        icnt = uni(icnt + cnt);
      }
      if constexpr (DIRECT != 0) {
        // the lane's column goes straight into its record: sequence nibble (the even lane stores the byte of both), quality, cd, ce.  A
        // column that waits for k_call_full leaves its nibble 0 (OR-ed in there) and its quality / ce (and, cold, cd) entries unwritten
        const bool have = incol && !cold && resolved;
        uint32_t ob = 0, oq = 0;
        if (have) {
          if (n1 < P.min_reads) { ob = 15; oq = 0; }
          else if (q_call < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; }
          else { ob = code_call; oq = q_call; }
        }
        const uint32_t nb = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ob, 0xB1, 0xF, 0xF, false);   // the neighbouring lane's code (quad_perm 1, 0, 3, 2)
        if (incol) {
          // (one predicate for the three per-column stores: a column that waits for k_call_full gets placeholders — quality 0, ce 0 — which
          // that kernel overwrites after every column kernel has finished; its cd entry is final either way)
          const uint32_t dcol = cold ? dcold : n1, bsel = in_b ? ~0u : 0u;
          fam_out[fA_qual + (bsel & dq_qual) + c] = (uint8_t)oq;
          if (P.per_base_tags) {
            *(uint16_t*)(fam_out + (fA_cd + (bsel & dq_cd) + 2u * c)) = (uint16_t)dcol;
            *(uint16_t*)(fam_out + (fA_ce + (bsel & dq_ce) + 2u * c)) = (uint16_t)0;
          }
          if (!(lane & 1u)) fam_out[fA_seq + (bsel & dq_seq) + (c >> 1)] = (uint8_t)((ob << 4) | nb);
          const uint32_t sh = bsel & 16u, dv = dcol << sh;
          acc_max = s2_pkmax(acc_max, dv); acc_min = s2_pkmin(acc_min, dv | (0xFFFF0000u >> sh)); acc_sum += dv;
        }
      } else if (incol && !cold && resolved) {
        uint8_t ob, oq;
        if (n1 < P.min_reads) { ob = 15; oq = 0; }
        else if (q_call < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; }
        else { ob = (uint8_t)code_call; oq = (uint8_t)q_call; }
        fam_code[oc] = ob; fam_qual[oc] = oq; fam_err[oc] = 0;
      }
    }
    }
  };
  // ---- round 5: the PACKED pass — a lane takes EIGHT neighbouring tile positions of its end (one 32-bit word of a sequence row, one 64-bit
  //      word of a quality row), so the 2 x 150 columns of the usual family are ONE pass of 38 lanes instead of five passes of 64 columns:
  //      the per-pass work (addresses, gates, ballots, four scratch stores per lane) is paid once, the stores are 8 / 16 bytes wide, and the
  //      arithmetic is on packed integers.  It answers what the sum-free pass of run_cols answers — an end of at least nsafe rows
  //      (unanimous_cap_depth, gate_core.h): a column whose accepted observations show ONE base nsafe times or more is (base, cap) —:
  //      per row, the codes of observations below --min-input-base-quality are cleared (a bytewise compare of the eight qualities; the
  //      clearing itself runs only for lanes that hold such a quality), then  OR |= codes  and two words of byte counters (even / odd
  //      positions) count the codes that are not 0.  One base <=> the OR of a column is one of 1, 2, 4, 8, and the counter is then the number
  //      of its observations.  A code 0 ('=') of good quality is no observation for the reference (k_call_full skips it the same way) and
  //      adds nothing here; any other non-ACGT code makes the OR a non-base.  Every column the pass does not answer — a second base, a
  //      non-ACGT code, or ONE base seen fewer than nsafe times (the f32 / f64 gates' business in run_cols) — travels to k_call_full with
  //      its observations; these columns of all lanes are compacted into a list and a LANE PER COLUMN writes its item (run_cols: the
  //      wavefront walks them one by one).  Reverse ends: bit reversal of the OR word complements the codes AND puts them in column order;
  //      the counters are byte-swapped.  Everything is decided before the first byte is written: without room for the items the family
  //      takes the next launch (larger slices) untouched.
  uint32_t ires_early = 0;            // the family's reservation in its k_call_full list, asked for as soon as the item count is known (packed pass, last run)
  bool ires_asked = false;
  auto run_cols_packed = [&](const uint32_t cnt_a, const uint32_t cnt_b, const uint32_t m, const bool last_run) -> bool {
    const uint32_t nsafe = P.s2_nsafe;
    const uint32_t ga = cnt_a ? (len_a + 7u) >> 3 : 0u, gb = cnt_b ? (len_b + 7u) >> 3 : 0u;      // lanes of end A, of end B
    const bool dbg = (P.s2_packed & 2u) != 0;
    if (!(P.s2_packed && m >= nsafe && m <= S2_PACKED_MAX_ROWS && P.min_reads <= nsafe && min_bq <= 128u && ((QS & 7u) | (SS & 3u)) == 0u && ga + gb <= 64u &&
          S0 + n * SS < 65536u && lc_a + lc_b < 65536u)) {       // (wave-uniform operands: the scalar multiply — s2_mul24's result is a vector register, and a branch on it a divergent one)
      if (dbg && lane == 0) atomicAdd(&g_s2_dbg[42], 1u);
      return false;
    }
    if (dbg && lane == 0) atomicAdd(&g_s2_dbg[0], 1u);
    const bool in_b = lane >= ga, inl = lane < ga + gb;
    const uint32_t k = inl ? (in_b ? lane - ga : lane) : 0u;
    const bool lrev = (in_b ? rev_b : rev_a) != 0;
    const uint32_t lenE = in_b ? len_b : len_a, cntE = in_b ? cnt_b : cnt_a;
    const uint32_t rowE = in_b ? m_a : 0u;                      // first row of the lane's end
    const uint32_t qaddr0 = s2_mul24(rowE, QS) + 8u * k, saddr0 = S0 + s2_mul24(rowE, SS) + 4u * k;
    // (the arithmetic is packed_core.h's: the same functions run on the host in tests/test_packed_core.py)
    const uint32_t mb4 = min_bq * 0x01010101u;
    pk::Acc A;
    pk::acc_reset(A);
    if (!__any(dirty_v != 0u)) {
      // CLEAN family (phase 1b): code 0 under every sub-floor quality already — the codes alone
      uint32_t sj = saddr0, j = 0;
      for (; j + 4 <= m; j += 4, sj += 4 * SS) {
        const uint32_t b0 = *(const uint32_t*)(W + sj), b1_ = *(const uint32_t*)(W + sj + SS), b2_ = *(const uint32_t*)(W + sj + 2 * SS), b3_ = *(const uint32_t*)(W + sj + 3 * SS);
        pk::acc_row_seq(A, b0); pk::acc_row_seq(A, b1_); pk::acc_row_seq(A, b2_); pk::acc_row_seq(A, b3_);
      }
      for (; j < m; j++, sj += SS) pk::acc_row_seq(A, *(const uint32_t*)(W + sj));
    } else {
      uint32_t qj = qaddr0, sj = saddr0, j = 0;
      for (; j + 4 <= m; j += 4, qj += 4 * QS, sj += 4 * SS) {
        const uint2 q0 = *(const uint2*)(W + qj), q1 = *(const uint2*)(W + qj + QS), q2 = *(const uint2*)(W + qj + 2 * QS), q3 = *(const uint2*)(W + qj + 3 * QS);
        const uint32_t b0 = *(const uint32_t*)(W + sj), b1_ = *(const uint32_t*)(W + sj + SS), b2_ = *(const uint32_t*)(W + sj + 2 * SS), b3_ = *(const uint32_t*)(W + sj + 3 * SS);
        pk::acc_row(A, q0.x, q0.y, b0, mb4); pk::acc_row(A, q1.x, q1.y, b1_, mb4);
        pk::acc_row(A, q2.x, q2.y, b2_, mb4); pk::acc_row(A, q3.x, q3.y, b3_, mb4);
      }
      for (; j < m; j++, qj += QS, sj += SS) { const uint2 q0 = *(const uint2*)(W + qj); const uint32_t b0 = *(const uint32_t*)(W + sj); pk::acc_row(A, q0.x, q0.y, b0, mb4); }
    }
    PH(9)
    // column order: slot s of the lane is column c_lo + s of its end (forward: position s of the group; reverse: position 7 - s, complemented)
    pk::Out F;
    pk::finalize(A, inl, lrev, lenE, cntE, k, nsafe, sT.cap, P.min_cons_bq, P.min_reads, F);
    const int32_t c_lo = F.c_lo, lo_s = F.lo_s, hi_s = F.hi_s;
    const uint32_t* const code2 = F.code2; const uint32_t* const qual2 = F.qual2; const uint32_t* const dep4 = F.dep4;
    const uint32_t* const flag2 = F.flag2; const uint32_t* const full2 = F.valid2;
    PH(10)
    // ---- the columns for k_call_full: flagged slots of all lanes -> a list of descriptors at the top of the wave's slice, then a lane per column
    uint32_t fm = (flag2[0] >> 7) | (flag2[1] >> 3);             // bit 8 j: slot j, bit 8 j + 4: slot 4 + j
    const uint32_t fc = (uint32_t)__builtin_popcount(fm);
    const unsigned long long pb0 = __ballot((fc & 1u) != 0), pb1 = __ballot((fc & 2u) != 0), pb2 = __ballot((fc & 4u) != 0), pb3 = __ballot((fc & 8u) != 0);
    const uint32_t T = uni((uint32_t)__popcll(pb0) + 2u * (uint32_t)__popcll(pb1) + 4u * (uint32_t)__popcll(pb2) + 8u * (uint32_t)__popcll(pb3));
    const uint32_t oc0 = (in_b ? offB : offA) + (uint32_t)c_lo;    // scratch column of slot 0 (c_lo may be below zero by up to seven: the padding in front of the end)
    const uint32_t list = (P.lds_wave_bytes - 8u * T) & ~7u;
    // (room: the descriptors of the flagged columns at the top of the slice; the items — of the columns that turn out to need one, below — grow
    // from ibase towards them and are checked as they are made)
    if (T && (8u * T + 8u > P.lds_wave_bytes || ibase + icnt * (uint32_t)sizeof(FullItem) > list)) {
      if (dbg && lane == 0) atomicAdd(&g_s2_dbg[3], 1u);
      gone = true; return true;
    }
    (void)last_run;
    // ---- the lane's columns: 8 + 8 + 16 + 16 bytes — all eight slots of its group, also when only the slots [lo_s, hi_s) are columns of its end:
    //      the others land in the padding around the end (offA / offB above).  (A column that is not answered here gets a placeholder: the lane
    //      that takes it below — later in the wavefront's program order: stores of ONE wavefront to one address reach memory in program order on
    //      gfx9, the vector memory pipeline is in-order per wavefront — or k_call_full, after every column kernel has finished, writes all four
    //      entries.)  32-bit offsets from the family's first scratch column: scalar base + lane offset addressing.
    (void)full2; (void)lo_s;
    if (hi_s > lo_s) {
      const Planes PL = planes();
      const uint2 cv = make_uint2(code2[0], code2[1]), qv = make_uint2(qual2[0], qual2[1]);
      const u32x4 dv = {dep4[0], dep4[1], dep4[2], dep4[3]}, zv = {0u, 0u, 0u, 0u};
      const uint32_t o1 = oc0, o2 = 2u * oc0;
      __builtin_memcpy(PL.code + o1, &cv, 8); __builtin_memcpy(PL.qual + o1, &qv, 8);
      __builtin_memcpy((uint8_t*)PL.depth + o2, &dv, 16); __builtin_memcpy((uint8_t*)PL.err + o2, &zv, 16);
    }
    PH(12)
    if (T) {
      uint32_t pre = mbcnt64(pb0) + 2u * mbcnt64(pb1) + 4u * mbcnt64(pb2) + 8u * mbcnt64(pb3);           // flagged slots in the lanes below
      while (fm) {
        const uint32_t bi = (uint32_t)__builtin_ctz(fm), slot = (bi >> 3) | (bi & 4u);
        fm &= fm - 1u;
        const uint32_t pos = lrev ? 7u - slot : slot;                                                       // position of the column in its group
        const uint2 d = make_uint2((qaddr0 + pos) | ((saddr0 + (pos >> 1)) << 16), (oc0 + slot) | (((~pos & 1u) << 2) << 16) | ((lrev ? 1u : 0u) << 20));
        *(uint2*)(W + list + 8u * pre) = d;
        pre++;
      }
      PH(11)
      wave_sync();
      // a lane per (column, row): 8 columns x 8 rows a step for ends of up to 8 rows, 4 x 16 beyond (m <= 16 here: one item per column).
      // Every lane reads ITS observation; the observations the column loop counted (a code that is not 0 at or above the quality floor) are
      // balloted.  A column that holds ONE such observation, or TWO of one base, is answered right here by the lane of its first observation:
      // the call is a function of the qualities (S2Lds::t1 / t2, packed_core.h) — 59 % + 20 % of the columns `simulate` data flags are such
      // columns (the read-through zone of a pair whose mates disagree: a random subset of the rows survives the overlap correction).  Every
      // OTHER column gets a k_call_full item: its slot = the number of such columns before it (round 6; round 5 wrote an item for every
      // flagged column and turned those of the answered ones into continuation items afterwards: 7.3 items per family went to k_call_full
      // where 3.3 were needed).
      const auto& K6 = KA::of(P);                                                                           // (one read of the segment for the planes and the table)
      const Planes PL = {K6.col_code + col_base, K6.col_qual + col_base, K6.col_depth + col_base, K6.col_err + col_base};
      const uint8_t* const t2g = ((const S2Image*)K6.s2_image)->t2;
      const uint32_t rp_sh = m <= 8u ? 3u : m <= 16u ? 4u : 5u, rows_per = 1u << rp_sh, cps = 64u >> rp_sh;   // (8 x 8, 4 x 16 or — ends of 17 .. 31 rows: two items per column — 2 x 32)
      const uint32_t per_cold = (m + 15u) >> 4;
      const uint32_t ce = lane >> rp_sh, j = lane & (rows_per - 1u), lane0 = lane & ~(rows_per - 1u);
      const unsigned long long below0 = (1ull << lane0) - 1ull;                                              // the lanes of the columns before this lane's
      for (uint32_t e0 = 0; e0 < T; e0 += cps) {
        const uint32_t e = e0 + ce;
        const bool col_on = e < T, on = col_on && j < m;
        const uint2 d = *(const uint2*)(W + list + 8u * (col_on ? e : 0u));
        const uint32_t qa_l = d.x & 0xFFFFu, sa_l = d.x >> 16, oc_l = d.y & 0xFFFFu, ish_l = (d.y >> 16) & 15u;
        const bool rv_l = ((d.y >> 20) & 1u) != 0;
        const uint32_t jj = on ? j : 0u;
        uint32_t cc = __builtin_amdgcn_ubfe((uint32_t)W[sa_l + s2_mul24(jj, SS)], ish_l, 4u);
        if (rv_l) cc = __builtin_bitreverse32(cc) >> 28;
        const uint32_t qv = W[qa_l + s2_mul24(jj, QS)];
        const uint32_t ob16 = (cc << 8) | qv;
        const bool acc1 = on && qv >= min_bq && cc != 0u;
        const unsigned long long bal = __ballot(acc1);
        const uint32_t seg = (uint32_t)(bal >> lane0) & (rows_per >= 32u ? 0xFFFFFFFFu : ((1u << rows_per) - 1u));   // the column's rows that hold a counted observation
        const uint32_t seg2 = seg & (seg - 1u);
        const uint32_t r1 = seg ? (uint32_t)__builtin_ctz(seg) : 0u, r2 = seg2 ? (uint32_t)__builtin_ctz(seg2) : r1;
        const uint32_t o1 = (uint32_t)__shfl((int)ob16, (int)(lane0 + r1)), o2 = (uint32_t)__shfl((int)ob16, (int)(lane0 + r2));
        const uint32_t c1 = o1 >> 8, q1 = o1 & 0xFFu, c2 = o2 >> 8, q2 = o2 & 0xFFu;
        const uint32_t q1c = q1 < 93u ? q1 : 93u, q2c = q2 < 93u ? q2 : 93u;
        const bool base1 = ((0x116u >> c1) & 1u) != 0u;
        const bool one = seg != 0u && seg2 == 0u, two = seg2 != 0u && (seg2 & (seg2 - 1u)) == 0u;
        uint32_t tq = 0xFFu;
        if (col_on && base1) {
          if (one) tq = sL.t1[q1c];
          else if (two && c2 == c1) tq = t2g[s2_mul24(q1c, pk::T2_DIM) + q2c];
        }
        const bool need = col_on && tq == 0xFFu;                                                             // (the same in every lane of the column)
        const unsigned long long needm = __ballot(need && j == 0u);
        const uint32_t n_need = per_cold * (uint32_t)__popcll(needm);                                       // items: ceil(m / 16) consecutive ones per column
        if (per_cold > 1u && needm) multi_items = true;
        if (ibase + (icnt + n_need) * (uint32_t)sizeof(FullItem) > list) {                                    // no room for this step's items: the next launch (larger slices)
          if (dbg && lane == 0) atomicAdd(&g_s2_dbg[3], 1u);
          gone = true; return true;
        }
        if (need) {
          uint8_t* const it = W + ibase + s2_mul24(icnt + per_cold * (uint32_t)__popcll(needm & below0), (uint32_t)sizeof(FullItem));
          if (on) *(uint16_t*)(it + (j >> 4) * (uint32_t)sizeof(FullItem) + 8 + 2 * (j & 15u)) = (uint16_t)ob16;   // observation j of the column: item j / 16
          // (the `obs` word of these items is free: the family's index + 1, through which k_call_full finds out whether the pair writer applies the answer — fastpath.h, FullResult)
          if (j == 0u) { *(uint64_t*)it = col_base + oc_l; *(uint32_t*)(it + 40) = g + 1u; *(uint32_t*)(it + 44) = FULL_ITEM_OBS | m; }
          if (j == 16u && per_cold > 1u) { *(uint32_t*)(it + sizeof(FullItem) + 40) = g + 1u; *(uint32_t*)(it + sizeof(FullItem) + 44) = FULL_ITEM_CONT; }
        } else if (col_on && j == r1) {
          const uint32_t nobs = one ? 1u : 2u;
          uint32_t ob, oq;
          if (nobs < P.min_reads) { ob = 15; oq = 0; }
          else if (tq < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; }
          else { ob = c1; oq = tq; }
          PL.code[oc_l] = (uint8_t)ob; PL.qual[oc_l] = (uint8_t)oq;
          *(uint16_t*)((uint8_t*)PL.depth + 2u * oc_l) = (uint16_t)nobs; *(uint16_t*)((uint8_t*)PL.err + 2u * oc_l) = (uint16_t)0;
        }
        icnt = uni(icnt + n_need);
      }
    }
    PH(13)
    if (dbg && lane == 0) { atomicAdd(&g_s2_dbg[1], 1u); atomicAdd(&g_s2_dbg[2], T); }
    return true;
  };
  // (packed build) the family's result for k_split_finish — phase 7 — goes out HERE, before the column pass: everything in it is known, and the
  // thirteen uniforms it is made of otherwise wait in spill lanes across the pass.  A family that leaves after all (no room in the slice, a full
  // list) overwrites it through the same lane: stores of one wavefront to one address reach memory in program order.
  if constexpr (COLS == 1) {
    leave(__any(dirty_v != 0u) ? 0x81u : 0xC1u, (ne << 8) | (type_a << 16) | (fk_a << 24), fk_b | (surv_a << 8) | (surv_b << 16) | (n << 24), lc_a | (lc_b << 16), rej, ov_agree, ov_dis);
    if (lane == 0) ((uint32_t*)&KA::of(P).split_out[g])[6] = ov_corr;
  }
  {
    const bool multi_a = ne >= 1u && surv_a >= 2u, multi_b = ne == 2u && surv_b >= 2u;
    if constexpr (DIRECT != 0) {
      if (ne >= 1u && surv_a == 1u) single_end_direct(mem_a, RA, false);
      if (ne == 2u && surv_b == 1u) single_end_direct(mem_b, RB, true);
    } else {
      if (ne >= 1u && surv_a == 1u) single_end(mem_a, lc_a, offA);
      if (ne == 2u && surv_b == 1u) single_end(mem_b, lc_b, offB);
    }
    // one run over both ends when they have equally many rows, else a run per end (the classic builds: ONE copy of the loop in the code)
    const bool both = multi_a && multi_b && m_a == m_b;
    const uint32_t nruns = both ? 1u : (multi_a ? 1u : 0u) + (multi_b ? 1u : 0u);
    if constexpr (COLS == 1) {
      // the packed pass WITHOUT the loop: the second run — ends of unequal row counts, rare — is a copy of its own behind the first.  A loop around
      // a body with divergent branches is structurized as a whole: every `return` of the pass became a lane mask carried round the loop in a pair
      // of scalar registers, eight pairs in all, and the family's uniforms went to spill lanes to make room for them.
      // (false: a shape the test at the top let through and the pass refuses — the next launch, run_cols)
      if (nruns != 0u) {
        const bool run_a = both || multi_a;
        if (!run_cols_packed(run_a ? lc_a : 0u, (both || !run_a) ? lc_b : 0u, run_a ? m_a : m_b, nruns == 1u)) gone = true;
      }
      if (nruns == 2u && !gone) { if (!run_cols_packed(0u, lc_b, m_b, true)) gone = true; }
    } else {
#pragma unroll 1
      for (uint32_t ri = 0; ri < nruns && !gone; ri++) {
        const bool first_is_a = both || multi_a;
        const bool run_a = ri == 0 && first_is_a, run_b = both || !run_a;
        const uint32_t rc_a = run_a ? lc_a : 0u, rc_b = run_b ? lc_b : 0u, rc_m = run_a ? m_a : m_b;
        run_cols(rc_a, rc_b, rc_m);
      }
    }
    // no room behind the tile for the columns that wait for k_call_full: the next launch of this kernel has larger slices (a family of a noisy
    // library); the last one hands the family to k_simplex_wave2.
    if (gone) { if (gone_far) to_route(); else to_retry(); return; }
  }
  PH(6)
  S2_ABLATE_AFTER(6, icnt + rej + ov_bases + ov_corr)

  // ---- 7. the family's result for k_split_finish (EndDescs, record sizes, counters: a thread per family there) ----------------------
  // reserve room for this family's items (the result is looked at after the store below)
  uint32_t ires = 0;
  if (ires_asked) ires = ires_early;
  else if (icnt && lane == 0) ires = atomicAdd(&KA::of(P).full_count[my_list], icnt);
  if constexpr (COLS != 1) {
    leave(COLS == 1 ? (__any(dirty_v != 0u) ? 0x81u : 0xC1u) : 1u, (ne << 8) | (type_a << 16) | (fk_a << 24), fk_b | (surv_a << 8) | (surv_b << 16) | (n << 24), lc_a | (lc_b << 16), rej, ov_agree, ov_dis);
    if (lane == 0) ((uint32_t*)&P.split_out[g])[6] = ov_corr;
  }
  if constexpr (DIRECT != 0) {
    // ---- 7b. what the rest of each record needs: the depth statistics (cD / cM here, the sum for cE), the patch descriptors ----
    // depth statistics over the wavefront: max / min of both ends two to a register, the sums likewise (an end's sum < 2^16: at most
    // 4000 columns of at most 16 reads)
    uint32_t mx = acc_max, mn = acc_min, sm = acc_sum;
    for (int o = 32; o > 0; o >>= 1) { mx = s2_pkmax(mx, (uint32_t)__shfl_xor((int)mx, o)); mn = s2_pkmin(mn, (uint32_t)__shfl_xor((int)mn, o)); sm += (uint32_t)__shfl_xor((int)sm, o); }
    mx = uni(mx); mn = uni(mn); sm = uni(sm);
    // (header, name and tags of the records are k_split_finish's: a thread per family there, 64 families to a vector instruction, where
    // this wavefront would spend ~450 instructions on ~230 bytes with a dozen lanes busy)
    auto tail = [&](const S2DirRec& R, uint32_t sumd) {
      if (lane == 0) {
        SlotDesc sd; sd.out_off = dir_off_early + R.base; sd.lc_seq = R.Lc | (R.o_seq << 16); sd.sum_depth = sumd;
        P.slot_desc[slot0 + R.type] = sd;
      }
    };
    if (ne >= 1u) tail(RA, sm & 0xFFFFu);
    if (ne == 2u) tail(RB, sm >> 16);
    if (lane == 0) ((uint32_t*)&KA::of(P).split_out[g])[7] = (mx & 0xFFu) | ((mn & 0xFFu) << 8) | (((mx >> 16) & 0xFFu) << 16) | (((mn >> 16) & 0xFFu) << 24);   // cD / cM of both records
    dir_tables(type_a == 0u ? RA.size : 0u, type_a == 0u ? 0u : RA.size, RB.size);
  }
  uint32_t fr_first = 0;                // where the family's items lie, for the pair writer (fastpath.h, FullResult): first slot of the pool, in one piece
  bool fr_whole = true;
  if (icnt) {   // the family's items: LDS -> the reserved range, 16 bytes per lane and step; a range that crosses the end of its list
                // continues in the next list (one more, synchronous, reservation — rare)
    wave_sync();
    const auto& K7 = KA::of(P);
    const uint32_t full_cap = K7.full_cap;
    FullItem* const full_items = K7.full_items;
    uint32_t base = uni(ires), l = my_list, done = 0, tries = 0;
    bool overflow = false;
    if (multi_items) {
      // a column of several consecutive items must not be cut at the end of a list: the reservation that does not hold the WHOLE family is
      // filled with continuation items (k_call_full skips them) and the family's items go to the next list that holds them all
      for (;;) {
        if (full_range_whole(base, icnt, full_cap)) {
          const uint4* src = (const uint4*)(W + ibase);
          uint4* dst = (uint4*)(full_items + ((size_t)l * full_cap + base));
          for (uint32_t c = lane; c < 3 * icnt; c += 64) dst[c] = src[c];
          fr_first = l * full_cap + base;
          break;
        }
        if (base < full_cap) {
          FullItem* pad = full_items + ((size_t)l * full_cap + base);
          for (uint32_t c = lane; c < full_cap - base; c += 64) { pad[c].dest = 0; pad[c].obs = 0; pad[c].chains = FULL_ITEM_CONT; }
        }
        if (++tries >= N_LISTS) { overflow = true; break; }
        l = (l + 1) & (N_LISTS - 1);
        uint32_t b2 = 0;
        if (lane == 0) b2 = atomicAdd(&KA::of(P).full_count[l], icnt);
        base = uni(b2);
      }
    } else {
    fr_whole = full_range_whole(base, icnt, full_cap);          // (a range that crosses the end of its list is cut: k_call_full scatters that family's answers)
    fr_first = l * full_cap + base;
    for (;;) {
      const uint32_t rem = icnt - done;
      const uint32_t fit = base < full_cap ? (rem < full_cap - base ? rem : full_cap - base) : 0u;
      const uint4* src = (const uint4*)(W + ibase) + 3 * done;
      uint4* dst = (uint4*)(full_items + ((size_t)l * full_cap + base));
      for (uint32_t c = lane; c < 3 * fit; c += 64) dst[c] = src[c];
      done += fit;
      if (done == icnt) break;
      if (++tries >= N_LISTS) { overflow = true; break; }
      l = (l + 1) & (N_LISTS - 1);
      uint32_t b2 = 0;
      if (lane == 0) b2 = atomicAdd(&KA::of(P).full_count[l], icnt - done);
      base = uni(b2);
    }
    }
    if (overflow) {   // every list is full: the general path redoes the family (its result is withdrawn: no records, nothing counted)
      leave(3u, 0, 0, 0, 0, 0, 0);
      if (DIRECT) dir_tables(0, 0, 0);                         // (its records are in place already: the host takes the batch through the merge)
      if (lane == 0) { uint32_t kk = atomicAdd(KA::of(P).n_deferred, 1u); KA::of(P).deferred[kk] = g; }
      return;
    }
  }
  // (packed build, scratch path) the range, in the 64-bit word `col_off` of the family's fragment EndDesc — k_split_finish touches only `valid` there
  if constexpr (COLS == 1 && DIRECT == 0) { if (lane == 0) KA::of(P).ends[slot0].col_off = full_range_word(fr_first, icnt, fr_whole); }
  (void)fr_first; (void)fr_whole;
  PH(8)
}

template <int QS_T, int SS_T, int DIRECT, int COLS>   // row strides of the quality / sequence tiles (0, 0: the family's own, from its descriptor); DIRECT 1: the
                                            // family's consensus records are written here, at the offsets k_split_parse's sizes gave (fastpath.h).
                                            // COLS 0: every family, 64 columns per pass (run_cols); COLS 1: the families of s2_packed_shape, the packed
                                            // pass only; COLS 2: run_cols for every OTHER family (the two are launched over the same families, each
                                            // leaves the other's alone: the packed pass in a kernel of its own keeps its registers, and run_cols its)
__global__ __launch_bounds__(256, COLS == 1 ? FGX_S2_OCC_PACKED : FGX_S2_OCC) void k_split_cols(FastParams P, uint32_t n_grp_total) {
  FGX_DYN_LDS(dyn);
  typedef typename S2SharedOf<COLS>::type S2Shared;
  __shared__ __align__(16) S2Shared sL;
  typedef s2_u32x4 u32x4;
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t gi_raw = blockIdx.x * (blockDim.x >> 6) + wv;
  bool bail = gi_raw >= n_grp_total;                        // a wavefront without a family still takes part in the table copy
  const uint32_t gi = bail ? 0u : gi_raw;
  const uint32_t g = P.group_list ? P.group_list[gi] : P.g0 + gi;
  if constexpr (COLS != 0) {
    // two launches over the same families: a workgroup that holds none of THIS kernel's families leaves before it loads anything else
    if (COLS == 2 || P.s2_partner) {
      bool other = true;
      if (!bail) {
        const u32x4 e0 = ((const u32x4*)&P.split_fam[g])[0], e1 = ((const u32x4*)&P.split_fam[g])[1];
        other = s2_packed_shape((e0.w >> 8) & 0xFFu, (e0.w >> 16) & 0xFFu, e1.y & 0xFFFFu, e1.y >> 16, P.s2_nsafe) != (COLS == 1);
      }
      if (__syncthreads_and(other ? 1 : 0)) return;
    }
  }
  // the table image: global -> registers now, registers -> LDS after the family's loads have left (one barrier)
  constexpr bool TINY = FGX_S2_F32 && COLS == 1;          // the packed build reads the cap and S2Lds::t1 only
  constexpr uint32_t IMG_V = TINY ? 0u : (uint32_t)((FGX_S2_F32 ? S2_HEAD_BYTES : (uint32_t)sizeof(S2Lds)) / 16);   // (f32 sums: the gate tables and the f32 pairs only)
  static_assert(IMG_V <= 6 * 64 || !FGX_S2_F32, "table image larger than six loads per thread");
  const u32x4* const img_src = (const u32x4*)P.s2_image;
  u32x4 im[6];
  uint32_t tiny_w = 0;
  if constexpr (TINY) {
    static_assert(offsetof(S2Lds, t1) % 4 == 0 && offsetof(GateTables, cap) % 4 == 0, "the packed build copies its tables as 32-bit words");
    const uint32_t* const w = (const uint32_t*)P.s2_image;
    if (threadIdx.x < 24u) tiny_w = w[offsetof(S2Lds, t1) / 4 + threadIdx.x];
    else if (threadIdx.x == 24u) tiny_w = w[(offsetof(S2Lds, g) + offsetof(GateTables, cap)) / 4];
  } else {
#pragma unroll
    for (int u = 0; u < 6; u++) { const uint32_t ii = threadIdx.x + u * blockDim.x; im[u] = img_src[ii < IMG_V ? ii : 0u]; }
  }
  uint8_t* W = dyn + (size_t)wv * P.lds_wave_bytes;
  const uint32_t my_list = blockIdx.x & (N_LISTS - 1);
  s2_cols_family<QS_T, SS_T, DIRECT, COLS, false>(P, g, bail, tiny_w, im, W, sL, lane, my_list);
}

// -----------------------------------------------------------------------------------------------------------------------------
// k_split_finish — a thread per family: the EndDescs and record sizes of the families k_split_cols finished, and the batch counters
// (summed over the wavefront before they touch memory).  In k_split_cols this was lane 0's work: ~220 vector instructions per
// family at 1 / 64 lane use.
// -----------------------------------------------------------------------------------------------------------------------------
// Launched per chunk of the first column-kernel launch (families P.g0 .. P.g0 + count) and per later launch (its family list): a family
// that a launch handed on (status 0) is left alone, and found again in the list of the launch that finishes it.
__global__ __launch_bounds__(256) void k_split_finish(FastParams P, uint32_t count) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  uint32_t c_total = 0, c_cons = 0, c_insuf = 0, c_zero = 0, c_orphan = 0, c_agree = 0, c_dis = 0, c_corr = 0, c_packed = 0, c_classic = 0, c_clean = 0;
  uint32_t c_ovp = 0, c_ovb = 0, c_ovg = 0;                 // (fgx_debug_last_packed_overlap: the packed build's families with overlapping mates by the step that corrected them)
  uint32_t c_apply = 0, c_cut = 0, c_over = 0;               // (fgx_debug_last_full_results: families whose answers the pair writer applies / refused because their items are not in one piece)
  if (gi < count) {
    const uint32_t g = P.group_list ? P.group_list[gi] : P.g0 + gi;
    const SplitOut O = P.split_out[g];
    const uint32_t slot0 = 3 * g;
    const uint32_t o_status = O.status & 0x3Fu;
    const bool padded = (O.status & 0x80u) != 0;   // finished by the packed build: its scratch layout (S2_PAD_FRONT / s2_padded_b)
    const bool clean = (O.status & 0x40u) != 0;    // ... by its clean row loop (no quality read), else by the general one
    if (o_status == 2) { c_total = O.n; c_insuf = O.n; }
    const bool direct = P.out != nullptr;      // k_split_cols wrote the records (and the slots of the offset / size tables) itself: counters only
    if (o_status != 0 && !direct) {
      EndDesc* D = &P.ends[slot0];
      D[0].valid = 0; D[1].valid = 0; D[2].valid = 0;
      P.rec_sizes[slot0] = 0; P.rec_sizes[slot0 + 1] = 0; P.rec_sizes[slot0 + 2] = 0;
    }
    if (o_status == 1) {
      c_packed = padded ? 1u : 0u; c_classic = padded ? 0u : 1u; c_clean = (padded && clean) ? 1u : 0u;
      c_total = O.n; c_cons = O.ne;
      c_insuf = O.rej & 0xFF; c_zero = (O.rej >> 8) & 0xFF; c_orphan = O.rej >> 16;
      c_agree = O.ov_agree; c_dis = O.ov_dis; c_corr = O.ov_corr & S2_OV_COUNT;
      if (padded) { c_ovp = (O.ov_corr & S2_OV_PACKED) ? 1u : 0u; c_ovb = (O.ov_corr & S2_OV_BYTEWISE) ? 1u : 0u; c_ovg = (O.ov_corr & S2_OV_GUARD) ? 1u : 0u; }
      const uint4 fd = P.fam_desc[g];
      const unsigned long long lo_off = (unsigned long long)fd.x | ((unsigned long long)fd.y << 32);
      const uint32_t r0 = P.grp_first[g];
      const SplitFam F = P.split_fam[g];
      const SplitRec R0 = P.split_rec[r0];
      const uint64_t col_base = P.col_base[g];
      if (direct) {
        // ---- direct records: everything of the family's records that is not a column — block_size + core, read name, RG, cD / cM / cE, the
        //      headers of cd / ce, MI, cell barcode, RX (vanilla_caller.rs:1767-1881) — at the offsets the column kernel used.  A thread per
        //      family: a vector instruction serves 64 families (the stores scatter, but the memory system has room and this runs under the
        //      next chunk's column kernel).
        const uint8_t* const fbase = P.blob + lo_off;
        const uint8_t* const strs = (const uint8_t*)P.strings;
        const uint32_t mi0 = R0.mi_len, nm = P.prefix_len + 1u + mi0;
        const uint8_t* const mi_src = fbase + R0.mi_rel;
        uint64_t rec_off = P.dir_off[g];
        for (uint32_t k = 0; k < O.ne; k++) {
          const uint32_t Lc = k == 0 ? O.lc_a : O.lc_b, e_type = k == 0 ? O.type_a : 2u;
          const uint32_t fk = k == 0 ? O.fk_a : O.fk_b, kept = k == 0 ? O.kept_a : O.kept_b;
          const uint32_t dst = k == 0 ? O.depth_stats & 0xFFFFu : O.depth_stats >> 16, maxd = dst & 0xFFu, mind = dst >> 8;
          const SplitRec RK = P.split_rec[r0 + fk];
          const bool hcb = P.cell0 && (RK.bits & 8u);
          const uint32_t cbl = RK.cb_len, rxn = F.rx_all ? kept : 0u, rxl = F.rx_len;
          const uint32_t o_seq = 36u + nm + 1u, o_rg = o_seq + ((Lc + 1u) >> 1) + Lc, o_t3 = o_rg + 3u + P.rg_len + 1u;
          const uint32_t o_cd = o_t3 + 15u + 8u, o_ce = o_cd + 2u * Lc + 8u, o_mi = P.per_base_tags ? o_ce + 2u * Lc : o_t3 + 15u;
          const uint32_t o_cb = o_mi + 3u + mi0 + 1u, o_rx = o_cb + (hcb ? 3u + cbl + 1u : 0u), size = o_rx + (rxn ? 3u + rxl + 1u : 0u);
          uint8_t* const q = P.out + rec_off;
          uint32_t flag = bam::F_UNMAPPED;
          if (e_type == 1u) flag |= bam::F_PAIRED | bam::F_FIRST | bam::F_MATE_UNMAPPED;
          else if (e_type == 2u) flag |= bam::F_PAIRED | bam::F_LAST | bam::F_MATE_UNMAPPED;
          // block_size; ref_id -1, pos -1, l_read_name | mapq 0 | bin 4680, n_cigar_op 0 | flag, l_seq, next_ref -1, next_pos -1, tlen 0
          gst32u(q, size - 4u); gst32u(q + 4, 0xFFFFFFFFu); gst32u(q + 8, 0xFFFFFFFFu); gst32u(q + 12, (nm + 1u) | (4680u << 16)); gst32u(q + 16, flag << 16);
          gst32u(q + 20, Lc); gst32u(q + 24, 0xFFFFFFFFu); gst32u(q + 28, 0xFFFFFFFFu); gst32u(q + 32, 0u);
          uint8_t* w = q + 36;                                 // <prefix>:<MI> NUL
          for (uint32_t i = 0; i < P.prefix_len; i++) *w++ = strs[i];
          *w++ = (uint8_t)':';
          for (uint32_t i = 0; i < mi0; i++) *w++ = mi_src[i];
          *w = 0;
          w = q + o_rg;                                        // RG:Z:<id>
          w[0] = 'R'; w[1] = 'G'; w[2] = 'Z'; w += 3;
          for (uint32_t i = 0; i < P.rg_len; i++) *w++ = strs[P.prefix_len + i];
          *w++ = 0;
          // cD cM cE (:1800-1810): depths of at most 16 reads are one signed byte each; cE = 0.0 here, rewritten by k_fix_ce when k_call_full
          // found errors in the record's columns (a column the column kernel decides itself has none)
          gst32u(w, (uint32_t)'c' | ((uint32_t)'D' << 8) | ((uint32_t)'c' << 16) | (maxd << 24));
          gst32u(w + 4, (uint32_t)'c' | ((uint32_t)'M' << 8) | ((uint32_t)'c' << 16) | (mind << 24));
          gst32u(w + 8, (uint32_t)'c' | ((uint32_t)'E' << 8) | ((uint32_t)'f' << 16));
          gst32u(w + 11, 0u);
          if (P.per_base_tags) {
            gst32u(q + o_cd - 8u, (uint32_t)'c' | ((uint32_t)'d' << 8) | ((uint32_t)'B' << 16) | ((uint32_t)'s' << 24)); gst32u(q + o_cd - 4u, Lc);
            gst32u(q + o_ce - 8u, (uint32_t)'c' | ((uint32_t)'e' << 8) | ((uint32_t)'B' << 16) | ((uint32_t)'s' << 24)); gst32u(q + o_ce - 4u, Lc);
          }
          w = q + o_mi;
          w[0] = (uint8_t)P.tag0; w[1] = (uint8_t)P.tag1; w[2] = 'Z'; w += 3;
          for (uint32_t i = 0; i < mi0; i++) *w++ = mi_src[i];
          *w++ = 0;
          if (hcb) {
            const uint8_t* const src = fbase + RK.body_off + RK.cb_rel;
            w[0] = (uint8_t)P.cell0; w[1] = (uint8_t)P.cell1; w[2] = 'Z'; w += 3;
            for (uint32_t i = 0; i < cbl; i++) *w++ = src[i];
            *w++ = 0;
          }
          if (rxn) {
            // consensus UMI (simple_umi.rs:46-117; every read of the family carries the same value): one read = its bytes as they stand;
            // several = A C G T N in either case -> upper case, the rest as it stands
            const uint8_t* const src = fbase + R0.rx_rel;
            w[0] = 'R'; w[1] = 'X'; w[2] = 'Z'; w += 3;
            for (uint32_t i = 0; i < rxl; i++) {
              const uint32_t c0 = src[i], up = c0 & 0xDFu, ix = up - 'A';
              const bool dna = ix < 26u && ((0x00082045u >> ix) & 1u);
              *w++ = (uint8_t)((rxn > 1u && dna) ? up : c0);
            }
            *w++ = 0;
          }
          rec_off += size;
        }
      }
      // (round 7) does the pair writer apply k_call_full's answers for this family (fastpath.h, FullResult)?  The range of its items: the word
      // the packed build left in the fragment slot's descriptor; the pair: emit_pair's own condition on the fields written below.
      const bool fr_pair = P.full_results && !direct && padded && O.ne == 2 && O.type_a == 1;
      const uint64_t fr_word = fr_pair ? P.ends[slot0].col_off : 0ull;
      uint32_t fr_cbl[2] = {0u, 0u}, fr_rxl[2] = {0u, 0u}, fr_size0 = 0u;
      for (uint32_t k = 0; k < (direct ? 0u : (uint32_t)O.ne); k++) {
        const uint32_t Lc = k == 0 ? O.lc_a : O.lc_b, e_type = k == 0 ? O.type_a : 2u;
        const uint32_t fk = k == 0 ? O.fk_a : O.fk_b, kept = k == 0 ? O.kept_a : O.kept_b;
        const SplitRec RK = P.split_rec[r0 + fk];
        const bool hcb = P.cell0 && (RK.bits & 8u);
        const uint32_t rx_cnt = F.rx_all ? kept : 0u, rx_ulen = F.rx_len;
        const uint32_t mi0_len = R0.mi_len, cbl = RK.cb_len;
        const uint32_t nm = P.prefix_len + 1 + mi0_len;
        const uint32_t size = 32 + nm + 1 + (Lc + 1) / 2 + Lc + (3 + P.rg_len + 1) + 4 + 4 + 7 +
                              (P.per_base_tags ? 2 * (8 + 2 * Lc) : 0) + (3 + mi0_len + 1) + (hcb ? 3 + cbl + 1 : 0) +
                              (rx_cnt ? 3 + rx_ulen + 1 : 0);
        // the descriptor as six 16-byte pieces (EndDesc: col_off, first_off | kept_off, cons_len, rec_size | mi_off, cb_off, mi_len, cb_len,
        // rx_len, type, has_cb, has_rx, valid, pad, rx[0..4) | rx[4..20) | rx[20..36) | rx[36..48)): as a local struct it lived in scratch memory
        static_assert(offsetof(EndDesc, kept_off) == 16 && offsetof(EndDesc, mi_off) == 32 && offsetof(EndDesc, rx) == 44 && sizeof(EndDesc) == 96, "EndDesc layout");
        // consensus UMI (simple_umi.rs:46-117; every read of the family carries the same value): one read = its bytes as they stand;
        // several = A C G T in either case -> upper case, N / n -> N, the rest as it stands
        uint32_t rxw[12];
#pragma unroll
        for (uint32_t w = 0; w < 12; w++) {
          uint32_t out = 0;
          if (rx_cnt && 4 * w < rx_ulen) {
            const uint32_t v = gld32(P.blob + lo_off + R0.rx_rel + 4 * w);   // (may read past the value: inside the record / the blob's slack)
#pragma unroll
            for (uint32_t bb = 0; bb < 4; bb++) {
              const uint32_t ch = (v >> (8 * bb)) & 0xFF, up = ch & 0xDFu, idx = up - 'A';
              const bool dna = idx < 26 && ((0x00082045u >> idx) & 1u);
              const uint32_t o = (4 * w + bb < rx_ulen) ? ((rx_cnt > 1 && dna) ? up : ch) : 0u;
              out |= o << (8 * bb);
            }
          }
          rxw[w] = out;
        }
        const uint64_t col_off = col_base + (padded ? (k == 0 ? S2_PAD_FRONT : s2_padded_b(O.lc_a)) : (k == 0 ? 0u : (uint32_t)O.lc_a)), kept_off = lo_off + RK.body_off;
        const u32x4 p0 = {(uint32_t)col_off, (uint32_t)(col_off >> 32), (uint32_t)lo_off, (uint32_t)(lo_off >> 32)};
        const u32x4 p1 = {(uint32_t)kept_off, (uint32_t)(kept_off >> 32), Lc, size};
        const u32x4 p2 = {(uint32_t)R0.mi_rel | ((uint32_t)RK.cb_rel << 16), mi0_len | (cbl << 8) | (rx_ulen << 16) | (e_type << 24),
                          (hcb ? 1u : 0u) | ((rx_cnt ? 1u : 0u) << 8) | (1u << 16), rxw[0]};
        const u32x4 p3 = {rxw[1], rxw[2], rxw[3], rxw[4]}, p4 = {rxw[5], rxw[6], rxw[7], rxw[8]}, p5 = {rxw[9], rxw[10], rxw[11], 0u};
        u32x4* dst = (u32x4*)&P.ends[slot0 + e_type];
        dst[0] = p0; dst[1] = p1; dst[2] = p2; dst[3] = p3; dst[4] = p4; dst[5] = p5;
        P.rec_sizes[slot0 + e_type] = (uint64_t)size + 4;
        fr_cbl[k & 1u] = hcb ? cbl : 0u; fr_rxl[k & 1u] = rx_cnt ? rx_ulen : 0u;
        if (k == 0) fr_size0 = size;
      }
      if (fr_pair) {
        // (both descriptors carry the family's first record and its MI value; R2's columns lie s2_padded_b - S2_PAD_FRONT behind R1's, and
        // its record follows R1's in the scan of the sizes)
        const uint32_t items = (uint32_t)(fr_word >> 32) & 0xFFFFu;
        const bool whole = ((fr_word >> 48) & 1u) != 0;
        const bool taken = emit_pair_takes(O.lc_a, O.lc_b, P.prefix_len + 1u + R0.mi_len, P.rg_len, R0.mi_len, fr_cbl[0], fr_cbl[1], fr_rxl[0], fr_rxl[1], true,
                                           (uint64_t)(s2_padded_b(O.lc_a) - S2_PAD_FRONT), (uint64_t)fr_size0 + 4ull);
        if (full_results_family(true, true, whole, items, taken)) { c_apply = 1u; P.full_flag[g] = 1; }
        else if (taken) { if (!whole) c_cut = 1u; else c_over = 1u; }   // (its answers are scattered: a range cut at a list's end / more items than the writer loads)
      }
    }
  }
  // counters: one atomic per wavefront and counter
  const uint32_t t_cons = wave_sum(c_cons), t_total = wave_sum(c_total), t_insuf = wave_sum(c_insuf), t_zero = wave_sum(c_zero), t_orphan = wave_sum(c_orphan);
  const uint32_t t_agree = wave_sum(c_agree), t_dis = wave_sum(c_dis), t_corr = wave_sum(c_corr);
  const uint32_t t_packed = wave_sum(c_packed), t_classic = wave_sum(c_classic);   // (diagnostics, fgx_debug_last_split_builds: which build finished how many families)
  const uint32_t t_clean = wave_sum(c_clean);                                       // (fgx_debug_last_packed_rows: the packed build's families by row loop)
  const uint32_t t_ovp = wave_sum(c_ovp), t_ovb = wave_sum(c_ovb), t_ovg = wave_sum(c_ovg);   // (fgx_debug_last_packed_overlap: ... by the step that corrected their overlapping mates)
  if (lane == 0) {
    unsigned long long* st = P.stats + (size_t)((blockIdx.x * 4 + (threadIdx.x >> 6)) & (STAT_SLOTS - 1)) * 32;
    if (t_total) atomicAdd(&st[0], (unsigned long long)t_total);
    if (t_cons) atomicAdd(&st[1], (unsigned long long)t_cons);
    const uint32_t filt = t_insuf + t_zero + t_orphan;
    if (filt) atomicAdd(&st[2], (unsigned long long)filt);
    if (t_insuf) atomicAdd(&st[3 + FGX_REJ_INSUFFICIENT_READS], (unsigned long long)t_insuf);
    if (t_zero) atomicAdd(&st[3 + FGX_REJ_ZERO_LENGTH_AFTER_TRIMMING], (unsigned long long)t_zero);
    if (t_orphan) atomicAdd(&st[3 + FGX_REJ_ORPHAN_CONSENSUS], (unsigned long long)t_orphan);
    if (t_agree + t_dis) atomicAdd(&st[24], (unsigned long long)(t_agree + t_dis));
    if (t_agree) atomicAdd(&st[25], (unsigned long long)t_agree);
    if (t_dis) atomicAdd(&st[26], (unsigned long long)t_dis);
    if (t_corr) atomicAdd(&st[27], (unsigned long long)t_corr);
    if (t_packed) atomicAdd(&st[28], (unsigned long long)t_packed);
    if (t_classic) atomicAdd(&st[29], (unsigned long long)t_classic);
    if (t_clean) atomicAdd(&st[30], (unsigned long long)t_clean);
    if (t_packed - t_clean) atomicAdd(&st[31], (unsigned long long)(t_packed - t_clean));
    if (t_ovp | t_ovb) {     // (the slots of the result counters, behind them: the 32 words of a slot above are taken)
      unsigned long long* fs = P.full_stats + (size_t)((blockIdx.x * 4 + (threadIdx.x >> 6)) & (STAT_SLOTS - 1)) * FULL_STATS_STRIDE + FULL_STATS_N;
      if (t_ovp) atomicAdd(&fs[0], (unsigned long long)t_ovp);
      if (t_ovb) atomicAdd(&fs[1], (unsigned long long)t_ovb);
      if (t_ovg) atomicAdd(&fs[2], (unsigned long long)t_ovg);
    }
  }
  if (P.full_results) {
    const uint32_t t_apply = wave_sum(c_apply), t_cut = wave_sum(c_cut), t_over = wave_sum(c_over);
    if (lane == 0) {
      unsigned long long* fs = P.full_stats + (size_t)((blockIdx.x * 4 + (threadIdx.x >> 6)) & (STAT_SLOTS - 1)) * FULL_STATS_STRIDE;
      if (t_apply) atomicAdd(&fs[2], (unsigned long long)t_apply);
      if (t_cut) atomicAdd(&fs[3], (unsigned long long)t_cut);
      if (t_over) atomicAdd(&fs[4], (unsigned long long)t_over);
    }
  }
}
