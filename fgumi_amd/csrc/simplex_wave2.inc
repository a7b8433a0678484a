// simplex_wave2.inc — k_simplex_wave2: the simplex family kernel for the COMMON record shape, built around a
// two-accumulator column loop.  Included by fastpath.hip inside `namespace fgx { namespace {` after the shared wave helpers.
//
// Why a second kernel: k_family_wave<0> spends ≈ 55 vector instructions per observation (three v_readlane, packed-descriptor
// unpacking, a 64-bit LUT shift, eight v_cndmask and SIXTEEN f64 operations for the four Kahan lanes).  The reference
// arithmetic does not need four running sums while a column has shown ONE base so far: the three lanes of the bases not yet
// observed receive the identical sequence `error_per_alt[q_1], error_per_alt[q_2], …` and therefore hold bit-identical
// (sum, compensation) pairs (base_builder.rs:836-868 adds `correct` to the observed lane and `error_per_alt` to the other
// three, lane by lane, in read order).  So a column is accumulated with TWO Kahan chains — `w` for the base seen, `l` for
// "any other base" — = 8 f64 operations per observation, and only when a second distinct base shows up (≈ 0.8 % of the
// columns of a depth-8 family at a 1e-3 error rate) does that lane fan `l` out into the other three lanes and finish the
// remaining reads with the four-lane update.  Results are bit-identical to the four-lane loop by construction.
//
// The loop around it is arranged so that everything that is the same for all 64 columns of a pass is scalar: reads are
// walked in file order by a wave-uniform loop, the read's LDS offsets / length / strand sit in SGPRs (one v_readlane pair per
// read and pass), the per-column byte offsets and nibble shifts of both orientations are computed once per pass, and the
// {correct, error_per_alt} pair table is padded to 256 rows so the quality needs no clamp.  ≈ 18 vector instructions per
// observation instead of ≈ 55.
//
// Shape taken here (everything else goes, untouched, to k_family_wave<0> through the `retry_old` list, which keeps the full
// semantics incl. clips, secondary / supplementary records, --trim, --max-reads): every record primary, mapped, with ONE
// M / = / X CIGAR op spanning the read, MC absent or `<n>M`, coordinates below 2^30, at most 64 records whose raw bytes fit the
// wave's LDS slice; options without --trim; a --max-reads cap that does not bite.
//
// Reference semantics restated: same as k_family_wave<0> (see the header of fastpath.hip).

// a value every lane holds alike, moved to an SGPR: loops and address arithmetic on it become scalar (wave reductions come out of
// cross-lane operations, which the compiler has to assume divergent)

// Mask of the lanes l with p0 + l < limit (both scalar), computed on the scalar unit (the compiler prefers a saturating vector
// subtract + 64-bit vector shift + two v_readfirstlane for the C++ spelling of this).
__device__ __forceinline__ unsigned long long lanes_below(uint32_t limit, uint32_t p0) {
#if defined(FGX_WAVEMU)
  const uint32_t span = (limit > p0 ? limit : p0) - p0;
  return span >= 64u ? ~0ull : ((1ull << span) - 1ull);
#else
  unsigned long long m;
  uint32_t span;
  asm("s_max_u32 %1, %2, %3\n\ts_sub_u32 %1, %1, %3\n\ts_bfm_b64 %0, %1, 0\n\ts_cmp_ge_u32 %1, 64\n\ts_cselect_b64 %0, -1, %0"
      : "=&s"(m), "=&s"(span) : "s"(limit), "s"(p0) : "scc");
  return m;
#endif
}

// index of the lowest set bit of a scalar mask, -1 for an empty one (s_ff1_i32_b64; __builtin_ctzll(0) is undefined)
__device__ __forceinline__ uint32_t first_bit(unsigned long long m) {
#if defined(FGX_WAVEMU)
  return m ? (uint32_t)__builtin_ctzll(m) : 0xFFFFFFFFu;
#else
  uint32_t r;
  asm("s_ff1_i32_b64 %0, %1" : "=s"(r) : "s"(m));
  return r;
#endif
}

// m without bit `bit` (both scalar): one s_bitset0_b64 instead of the 64-bit add / and pair of m & (m - 1)
__device__ __forceinline__ unsigned long long clear_bit(unsigned long long m, uint32_t bit) {
#if defined(FGX_WAVEMU)
  return m & ~(1ull << (bit & 63u));
#else
  asm("s_bitset0_b64 %0, %1" : "+s"(m) : "s"(bit));
  return m;
#endif
}

#ifndef FGX_W2_PAIRS
#define FGX_W2_PAIRS 96   /* entries of the {correct, error} table in LDS: 256 = indexed by the raw quality byte, 96 = clamped index; what a
                             workgroup needs beside its wave slices decides how many workgroups a CU holds */
#endif
#if FGX_W2_PAIRS >= 256
#define W2_PAIR_OFF(q) ((q) << 4)
#else
#define W2_PAIR_OFF(q) (((q) < 93u ? (q) : 93u) << 4)
#endif
__device__ __forceinline__ void load_gate_tables(GateTables& G, const ConsensusTables& t) {
  for (uint32_t i = threadIdx.x; i < 98; i += blockDim.x) { G.thresholds[i] = t.thresholds[i < 93 ? i : 93]; if (i < 94) G.margin_scale[i] = t.margin_scale[i]; }
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) G.qguess[i] = t.qguess[i];
  if (threadIdx.x == 0) { G.cap_threshold = t.cap_threshold; G.half_cerr_at_cap = t.half_cerr_at_cap; G.cap = t.cap; }
}

// Everything k_simplex_wave2 keeps in LDS beside the wave slices, as ONE block: the host builds its image once per caller
// (FastPath::w2_image) and a workgroup copies it with one 16-byte load per thread — issued before the family's own loads and
// written to LDS after them, so its latency hides behind the staging of the records (filling the tables entry by entry from the
// ConsensusTables cost every wavefront ~2 us before its first useful instruction).
struct W2Lds {
  GateTables g;
  alignas(16) double pair[FGX_W2_PAIRS][2];    // {correct[min(q,93)], error_per_alt[min(q,93)]}: one ds_read_b128 per observation
  uint8_t tagcls[256];             // aux value type -> 1 / 2 / 4 (fixed size), 8 (Z), 16 (H), 32 (B), 0 (unknown)
};
static_assert(sizeof(W2Lds) % 16 == 0, "W2Lds is copied in 16-byte pieces");
inline void build_w2_image(W2Lds& L, const ConsensusTables& t) {
  memset(&L, 0, sizeof(L));
  fill_gate_tables(L.g, t);
  for (uint32_t i = 0; i < FGX_W2_PAIRS; i++) { const uint32_t q = i < 93 ? i : 93; L.pair[i][0] = t.correct[q]; L.pair[i][1] = t.error_per_alt[q]; }
  for (uint32_t i = 0; i < 256; i++) { const int fx = bam::tag_fixed_size((uint8_t)i); L.tagcls[i] = (uint8_t)(fx ? fx : i == 'Z' ? 8 : i == 'H' ? 16 : i == 'B' ? 32 : 0); }
}

#define ABLATE_AFTER(k) if (FGX_ABLATE == (k)) return;
#ifndef FGX_V2_OCC
#define FGX_V2_OCC 5
#endif
#ifndef FGX_W2_BATCH
#define FGX_W2_BATCH 2   /* member reads per step of k_simplex_wave2's regular-end loop (their LDS reads are in flight together) */
#endif
#ifndef FGX_V2_MERGE
#define FGX_V2_MERGE 1   /* 1: the tails of two regular ends share one pass (0: measurement builds) */
#endif
#ifndef FGX_V2_BATCH
#define FGX_V2_BATCH 1   /* member reads per step of the column loop (their LDS loads are in flight together) */
#endif

// (W2_OBSERVE, the observation step of the column loop, lives in chain_observe.inc: k_family_wave's duplex sets use it too)

__global__ __launch_bounds__(256, FGX_V2_OCC) void k_simplex_wave2(FastParams P, uint32_t n_grp_total) {
  FGX_DYN_LDS(dyn);
  __shared__ __align__(16) W2Lds sL;
  GateTables& sT = sL.g;
  double (&sPair)[FGX_W2_PAIRS][2] = sL.pair;
  uint8_t* const sTagCls = sL.tagcls;
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t gi_raw = blockIdx.x * (blockDim.x >> 6) + wv;
  bool bail = gi_raw >= n_grp_total;                        // a wavefront without a family still takes part in the table copy
  const uint32_t gi = bail ? 0u : gi_raw;
  // (a retry launch reads its family index from a list: that load goes out BEFORE the table image, so that waiting for it does
  // not wait for the image)
  const uint32_t g = P.group_list ? P.group_list[gi] : P.g0 + gi;
  // the table image: global -> registers now, registers -> LDS after the records have been staged (one barrier for both)
  constexpr uint32_t IMG_V = (uint32_t)(sizeof(W2Lds) / 16);
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  static_assert(IMG_V <= 4 * 64, "table image larger than four loads per thread");   // (64 threads per workgroup at least)
  const uint32_t ii0 = threadIdx.x, ii1 = ii0 + blockDim.x, ii2 = ii1 + blockDim.x, ii3 = ii2 + blockDim.x;
  const u32x4* const img_src = (const u32x4*)P.w2_image;
  const u32x4 im0 = img_src[ii0 < IMG_V ? ii0 : 0u], im1 = img_src[ii1 < IMG_V ? ii1 : 0u], im2 = img_src[ii2 < IMG_V ? ii2 : 0u], im3 = img_src[ii3 < IMG_V ? ii3 : 0u];
  uint8_t* W = dyn + (size_t)wv * P.lds_wave_bytes;
  const uint32_t my_list = blockIdx.x & (N_LISTS - 1);
  bool list_overflow = false;
  // an item straight into one of the global lists: one atomic WITH its return value per call (a memory round trip the wavefront
  // sits out) — the fallback of the wave-local list below
  auto push_direct = [&](bool need, uint64_t dest, const double* ll, uint32_t obs_packed, uint32_t chains) {
    list_overflow |= push_full_global(P, lane, my_list, need, dest, ll, obs_packed, chains);
  };
  unsigned long long* st = P.stats + (size_t)(blockIdx.x & (STAT_SLOTS - 1)) * 32;
  // the family's descriptor (k_col_bound) and its first record index: one memory round trip; the record table and the records
  // themselves: the next one
  const uint4 fd = P.fam_desc[g];
  const uint64_t col_base_early = P.col_base[g];              // (used by the column phase: asked for here, with the first round trip)
  const uint32_t r0 = P.grp_first[g], n = uni(fd.w);
  const uint32_t slot0 = 3 * g;
  if (!bail && lane < 3) { P.ends[slot0 + lane].valid = 0; P.rec_sizes[slot0 + lane] = 0; }

  if (!bail && n < P.min_reads) {   // simplex.rs:673-683
    if (lane == 0) { atomicAdd(&st[0], (unsigned long long)n); atomicAdd(&st[2], (unsigned long long)n); atomicAdd(&st[3 + FGX_REJ_INSUFFICIENT_READS], (unsigned long long)n); }
    bail = true;
  }
  // not this kernel's shape: k_family_wave<0> decides (it keeps every rule, and defers what the device cannot decide)
  auto to_old = [&]() { if (lane == 0) { uint32_t k = atomicAdd(P.n_retry_old, 1u); P.retry_old[k] = g; } };
  // fits the shape but not this launch's LDS slice: the next launch of this kernel (bigger slices)
  auto to_retry = [&]() { if (!P.retry) { to_old(); return; } if (lane == 0) { uint32_t k = atomicAdd(P.n_retry, 1u); P.retry[k] = g; } };
  if (!bail && n > 64 && P.big) { if (lane == 0) { uint32_t k = atomicAdd(P.n_big, 1u); P.big[k] = g; } bail = true; }   // no wavefront-per-family kernel takes it: k_family's, directly
  if (!bail && (n > 64 || n == 0)) { to_old(); bail = true; }   // (an empty group has no byte span: k_family_wave<0> defers it)

#if FGX_PHASE_TIMING
  unsigned long long _t = __builtin_amdgcn_s_memtime();
#endif
  // ---- 1. stage the family's raw records into LDS ------------------------------------------------------
  const bool act = !bail && lane < n;
  unsigned long long off = act ? P.rec_off[r0 + lane] : ~0ull;
  uint32_t len = act ? P.rec_len[r0 + lane] : 0;
  // records of a family are normally stored back to back in ascending order: the span is first offset .. last end (the descriptor);
  // anything else — a record outside that span — is k_family_wave<0>'s
  const unsigned long long lo_off = uniform_u64((unsigned long long)fd.x | ((unsigned long long)fd.y << 32));
  const uint32_t span0 = uni(fd.z);
  const unsigned long long hi_end = lo_off + span0;
  if (!bail && (span0 == 0xFFFFFFFFu || hi_end > P.blob_len)) { to_old(); bail = true; }
  const unsigned long long base16 = lo_off & ~15ull;
  const unsigned long long span = hi_end - base16;
  if (!bail && span + 16 > (unsigned long long)P.lds_wave_bytes) { to_retry(); bail = true; }   // +16: slack for the dword-composed reads
  const uint32_t span16 = bail ? 0u : ((uint32_t)span + 15) & ~15u;
  {
    const uint8_t* src = P.blob + base16;
    for (uint32_t i = lane * 16; i < span16; i += 64 * 16) *(uint4*)(W + i) = *(const uint4*)(src + i);
  }
  if (!bail && __any(act && (len < 32 || off < lo_off || off + len > hi_end))) { to_old(); bail = true; }   // a record outside the staged span
  // Columns (and UMI characters) that need the full call are collected in the unused tail of this wavefront's LDS slice and
  // appended to a global list ONCE per family: the reservation (an atomic with a return value) is issued after the UMI phase and
  // its result is used after the descriptors are written — nobody waits for it.  (One atomic per pass that had such a column
  // cost the wavefront ~1.8 memory round trips per family.)
  const uint32_t ibase = span16 + 16;                         // (the 16 bytes after the records are read, never written, by dword-composed loads)
  const uint32_t icap = uni(P.lds_wave_bytes > ibase ? (P.lds_wave_bytes - ibase) / (uint32_t)sizeof(FullItem) : 0u);
  uint32_t icnt = 0;
  static_assert(sizeof(FullItem) == 48, "FullItem is moved as three 16-byte pieces");
  auto push_full = [&](bool need, uint64_t dest, const double* ll, uint32_t obs_packed, uint32_t chains) {
    const unsigned long long m = __ballot(need);
    if (!m) return;
    const uint32_t cnt = (uint32_t)__popcll(m);
    if (icnt + cnt > icap) { push_direct(need, dest, ll, obs_packed, chains); return; }   // no room left in the slice (rare)
    if (need) {
      FullItem* it = (FullItem*)(W + ibase) + (icnt + (uint32_t)__popcll(m & ((1ull << lane) - 1)));
      it->dest = dest; it->ll[0] = ll[0]; it->ll[1] = ll[1]; it->ll[2] = ll[2]; it->ll[3] = ll[3];
      it->obs = obs_packed; it->chains = chains;
    }
    icnt = uni(icnt + cnt);
  };
  {
    u32x4* const img_dst = (u32x4*)&sL;
    if (ii0 < IMG_V) img_dst[ii0] = im0;
    if (ii1 < IMG_V) img_dst[ii1] = im1;
    if (ii2 < IMG_V) img_dst[ii2] = im2;
    if (ii3 < IMG_V) img_dst[ii3] = im3;
  }
  __syncthreads();                                            // the tables (workgroup) and this wavefront's records are in LDS
  if (bail) return;

  PH(1)
  ABLATE_AFTER(1)
  // ---- 2. parse: lane r owns record r ---------------------------------------------------------------------
  const uint32_t lo = act ? (uint32_t)(off - base16) : 0;       // LDS offset of this lane's record
  uint32_t flags = 0, l_seq = 0, seq_lo = 0, qual_lo = 0, name_len = 0, clip = 0, hash = 0;
  int32_t pos = 0, ref_id = 0;
  uint32_t mi_lo = 0, mi_len = 0, rx_lo = 0, rx_len = 0, cb_lo = 0, cb_len = 0;   // LDS offsets of tag values
  bool has_mi = false, has_rx = false, has_cb = false, odd = false;
  if (act) {
    const record::FixedHeader H = record::decode_header(ld32u(W, lo), ld32u(W, lo + 4), ld32u(W, lo + 8), ld32u(W, lo + 12), ld32u(W, lo + 16));
    const record::Layout lay = record::layout(H, len);
    l_seq = H.l_seq; flags = H.flags;
    const bool unm = (flags & bam::F_UNMAPPED) != 0;          // an unmapped record: a read without a CIGAR — l_seq query bases, ref_id / pos unused
    if (lay.odd || record::streaming_header_odd(H, 1u, true, 0u)) odd = true;
    else {
      name_len = H.l_name - 1;
      ref_id = unm ? unmapped_ref_key(lane) : H.ref_id; pos = H.pos;
      seq_lo = lo + lay.seq_off; qual_lo = lo + lay.qual_off;
      if (record::streaming_flags_odd(H, false)) odd = true;
      if (!unm && !record::single_block_op(ld32u(W, lo + 32 + H.l_name), l_seq)) odd = true;
      // aux walk in LDS (tags.rs:13-34): first occurrence of MC / <tag> / RX / <cell tag>
      AuxTags ax;
      aux_walk(W, sTagCls, lo + lay.aux_off, len - lay.aux_off, P, ax);
      if (ax.oddw) odd = true;
      const record::TagFields tg = record::unpack_tags(ax);
      has_mi = tg.has_mi; mi_lo = tg.mi_lo; mi_len = tg.mi_len;
      has_rx = tg.has_rx; rx_lo = tg.rx_lo; rx_len = tg.rx_len;
      has_cb = tg.has_cb; cb_lo = tg.cb_lo; cb_len = tg.cb_len;
      if (!odd && tg.has_mc && !(flags & (bam::F_UNMAPPED | bam::F_MATE_UNMAPPED))) {   // (either of them: no clip, whatever MC says)
        // this read and its mate are both one M op, the mate in [0, 2^30): the closed form; anything else is not this kernel's
        const uint32_t ML = record::mc_single_m(tg.mc_len, [&]() { return ld64u(W, tg.mc_lo); });
        const record::MateFields M = record::decode_mate(ld32u(W, lo + 20), ld32u(W, lo + 24));
        if (ML == 0 || !record::mate_in_range(M)) odd = true;
        else clip = record::single_m_mate_clip(H, ref_id, M, (int32_t)ML);        // <= l_seq <= 65535
      }
      if (!odd) hash = record::name_hash30(name_len, [&](uint32_t o) { return ld32u(W, lo + 32 + o); }, [&](uint32_t o) { return ld64u(W, lo + 32 + o); });
    }
  }
  const uint32_t mi0_lo = rlane(mi_lo, 0), mi0_len = rlane(mi_len, 0);
  if (lane == 0 && record::first_record_odd(has_mi, mi_len, P.prefix_len)) odd = true;
  if (act && !odd && W[qual_lo] == 0xFF) odd = true;                              // absent qualities (:1119-1124): the first one decides here
  if (__any(odd)) { to_old(); return; }
  if (__any(act && (flags & bam::F_UNMAPPED)) && mixed_unmapped_end(act, flags, [](bool p) { return __ballot(p); })) { to_old(); return; }
  const bool cand = act;                  // no secondary / supplementary records in this shape
  const bool rev = (flags & bam::F_REVERSE) != 0;
  const unsigned long long rxmask = __ballot(cand && has_rx), cbmask = __ballot(cand && has_cb);

  PH(2)
  ABLATE_AFTER(2)
  // ---- 3. overlapping-bases pre-correction in LDS (overlapping.rs:236-336, 627-684) ----------------------
  uint32_t ov_bases = 0, ov_agree = 0, ov_dis = 0, ov_corr = 0;
  if (P.overlap) {
    // pair map: per name, the LAST R1-type and the LAST R2-type primary record; an R1 is paired unless a later R1 has its name.
    // All-pairs by rotation: step k compares lane l with lane (l + k) mod n by name hash; the names are verified afterwards.
    const uint32_t ty = !cand ? 0u : (flags & bam::F_FIRST) ? 1u : (flags & bam::F_LAST) ? 2u : 0u;
    const uint32_t kh = (hash << 2) | ty;
    // (key ^ other key) is 0 for an R1 with this R1's hash and 3 for an R2 with it; selects and max only, no lane-mask branches
    int cmate = -1, clater = -1;
    for (uint32_t k = 1; k < n; k++) {
      const uint32_t up = lane + k;
      const bool wrap = up >= n;
      const uint32_t sidx = wrap ? up - n : up;
      const uint32_t d = (uint32_t)__shfl((int)kh, (int)sidx) ^ kh;
      const int as_later = (d == 0 && !wrap) ? (int)sidx : -1;   // a later R1 of this name
      const int as_mate = d == 3 ? (int)sidx : -1;
      clater = as_later > clater ? as_later : clater;
      cmate = as_mate > cmate ? as_mate : cmate;
    }
    if (ty != 1) { cmate = -1; clater = -1; }
    int mate = -1;
    {
      const int other = clater >= 0 ? clater : cmate;
      const uint32_t osl = other >= 0 ? (uint32_t)other : lane;
      const uint32_t lou = (uint32_t)__shfl((int)lo, (int)osl), nlo = (uint32_t)__shfl((int)name_len, (int)osl);
      bool collide = false;
      if (other >= 0) {
        bool same = nlo == name_len;
        for (uint32_t i = 0; i < name_len && same; i += 8) {
          unsigned long long wa = ld64u(W, lou + 32 + i), wb = ld64u(W, lo + 32 + i);
          if (i + 8 > name_len) { unsigned long long mk = (1ULL << (8 * (name_len - i))) - 1; wa &= mk; wb &= mk; }
          if (wa != wb) same = false;
        }
        if (!same) collide = true;                          // equal hashes, different names: the exact rules live in k_family_wave<0>
        else if (clater < 0) mate = cmate;
      }
      if (__any(collide)) { to_old(); return; }
    }
    // shared reference span of each pair, owned by its R1 lane; pair after pair, 64 positions per step
    const int msrc = mate >= 0 ? mate : (int)lane;
    const int32_t pos_b = (int32_t)__shfl((int)pos, msrc), ref_b = (int32_t)__shfl((int)ref_id, msrc);
    const uint32_t len_b = (uint32_t)__shfl((int)l_seq, msrc);
    const uint32_t dsc_a = seq_lo | (qual_lo << 16), dsc_b = (uint32_t)__shfl((int)dsc_a, msrc);
    uint32_t cntp = 0, off12 = 0;
    if (mate >= 0 && ref_id == ref_b) {
      const int32_t s1 = pos + 1, e1 = pos + (int32_t)l_seq, s2 = pos_b + 1, e2 = pos_b + (int32_t)len_b;
      const int32_t lox = s1 > s2 ? s1 : s2, hix = e1 < e2 ? e1 : e2;
      if (hix >= lox) { cntp = (uint32_t)(hix - lox + 1); off12 = (uint32_t)(lox - s1) | ((uint32_t)(lox - s2) << 16); }
    }
    for (unsigned long long om = __ballot(cntp != 0); om; om &= om - 1) {
      const uint32_t a = (uint32_t)__builtin_ctzll(om);
      const uint32_t da = rlane(dsc_a, a), db = rlane(dsc_b, a), oo = rlane(off12, a), cn = rlane(cntp, a);
      const uint32_t sa = da & 0xFFFF, qa0 = da >> 16, sb = db & 0xFFFF, qb0 = db >> 16;
      // lane addresses advance by whole chunks (64 positions = 32 sequence bytes): nibble parities are fixed per pair
      const uint32_t i1 = (oo & 0xFFFF) + lane, i2 = (oo >> 16) + lane;
      uint32_t o1 = sa + (i1 >> 1), o2 = sb + (i2 >> 1), q1 = qa0 + i1, q2 = qb0 + i2;
      const uint32_t sh1 = (~i1 & 1) << 2, sh2 = (~i2 & 1) << 2;
      for (uint32_t w = lane; w < cn; w += 64, o1 += 32, o2 += 32, q1 += 64, q2 += 64) {
        const uint32_t c1 = ((uint32_t)W[o1] >> sh1) & 15, c2 = ((uint32_t)W[o2] >> sh2) & 15;
        if ((c1 > c2 ? c1 : c2) != 15) {                      // neither is N
          // agreement: both qualities become min(qa + qb, 93).  Disagreement: the higher quality's base wins with the difference
          // (at least 2); a tie masks both (N, 2).  One select-only path; a changed base is ONE 32-bit LDS atomic — XOR with
          // (old ^ new) nibble: neighbouring lanes own the other nibble of the same byte.
          const uint32_t qa = W[q1], qb = W[q2];
          const bool agree = c1 == c2;
          const uint32_t sm = qa + qb, nq = sm < 93 ? sm : 93;
          const int32_t d = (int32_t)qa - (int32_t)qb;
          const uint32_t ad = (uint32_t)(d < 0 ? -d : d), dq = ad < FGX_MIN_PHRED ? (uint32_t)FGX_MIN_PHRED : ad;
          const uint32_t cb = d == 0 ? 15u : d > 0 ? c1 : c2;
          const uint32_t newq = agree ? nq : dq;
          const uint32_t x1 = agree ? 0u : (c1 ^ cb), x2 = agree ? 0u : (c2 ^ cb);
          atomicXor((uint32_t*)(W + (o1 & ~3u)), x1 << (8 * (o1 & 3) + sh1));
          atomicXor((uint32_t*)(W + (o2 & ~3u)), x2 << (8 * (o2 & 3) + sh2));
          W[q1] = (uint8_t)newq; W[q2] = (uint8_t)newq;
          ov_agree += agree ? 1u : 0u;
          ov_dis += agree ? 0u : 1u;
          ov_corr += agree ? ((nq != qa || nq != qb) ? 1u : 0u) : 2u;
        }
      }
    }
    ov_bases = ov_agree + ov_dis;
  }
  wave_sync();

  PH(3)
  ABLATE_AFTER(3)
  // ---- 4. source-read length per lane (vanilla_caller.rs:1129-1160; no --trim in this shape) ------------------
  // final length = the read up to the mate clip, without its trailing N / masked bases
  const uint32_t min_bq = uni((uint32_t)P.min_input_bq & 0xFFu);
  auto view = [&](uint32_t s_lo, uint32_t q_lo, uint32_t L, bool rv, uint32_t p, uint32_t* code, uint32_t* qual) {
    const uint32_t idx = rv ? L - 1 - p : p;
    const uint32_t bb = W[s_lo + (idx >> 1)];
    uint32_t c = (bb >> ((~idx & 1) << 2)) & 15;
    uint32_t q = W[q_lo + idx];
    if (rv) c = comp_code((uint8_t)c);
    if (q < min_bq) { c = 15; q = FGX_MIN_PHRED; }      // p < trim_to == L always
    *code = c; *qual = q;
  };
  uint32_t final_len = 0;
  {
    const uint32_t fl = l_seq > clip ? l_seq - clip : 0;
    bool tail_n = false;
    if (cand && fl > 0) { uint32_t c, q; view(seq_lo, qual_lo, l_seq, rev, fl - 1, &c, &q); tail_n = (c == 15); }
    final_len = cand ? fl : 0;
    for (unsigned long long tm = __ballot(tail_n); tm; tm &= tm - 1) {
      const uint32_t r = (uint32_t)__builtin_ctzll(tm);
      uint32_t flr = rlane(final_len, r);
      const uint32_t s_r = rlane(seq_lo, r), q_r = rlane(qual_lo, r), L_r = rlane(l_seq, r);
      const bool rv_r = (rlane(flags, r) & bam::F_REVERSE) != 0;
      while (flr > 0) {
        bool real = false;
        if (lane < flr) { uint32_t c, q; view(s_r, q_r, L_r, rv_r, flr - 1 - lane, &c, &q); real = (c != 15); }
        unsigned long long bm = __ballot(real);
        if (bm) { flr -= (uint32_t)__builtin_ctzll(bm); break; }
        flr -= flr < 64 ? flr : 64;
      }
      if (lane == r) final_len = flr;
    }
  }

  PH(4)
  ABLATE_AFTER(4)
  // ---- 5. family gates with ballots (process_group :1329-1422, process_subgroup :1454-1646) -----------------
  uint32_t rej = 0;        // rejected reads by reason, packed: insufficient | zero-length << 8 | orphan << 16 (each <= 64); the rest derives
                           // (total = n, consensus reads = ne, filtered = the sum): scalar registers are scarce in this kernel
  bool go = true;
  if (n < P.min_reads) { rej += n; go = false; }
  uint32_t my_end = 255;
  if (cand) { if (!(flags & bam::F_PAIRED)) my_end = 0; else if (flags & bam::F_FIRST) my_end = 1; else my_end = 2; }
  bool ok[3] = {false, false, false};
  unsigned long long mem[3] = {0, 0, 0};
  uint32_t surv[3] = {0, 0, 0}, clen[3] = {0, 0, 0};
  bool bites = false;
  if (go) {
#pragma unroll
    for (uint32_t e = 0; e < 3; e++) {
      unsigned long long in_e = __ballot(my_end == e);
      uint32_t cnt = (uint32_t)__popcll(in_e);
      if (cnt == 0) continue;
      if (cnt < P.min_reads) { rej += cnt; continue; }
      unsigned long long kept = __ballot(my_end == e && final_len > 0);
      uint32_t rem = (uint32_t)__popcll(kept), zero = cnt - rem;
      rej += zero << 8;
      if (rem < P.min_reads) { rej += rem; continue; }
      if (P.max_reads >= 0 && (long long)rem > P.max_reads) { bites = true; continue; }   // downsampling: k_family_wave<0>
      bool mine = (kept >> lane) & 1;
      const uint32_t f0 = rlane(final_len, (uint32_t)__builtin_ctzll(kept));
      if (__all(!mine || final_len == f0)) clen[e] = f0;     // one final length (the usual family): it is the consensus length under either rule
      else if (P.min_reads == 1) clen[e] = uni(wave_max(mine ? final_len : 0));
      else {
        uint32_t ge = 0;
        for (unsigned long long m = kept; m; m &= m - 1) { uint32_t fj = rlane(final_len, (uint32_t)__builtin_ctzll(m)); ge += (fj >= final_len) ? 1 : 0; }
        clen[e] = uni(wave_max((mine && ge >= P.min_reads) ? final_len : 0));
      }
      mem[e] = kept; surv[e] = rem; ok[e] = true;
    }
  }
  if (bites) { to_old(); return; }
  const bool has_frag = ok[0], has_pair = ok[1] && ok[2];
  // a fragment consensus AND a pair from one family (three consensus reads) is rare: k_family_wave<0> takes it, and everything
  // per end below is held twice instead of three times (scalar registers are what this kernel runs out of)
  if (has_frag && has_pair) { to_old(); return; }
  uint32_t e_type[2], e_len[2], e_coloff[2];
  unsigned long long e_mem[2];
  const uint32_t ne = (has_frag ? 1u : 0u) + (has_pair ? 2u : 0u);
  e_type[0] = has_frag ? 0u : 1u; e_len[0] = has_frag ? clen[0] : clen[1]; e_mem[0] = has_frag ? mem[0] : mem[1];
  e_type[1] = 2u; e_len[1] = clen[2]; e_mem[1] = mem[2];
  if (!has_pair) { if (ok[1]) rej += surv[1] << 16; else if (ok[2]) rej += surv[2] << 16; }
  uint32_t total_cols = 0;
#pragma unroll
  for (uint32_t k = 0; k < 2; k++) if (k < ne) { e_coloff[k] = total_cols; total_cols += e_len[k]; }

  // UMIs carried by the kept reads of each end; unequal lengths → consensus_umis panics → general path (through the old kernel)
  uint32_t e_rx[2] = {0, 0};                             // reads with a UMI | UMI length << 8 | first such lane << 16 (one scalar per end)
  bool rx_odd = false;
#pragma unroll
  for (uint32_t k = 0; k < 2; k++) {
    if (k >= ne) break;
    unsigned long long with = e_mem[k] & rxmask;
    uint32_t cnt = (uint32_t)__popcll(with);
    if (cnt) {
      const uint32_t f = (uint32_t)__builtin_ctzll(with), ul = rlane(rx_len, f);      // (rx_len <= 255)
      e_rx[k] = cnt | (ul << 8) | (f << 16);
      if (__any(((with >> lane) & 1) && rx_len != ul)) rx_odd = true;
      if (ul > FAST_RX_CAP) rx_odd = true;
    }
  }
  if (rx_odd) { to_old(); return; }

  PH(5)
  ABLATE_AFTER(5)
  // ---- 6. consensus columns ------------------------------------------------------------------------------------
  // One lane per column, 64 columns per pass; the member reads of the end are walked in file order by a wave-uniform loop.
  const DeviceTables* T = P.T;
  const uint64_t col_base = uniform_u64(col_base_early);
  // the family's own scratch columns: scalar base pointers + 32-bit column offsets (no 64-bit vector address arithmetic per store)
  uint8_t* const fam_code = P.col_code + col_base;
  uint8_t* const fam_qual = P.col_qual + col_base;
  uint16_t* const fam_depth = P.col_depth + col_base;
  uint16_t* const fam_err = P.col_err + col_base;
  // per-read descriptors for the scalar broadcast: d0 = seq_lo | rev << 15 | qual_lo << 16 (LDS offsets < 2^15) ; d1 = l_seq | final_len << 16
  const uint32_t d0 = seq_lo | ((rev ? 1u : 0u) << 15) | (qual_lo << 16), d1 = l_seq | (final_len << 16);
  const uint8_t* const pairs = (const uint8_t*)&sPair[0][0];
  // Per end: a single-read end is written at once; a multi-read end gets its strand pattern.  Packed scalars (this kernel runs
  // out of scalar registers before anything else): regs = pattern of end 0 | pattern of end 1 << 2 | multi-read flags << 4,
  // lrevs = Lrev of end 0 | Lrev of end 1 << 16.
  uint32_t regs = 0, lrevs = 0;
#pragma unroll 1
  for (uint32_t k = 0; k < uni(ne); k++) {
    const unsigned long long members = uniform_u64(k == 0 ? e_mem[0] : e_mem[1]);
    const uint32_t Lc = uni(k == 0 ? e_len[0] : e_len[1]);
    const uint32_t coff = uni(k == 0 ? e_coloff[0] : e_coloff[1]);
    const uint32_t mc = (uint32_t)__popcll(members);
    if (mc == 1) {   // single-read consensus: LUT keyed by the unclamped quality (:1677-1708)
      const uint32_t r = (uint32_t)__builtin_ctzll(members);
      const uint32_t s_r = rlane(seq_lo, r), q_r = rlane(qual_lo, r), L_r = rlane(l_seq, r);
      const bool rv_r = (rlane(flags, r) & bam::F_REVERSE) != 0;
      for (uint32_t p = lane; p < Lc; p += 64) {
        uint32_t code, q;
        view(s_r, q_r, L_r, rv_r, p, &code, &q);
        const uint8_t adj = q < 94 ? T->single_input_quals[q] : 0;
        uint8_t ob, oq;
        if (adj < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; } else { ob = (uint8_t)code; oq = adj; }
        const uint32_t oc = coff + p;
        fam_code[oc] = ob; fam_qual[oc] = oq; fam_depth[oc] = (uint16_t)(code != 15 ? 1 : 0); fam_err[oc] = 0;
      }
      continue;
    }
    // Reverse-strand members of one length share their index arithmetic: it is done once per pass for the length of the
    // first reverse member (reads of an end almost always have one length); other lengths recompute it in the loop.
    uint32_t Lrev = 0;
    uint32_t regular = 0;                                     // 1: all forward, 2: all reverse with one l_seq — and one final length
    {
      const unsigned long long rm = members & __ballot(rev);
      if (rm) Lrev = rlane(l_seq, (uint32_t)__builtin_ctzll(rm));
      const bool mine = (members >> lane) & 1;
      const bool odd = mine && (final_len != Lc || (rm != 0 && l_seq != Lrev));
      if (!__any(odd)) regular = rm == 0 ? 1u : rm == members ? 2u : 0u;
      regular = uni(regular);
    }
    regs |= (regular << (2 * k)) | (16u << k);
    lrevs |= Lrev << (16 * k);
  }
  // Pass schedule: 64 columns of one end per pass.  When both ends are regular, have equally many members and each ends in a
  // tail of at most 32 columns (150 = 64 + 64 + 22), ONE merged pass takes both tails — lanes 0..31 the columns of end 0, lanes
  // 32..63 those of end 1, member i of either end in step i — so a 2 x 150 family needs five passes, not six.
  const bool merged_tail = FGX_V2_MERGE && (regs & 48u) == 48u && (regs & 3u) != 0 && (regs & 12u) != 0 &&
                           __popcll(e_mem[0]) == __popcll(e_mem[1]) && ((e_len[0] - 1) & 63u) < 32u && ((e_len[1] - 1) & 63u) < 32u;

  // One pass.  `regular`: 0 = a mixed end, 1 = a regular end, 3 = the merged tail pass (the caller's site fixes which of them exist).
  // p = this lane's column inside its end, oc = its scratch column, ix = its index into a member read (regular ends: one for the
  // whole pass — forward p, reverse (one l_seq) Lrev - 1 - p), lane_rev = its end is a reverse-strand end.
  auto do_pass = [&](auto site_tag, const uint32_t regular, const unsigned long long members, const unsigned long long membersB,
                     const uint32_t p, const bool incol, const uint32_t oc, const uint32_t Lrev, const uint32_t ix,
                     const bool lane_rev, const uint32_t p0s, const bool upper) __attribute__((always_inline)) {
    constexpr int SITE = decltype(site_tag)::value;          // 0: one-end passes (modes 0 and 1), 1: the merged pass (mode 3)
    double s2, c2, s3, c3;                                    // chains 2 / 3: written when opened; until then any value will do, and
    FGX_UNDEF4(s2, c2, s3, c3);
    const uint32_t iq = ix, is = ix >> 1, ish = (~ix & 1) << 2;
    // Kahan chains by order of appearance: chain 1 = the first base seen, chains 2 / 3 = the second / third distinct base,
    // chain R = every base not seen yet (their lanes receive identical additions, so one chain stands for all of them; once
    // three bases have been seen it IS the fourth base).  A column with one base only ever touches chains 1 and R.
    double s1 = 0.0, c1 = 0.0, sR = 0.0, cR = 0.0;
    // What a lane may still take on the hot path, as a bit mask over the 4-bit codes: 0x116 (A C G T = codes 1 2 4 8) while
    // nothing has been seen, 1 << code once one base has been seen, 0 after a second distinct base (or outside the columns
    // of a regular end): `(allow >> code) & 1` is the whole one-hot / same-base test.
    uint32_t allow = (regular != 0 && !incol) ? 0u : 0x116u;
    uint32_t b1 = 0, b2 = 0, b3 = 0;                        // several bases: one-hot codes of chains 1..3, 0 = not opened
    uint32_t n1 = 0, n2 = 0, n3 = 0, nR = 0;                // observations per chain (nR: the fourth base, after three were seen)
    // one observation (q, c, table entry) of a lane that is inside its read (`in`): W2_OBSERVE, a macro — as a nested lambda the
    // chain registers were captured through pointers and the "open chain 2 or 3" assignments became stores through a selected
    // pointer, i.e. scratch memory.
    // Members in file order.  MODE 0: any mix of strands and lengths (per-member strand branch and final-length mask).
    // MODE 1: a regular end — every member forward, or every member reverse with one l_seq, and one final length (= the
    // consensus length): the mask of a pass is `incol` for every member, the index is the lane's for the whole pass, and the
    // codes stay as stored inside the loop: chains are kept by order of appearance, so complementing b1 / b2 / b3 afterwards
    // is the same thing.  Its members go FGX_W2_BATCH at a time: the loop is bound by the latency of its two dependent LDS
    // reads (byte, then table entry), not by instruction issue, so the reads of a batch are in flight together and only the
    // Kahan updates stay in file order.  MODE 3: the merged tail pass of two regular ends.
    if constexpr (SITE == 1) {
      unsigned long long mB = membersB;
      for (unsigned long long m = members; m;) {
        const uint32_t r = (uint32_t)__builtin_ctzll(m), rB = (uint32_t)__builtin_ctzll(mB);
        m = clear_bit(m, r); mB = clear_bit(mB, rB);
        const uint32_t x0 = rlane(d0, r), xB = rlane(d0, rB);
        const uint32_t x = upper ? xB : x0;
        const uint32_t q = W[iq + (x >> 16)];
        const uint32_t c = __builtin_amdgcn_ubfe((uint32_t)W[is + (x & 0x7FFF)], ish, 4u);
        W2_OBSERVE(3, incol, q, c, *(const double2*)(pairs + W2_PAIR_OFF(q)));
      }
    } else if (regular != 0) {
      constexpr int NB = FGX_W2_BATCH;
      for (unsigned long long m = members; m;) {
        uint32_t q_[NB], c_[NB];
        bool on_[NB];
#pragma unroll
        for (int j = 0; j < NB; j++) {
          on_[j] = m != 0;                                    // (uniform; the first of a batch always is)
          const uint32_t r = first_bit(m) & 63u;              // no member left: lane 63's descriptor, a harmless read nobody uses
          m = clear_bit(m, r);
          const uint32_t x0 = rlane(d0, r);
          q_[j] = W[iq + (x0 >> 16)];
          c_[j] = W[is + (x0 & 0x7FFF)];                      // BAM 4-bit codes as stored
        }
        double2 pr_[NB];
#pragma unroll
        for (int j = 0; j < NB; j++) { c_[j] = __builtin_amdgcn_ubfe(c_[j], ish, 4u); pr_[j] = *(const double2*)(pairs + W2_PAIR_OFF(q_[j])); }
#pragma unroll
        for (int j = 0; j < NB; j++) if (j == 0 || on_[j]) W2_OBSERVE(1, incol, q_[j], c_[j], pr_[j]);
      }
    } else {
      // mixed ends: forward index p, reverse index for the length of the first reverse member
      const uint32_t fq = p, fs = p >> 1, fsh = (~p & 1) << 2;
      const uint32_t ir = Lrev > p ? Lrev - 1 - p : 0;
      const uint32_t rq = ir, rs = ir >> 1, rsh = (~ir & 1) << 2;
      for (unsigned long long m = members; m;) {
        const uint32_t r = (uint32_t)__builtin_ctzll(m);
        m = clear_bit(m, r);                                 // (one s_bitset0_b64)
        const uint32_t x0 = rlane(d0, r);
        const uint32_t slo = x0 & 0x7FFF, qlo = x0 >> 16;
        const uint32_t x1 = rlane(d1, r);
        const uint32_t Lr = x1 & 0xFFFF;
        // inside the read's final length: lanes [0, final_len - p0) of this pass — a scalar mask, no vector compare
        const bool in = __builtin_amdgcn_inverse_ballot_w64(lanes_below(x1 >> 16, p0s));
        uint32_t q, c;
        if (!((x0 >> 15) & 1)) {                             // forward strand (wave-uniform branches: the asm statements keep them branches)
          q = W[fq + qlo];
          c = ((uint32_t)W[fs + slo] >> fsh) & 15;
          FGX_MEM_PIN();
        } else {                                             // reverse strand: index from the end
          uint32_t bb;
          if (Lr == Lrev) { q = W[rq + qlo]; bb = (uint32_t)W[rs + slo] >> rsh; FGX_MEM_PIN(); }
          else { const uint32_t jx = Lr > p ? Lr - 1 - p : 0; q = W[jx + qlo]; bb = (uint32_t)W[(jx >> 1) + slo] >> ((~jx & 1) << 2); FGX_MEM_PIN(); }
          c = __builtin_bitreverse32(bb) >> 28;              // complement = bit reversal of the code (A1 C2 G4 T8, IUPAC alike)
        }
        W2_OBSERVE(0, in, q, c, *(const double2*)(pairs + W2_PAIR_OFF(q)));
      }
    }
    if (allow != 0) b1 = (uint32_t)__builtin_ctz(allow);     // one base only (nothing seen: a value nobody reads — n1 == 0, b2 == 0)
    if (regular != 0 && lane_rev) { b1 = __builtin_bitreverse32(b1) >> 28; b2 = __builtin_bitreverse32(b2) >> 28; b3 = __builtin_bitreverse32(b3) >> 28; }
#if FGX_ABLATE == 61 || FGX_ABLATE == 62
    if (incol) fam_depth[oc] = (uint16_t)(n1 + n2 + n3 + nR + (uint32_t)(s1 + sR + s2 + s3));   // keeps the loop alive; no call section
    return;
#endif
    // ---- call ----
    const uint64_t o = col_base + oc;
    bool need_full = false;
    uint32_t depth = 0, q_call = FGX_MIN_PHRED, code_call = 15, err = 0;
    bool resolved = true;
    if (incol) {
      depth = n1 + n2 + n3 + nR;
      if (b2 != 0) resolved = false;                         // two or more distinct bases: never the unanimous fast path
      else if (n1 != 0) {
        uint32_t qq = 0;
        CallConst KC;                                        // read from LDS here: five scalars less to hold across the kernel
        KC.cap = sT.cap; KC.cap_threshold = sT.cap_threshold; KC.half_cerr_at_cap = sT.half_cerr_at_cap;
        resolved = unanimous_call_lds(sT, P.T->t.cerr_min, KC, s1, sR, &qq);
        if (resolved) { q_call = qq; code_call = b1; err = 0; }
      }                                                      // else: no observation → ('N', 2), depth 0
      need_full = !resolved;
      fam_depth[oc] = (uint16_t)depth;                       // (at most 64 member reads: no saturation to apply)
    }
    {   // the chains as they stand; k_call_full sorts them into A, C, G, T (a base never seen reads chain R)
      const double chain[4] = {s1, s2, s3, sR};
      push_full(need_full, o, chain, n1 | (n2 << 8) | (n3 << 16) | (nR << 24), b1 | (b2 << 4) | (b3 << 8));
    }
    if (incol && resolved) {
      uint8_t ob, oq;
      if (depth < P.min_reads) { ob = 15; oq = 0; }
      else if (q_call < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; }
      else { ob = (uint8_t)code_call; oq = (uint8_t)q_call; }
      fam_code[oc] = ob; fam_qual[oc] = oq; fam_err[oc] = (uint16_t)err;
    }
  };

#pragma unroll 1
  for (uint32_t k = 0; k < uni(ne); k++) {
    if (!((regs >> (4 + k)) & 1u)) continue;                  // a single-read end: written above
    const unsigned long long members = uniform_u64(k == 0 ? e_mem[0] : e_mem[1]);
    const uint32_t Lc = uni(k == 0 ? e_len[0] : e_len[1]);
    const uint32_t coff = uni(k == 0 ? e_coloff[0] : e_coloff[1]);
    const uint32_t regular = uni((regs >> (2 * k)) & 3u), Lrev = uni((lrevs >> (16 * k)) & 0xFFFFu);
    const uint32_t Lc_own = uni(merged_tail ? (Lc - 1) & ~63u : Lc);   // without the tail the merged pass takes
    for (uint32_t p0 = 0; p0 < Lc_own; p0 += 64) {
      const uint32_t p0s = uni(p0);                           // (the pass counter, certainly scalar)
      const uint32_t p = p0s + lane;
      const uint32_t ix = regular == 2 ? (Lrev > p ? Lrev - 1 - p : 0u) : p;
      do_pass(std::integral_constant<int, 0>{}, regular != 0 ? 1u : 0u, members, 0ull, p, p < Lc, coff + p, Lrev, ix, regular == 2, p0s, false);
    }
  }
  if (merged_tail) {
    const bool upper = lane >= 32;
    const uint32_t Lc_l = upper ? e_len[1] : e_len[0], Lrev_l = upper ? lrevs >> 16 : lrevs & 0xFFFFu;
    const uint32_t p = (((upper ? e_len[1] : e_len[0]) - 1) & ~63u) + (lane & 31u);
    const bool lane_rev = ((upper ? regs >> 2 : regs) & 3u) == 2u;
    const uint32_t ix = lane_rev ? (Lrev_l > p ? Lrev_l - 1 - p : 0u) : p;
    do_pass(std::integral_constant<int, 1>{}, 3u, uniform_u64(e_mem[0]), uniform_u64(e_mem[1]), p, p < Lc_l, (upper ? e_coloff[1] : e_coloff[0]) + p,
            0u, ix, lane_rev, 0u, upper);
  }

  PH(6)
  ABLATE_AFTER(6)
  // ---- 7. consensus UMI per end (simple_umi.rs:46-117) ---------------------------------------------------------
  const DeviceTables* TU = P.TU;
  char my_rx[2] = {0, 0};      // lane i holds character i of each end's consensus UMI
  bool rx_bad = false;
#pragma unroll
  for (uint32_t k = 0; k < 2; k++) {
    if (k >= ne) break;
    const uint32_t rx_cnt = e_rx[k] & 0xFF, rx_ulen = (e_rx[k] >> 8) & 0xFF, rx_first = e_rx[k] >> 16;
    if (rx_cnt == 0) continue;                          // uniform
    const bool mychar = lane < rx_ulen;
    if (rx_cnt == 1) { if (mychar) my_rx[k] = (char)W[rlane(rx_lo, rx_first) + lane]; continue; }
    {
      const uint32_t f_lo = rlane(rx_lo, rx_first), ulen = rx_ulen;
      // whole 8-byte steps, then one step over the LAST 8 bytes (it may overlap): no masks; differences are OR-ed as integers
      unsigned long long diff = 0;
      if ((e_mem[k] & rxmask) >> lane & 1) {
        uint32_t i = 0;
        for (; i + 8 <= ulen; i += 8) diff |= ld64u(W, rx_lo + i) ^ ld64u(W, f_lo + i);
        if (i < ulen) {
          if (ulen >= 8) diff |= ld64u(W, rx_lo + ulen - 8) ^ ld64u(W, f_lo + ulen - 8);
          else diff |= (ld64u(W, rx_lo) ^ ld64u(W, f_lo)) & ((1ULL << (8 * ulen)) - 1ULL);
        }
      }
      if (!__any(diff != 0)) {
        if (mychar) {   // A C G T in either case → upper case; N / n → N; anything else as it stands
          const uint32_t ch = W[f_lo + lane], up = ch & 0xDFu, idx = up - 'A';
          const bool dna = idx < 26 && ((0x00082045u >> idx) & 1u);
          my_rx[k] = (char)(dna ? up : ch);
        }
        continue;
      }
    }
    ColumnAcc acc;
    acc.reset();
    uint32_t non_dna = 0, seenu = 0;
    uint8_t fc = 0;
    bool mixed = false;
    const double uc = TU->t.correct[20], ue = TU->t.error_per_alt[20];
    for (unsigned long long m = e_mem[k] & rxmask; m; m &= m - 1) {
      uint32_t r = (uint32_t)__builtin_ctzll(m);
      uint8_t ch = mychar ? W[rlane(rx_lo, r) + lane] : (uint8_t)'A';
      if (seenu == 0) fc = ch;
      seenu++;
      uint8_t up = (ch >= 'a' && ch <= 'z') ? (uint8_t)(ch - 32) : ch;
      bool dna = up == 'A' || up == 'C' || up == 'G' || up == 'T' || up == 'N';
      if (dna) { int bl = bam::ascii_to_lane(ch); if (bl != 255) acc.add(bl, uc, ue); }
      else { non_dna++; if (ch != fc) mixed = true; }
    }
    bool need_full = false;
    if (!mychar) { }
    else if (non_dna == 0) {
      int bi; uint8_t q;
      CallConst KU;
      KU.cap = TU->t.cap; KU.cap_threshold = TU->t.cap_threshold; KU.half_cerr_at_cap = TU->t.half_cerr_at_cap;
      bool resolved = column_call_fast_lds(TU->t, KU, acc.s, acc.obs, &bi, &q);
      my_rx[k] = bi >= 0 ? "ACGT"[bi] : 'N';
      need_full = !resolved;
    }
    else if (non_dna == seenu && !mixed) my_rx[k] = (char)fc;
    else rx_bad = true;
    if (!mychar) { need_full = false; rx_bad = false; }
    push_full(need_full, (1ull << 63) | ((uint64_t)(slot0 + e_type[k]) << 8) | lane, acc.s, acc.obs[0] | (acc.obs[1] << 8) | (acc.obs[2] << 16) | (acc.obs[3] << 24), 0u);
  }
  if (__any(rx_bad) || __any(list_overflow)) { if (lane == 0) { uint32_t kk = atomicAdd(P.n_deferred, 1u); P.deferred[kk] = g; } return; }
  // reserve room for this family's items (the result is looked at after phase 8's descriptors)
  uint32_t ires = 0;
  if (icnt && lane == 0) ires = atomicAdd(&P.full_count[my_list], icnt);

  PH(7)
  // ---- 8. descriptors + stats ---------------------------------------------------------------------------------------
#pragma unroll
  for (uint32_t k = 0; k < 2; k++) {
    if (k >= ne) break;
    uint32_t Lc = e_len[k];
    uint32_t slot = slot0 + e_type[k];
    EndDesc* D = &P.ends[slot];
    const uint32_t rx_cnt = e_rx[k] & 0xFF, rx_ulen = (e_rx[k] >> 8) & 0xFF;
    if (lane < rx_ulen && rx_cnt) D->rx[lane] = my_rx[k];
    uint32_t fk = (uint32_t)__builtin_ctzll(e_mem[k]);     // first retained read (cell barcode source)
    uint32_t fk_has_cb = (uint32_t)((cbmask >> fk) & 1), fk_cb_lo = rlane(cb_lo, fk), fk_cb_len = rlane(cb_len, fk), fk_lo = rlane(lo, fk);
    const unsigned long long off0 = (unsigned long long)rlane((uint32_t)off, 0) | ((unsigned long long)rlane((uint32_t)(off >> 32), 0) << 32);
    const unsigned long long off_fk = (unsigned long long)rlane((uint32_t)off, fk) | ((unsigned long long)rlane((uint32_t)(off >> 32), fk) << 32);
    if (lane == 0) {
      D->col_off = col_base + e_coloff[k];
      D->cons_len = Lc;
      D->first_off = off0; D->kept_off = off_fk;
      D->type = (uint8_t)e_type[k];
      D->mi_off = (uint16_t)(mi0_lo - lo); D->mi_len = (uint8_t)mi0_len;          // lane 0: lo = record 0
      bool hcb = P.cell0 && fk_has_cb;
      D->has_cb = hcb ? 1 : 0; D->cb_off = (uint16_t)(fk_cb_lo - fk_lo); D->cb_len = (uint8_t)fk_cb_len;
      D->has_rx = rx_cnt > 0; D->rx_len = (uint8_t)rx_ulen;
      uint32_t nm = P.prefix_len + 1 + mi0_len;
      uint32_t size = 32 + nm + 1 + (Lc + 1) / 2 + Lc + (3 + P.rg_len + 1) + 4 + 4 + 7 +
                      (P.per_base_tags ? 2 * (8 + 2 * Lc) : 0) + (3 + mi0_len + 1) + (hcb ? 3 + fk_cb_len + 1 : 0) +
                      (rx_cnt ? 3 + rx_ulen + 1 : 0);
      D->rec_size = size;
      D->valid = 1;
      P.rec_sizes[slot] = (uint64_t)size + 4;
    }
  }
  if (icnt) {   // the family's items: LDS -> the reserved range, 16 bytes per lane and step; a range that crosses the end of its list
                // continues in the next list (one more, synchronous, reservation — rare)
    wave_sync();
    uint32_t base = uni(ires), l = my_list, done = 0, tries = 0;
    bool overflow = false;
    for (;;) {
      const uint32_t rem = icnt - done;
      const uint32_t fit = base < P.full_cap ? (rem < P.full_cap - base ? rem : P.full_cap - base) : 0u;
      const uint4* src = (const uint4*)(W + ibase) + 3 * done;
      uint4* dst = (uint4*)(P.full_items + ((size_t)l * P.full_cap + base));
      for (uint32_t c = lane; c < 3 * fit; c += 64) dst[c] = src[c];
      done += fit;
      if (done == icnt) break;
      if (++tries >= N_LISTS) { overflow = true; break; }
      l = (l + 1) & (N_LISTS - 1);
      uint32_t b2 = 0;
      if (lane == 0) b2 = atomicAdd(&P.full_count[l], icnt - done);
      base = uni(b2);
    }
    if (overflow) {   // every list is full: the general path redoes the family (its descriptors are withdrawn, nothing was counted yet)
      if (lane < 3) { P.ends[slot0 + lane].valid = 0; P.rec_sizes[slot0 + lane] = 0; }
      if (lane == 0) { uint32_t kk = atomicAdd(P.n_deferred, 1u); P.deferred[kk] = g; }
      return;
    }
  }
  {   // per-lane counts are < 2^16 even summed over the wave (<= 32 pairs x 300 positions): two packed sums instead of four
    const uint32_t ba = wave_sum(ov_bases | (ov_agree << 16)), dc = wave_sum(ov_dis | (ov_corr << 16));
    ov_bases = ba & 0xFFFF; ov_agree = ba >> 16; ov_dis = dc & 0xFFFF; ov_corr = dc >> 16;
  }
  if (lane == 0) {
    const uint32_t s_insuf = rej & 0xFF, s_zero = (rej >> 8) & 0xFF, s_orphan = rej >> 16;
    atomicAdd(&st[0], (unsigned long long)n);
    if (ne) atomicAdd(&st[1], (unsigned long long)ne);
    if (rej) atomicAdd(&st[2], (unsigned long long)(s_insuf + s_zero + s_orphan));
    if (s_insuf) atomicAdd(&st[3 + FGX_REJ_INSUFFICIENT_READS], (unsigned long long)s_insuf);
    if (s_zero) atomicAdd(&st[3 + FGX_REJ_ZERO_LENGTH_AFTER_TRIMMING], (unsigned long long)s_zero);
    if (s_orphan) atomicAdd(&st[3 + FGX_REJ_ORPHAN_CONSENSUS], (unsigned long long)s_orphan);
    if (ov_bases) atomicAdd(&st[24], (unsigned long long)ov_bases);
    if (ov_agree) atomicAdd(&st[25], (unsigned long long)ov_agree);
    if (ov_dis) atomicAdd(&st[26], (unsigned long long)ov_dis);
    if (ov_corr) atomicAdd(&st[27], (unsigned long long)ov_corr);
  }
  PH(8)
}
