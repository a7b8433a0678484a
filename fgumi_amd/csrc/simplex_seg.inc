// simplex_seg.inc — k_simplex_seg<G>: G simplex families per wavefront (G = 2, 4; LPF = 64 / G lanes per family).
// Included by fastpath.hip inside `namespace fgx { namespace {` after simplex_wave2.inc (kahan2, unanimous_call_lds).
//
// Why: with one family per wavefront the record-per-lane phases (parse, aux walk, mate pairing, source-read geometry, gates,
// descriptors) run with n of 64 lanes busy — 16 of 64 at depth 8, 6 of 64 at depth 3 — and everything that is "one value per
// family" sits on the scalar unit, which the PMC passes show as loaded as the vector ALUs (profiles/r02b_pmc_1M.json:
// 4.5 k VALU + 4.5 k SALU wave-instructions per 16-read family).  Here a wavefront carries G families side by side:
//   * lane = sub * LPF + sl: family `sub`, record / column `sl`; each family owns one slice of the wave's LDS
//   * what was wave-uniform becomes FAMILY-uniform and lives in ordinary VGPRs (every lane of a family holds the same value);
//     ballots are cut to the family's lane range (`fbal`), broadcasts are ds_bpermute inside the family (`fbc`), reductions go
//     through a few LDS cells per family — so there is no per-family scalar loop anywhere
//   * mate pairing is an all-pairs rotation of a 32-bit name hash inside the family (verified byte-wise afterwards), the overlap
//     correction walks "pair j of every family" in lockstep with the family's lanes over the shared positions
//   * the column phase gives a family LPF columns per pass (150 columns = 5 passes of 32: 94 % of the lanes busy, 78 % with 64)
//     and reads each member read's descriptor from a compact per-family list in LDS; the column arithmetic is k_simplex_wave2's
//     two-chain Kahan loop (chains by order of appearance, bit-identical to the four-lane loop)
// A family that does not fit (more than LPF records, more bytes than its LDS slice) goes to the next launch (fewer, larger
// families per wavefront, finally k_simplex_wave2 = one per wavefront); one outside the record shape goes to k_family_wave<0>
// — per family, the other families of the wavefront carry on.
//
// Record shape and reference semantics: exactly those of k_simplex_wave2 (see simplex_wave2.inc), plus: UMIs that differ
// inside an end, unordered record offsets → the next kernel.

#ifndef FGX_SEG_OCC
#define FGX_SEG_OCC 3
#endif

template <int G>
__global__ __launch_bounds__(256, FGX_SEG_OCC) void k_simplex_seg(FastParams P, uint32_t n_grp_total) {
  constexpr uint32_t LPF = 64 / G;
  constexpr uint32_t FMASK = LPF >= 32 ? 0xFFFFFFFFu : ((1u << (LPF & 31)) - 1u);
  constexpr uint32_t RES = LPF * 8 + 64;                 // tail of a family's slice: member descriptor list (8 B each) + 16 cells
  FGX_DYN_LDS(dyn);
  __shared__ GateTables sT;
  __shared__ __align__(16) double sPair[256][2];
  __shared__ __align__(16) uint8_t sTagCls[256];
  {
    fill_tag_classes(sTagCls);
    load_gate_tables(sT, P.T->t);
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) { const uint32_t q = i < 93 ? i : 93; sPair[i][0] = P.T->t.correct[q]; sPair[i][1] = P.T->t.error_per_alt[q]; }
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t sub = lane / LPF, sl = lane % LPF, subbase = sub * LPF;
  const uint32_t lt = (1u << sl) - 1u;                   // family lanes below this one
  const uint32_t gi = (blockIdx.x * (blockDim.x >> 6) + wv) * G + sub;
  bool alive = gi < n_grp_total;                         // family-uniform; cleared when the family leaves this kernel
  if (!__any(alive)) return;
  const uint32_t g = alive ? (P.group_list ? P.group_list[gi] : P.g0 + gi) : 0u;
  const uint32_t SL = (P.lds_wave_bytes / G) & ~15u;     // bytes of one family's slice
  uint8_t* const W = dyn + (size_t)wv * P.lds_wave_bytes + (size_t)sub * SL;
  uint32_t* const cell = (uint32_t*)(W + SL - 64);
  uint8_t* const LST = W + SL - RES;

  // the family's part of a wave ballot, bit i = lane sl == i
  auto fbal = [&](bool p) -> uint32_t { return (uint32_t)(__ballot(p) >> subbase) & FMASK; };
  // value of lane `s` of this family (every lane of the wave must reach the call: ds_bpermute reads 0 from inactive lanes)
  auto fbc = [&](uint32_t v, uint32_t s) -> uint32_t { return (uint32_t)__builtin_amdgcn_ds_bpermute((int)((subbase + s) << 2), (int)v); };

  const uint32_t my_list = blockIdx.x & (N_LISTS - 1);
  bool list_overflow = false;
  auto push_full = [&](bool need, uint64_t dest, const double* ll, uint32_t obs_packed, uint32_t chains) {
    list_overflow |= push_full_global(P, lane, my_list, need, dest, ll, obs_packed, chains);
  };
  // the family leaves this kernel (conditions are family-uniform): record shape → k_family_wave<0>; size → next launch
  auto kill_old = [&](bool c) { if (alive && c) { if (sl == 0) { uint32_t k = atomicAdd(P.n_retry_old, 1u); P.retry_old[k] = g; } alive = false; } };
  auto kill_retry = [&](bool c) {
    if (alive && c) {
      if (sl == 0) { if (P.retry) { uint32_t k = atomicAdd(P.n_retry, 1u); P.retry[k] = g; } else { uint32_t k = atomicAdd(P.n_retry_old, 1u); P.retry_old[k] = g; } }
      alive = false;
    }
  };

  const uint32_t r0 = alive ? P.grp_first[g] : 0u, n = alive ? P.grp_first[g + 1] - r0 : 0u;
  const uint32_t slot0 = 3 * g;
  if (alive && sl < 3) { P.ends[slot0 + sl].valid = 0; P.rec_sizes[slot0 + sl] = 0; }
  // per-family counters (family-uniform), added to the batch totals at the end for the families this kernel finished
  uint32_t s_total = 0, s_cons = 0, s_filtered = 0, s_insuf = 0, s_zero = 0, s_orphan = 0;
  bool counted = false;
  if (alive && n < P.min_reads) { s_total = n; s_filtered = n; s_insuf = n; counted = true; alive = false; }   // simplex.rs:673-683
  kill_retry(n > LPF || (alive && n == 0));              // (an empty group has no byte span; the last kernel of the chain defers it)

  // ---- 1. stage each family's raw records into its LDS slice ------------------------------------------------------
  bool act = alive && sl < n;
  unsigned long long off = act ? P.rec_off[r0 + sl] : 0ull;
  uint32_t len = act ? P.rec_len[r0 + sl] : 0u;
  unsigned long long abs_off = 0;                        // the record's offset in the blob (descriptors)
  {
    const unsigned long long nxt = __shfl_down(off, 1);
    const bool disorder = act && sl + 1 < n && off + len > nxt;       // records are normally stored back to back in ascending order
    const uint32_t last = n ? n - 1 : 0;
    const unsigned long long end = off + len;
    const unsigned long long lo_off = (unsigned long long)fbc((uint32_t)off, 0) | ((unsigned long long)fbc((uint32_t)(off >> 32), 0) << 32);
    const unsigned long long hi_end = (unsigned long long)fbc((uint32_t)end, last) | ((unsigned long long)fbc((uint32_t)(end >> 32), last) << 32);
    kill_old(fbal(disorder || (act && len < 32)) != 0 || hi_end > P.blob_len);
    const unsigned long long base16 = lo_off & ~15ull;
    const unsigned long long span = hi_end - base16;
    kill_retry(span + 16 + RES > (unsigned long long)SL);
    if (alive) {
      const uint32_t span16 = ((uint32_t)span + 15) & ~15u;
      const uint8_t* src = P.blob + base16;
      for (uint32_t i = sl * 16; i < span16; i += LPF * 16) *(uint4*)(W + i) = *(const uint4*)(src + i);
    }
    abs_off = off;
    off -= base16;                                        // from here on: offset inside the slice
  }
  wave_sync();
  act = alive && sl < n;

  // ---- 2. parse: lane sl owns record sl of its family ----------------------------------------------------------------
  const uint32_t lo = act ? (uint32_t)off : 0u;
  uint32_t flags = 0, l_seq = 0, seq_lo = 0, qual_lo = 0, name_len = 0, clip = 0, hash = 0;
  int32_t pos = 0, ref_id = 0;
  uint32_t mi_lo = 0, mi_len = 0, rx_lo = 0, rx_len = 0, cb_lo = 0, cb_len = 0;
  bool has_mi = false, has_rx = false, has_cb = false, odd = false;
  if (act) {
    const record::FixedHeader H = record::decode_header(ld32u(W, lo), ld32u(W, lo + 4), ld32u(W, lo + 8), ld32u(W, lo + 12), ld32u(W, lo + 16));
    const record::Layout lay = record::layout(H, len);
    l_seq = H.l_seq; flags = H.flags;
    const bool unm = (flags & bam::F_UNMAPPED) != 0;          // an unmapped record: a read without a CIGAR — l_seq query bases, ref_id / pos unused
    if (lay.odd || record::streaming_header_odd(H, 1u, true, 0u)) odd = true;
    else {
      name_len = H.l_name - 1;
      ref_id = unm ? unmapped_ref_key(sl) : H.ref_id; pos = H.pos;
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
  const uint32_t mi0_lo = fbc(mi_lo, 0), mi0_len = fbc(mi_len, 0);
  if (act && sl == 0 && record::first_record_odd(has_mi, mi_len, P.prefix_len)) odd = true;
  if (act && !odd && W[qual_lo] == 0xFF) odd = true;                                  // absent qualities (:1119-1124): the first one decides here
  kill_old(fbal(odd) != 0);
  act = alive && sl < n;
  kill_old(mixed_unmapped_end(act, flags, fbal));         // drop_unmapped_if_any_mapped needs the final lengths: k_family_wave<0>'s
  act = alive && sl < n;
  const bool rev = (flags & bam::F_REVERSE) != 0;
  const uint32_t rxmask = fbal(act && has_rx), cbmask = fbal(act && has_cb);
  const uint32_t nmax = uni(wave_max(alive ? n : 0u));

  // ---- 3. overlapping-bases pre-correction in LDS (overlapping.rs:236-336, 627-684) ----------------------------------
  uint32_t ov_agree = 0, ov_dis = 0, ov_corr = 0;
  if (P.overlap) {
    // pair map: per name, the LAST R1-type and the LAST R2-type primary record; an R1 is paired unless a later R1 has its name.
    // All-pairs inside the family: step k compares lane sl with lane (sl + k) mod n by hash; names are verified afterwards.
    const uint32_t ty = !act ? 0u : (flags & bam::F_FIRST) ? 1u : (flags & bam::F_LAST) ? 2u : 0u;
    const uint32_t kh = (hash << 2) | ty;
    // (key ^ other key) is 0 for an R1 with this R1's hash and 3 for an R2 with it; selects and max only, no lane-mask branches
    int cmate = -1, clater = -1;
    for (uint32_t k = 1; k < nmax; k++) {
      const uint32_t up = sl + k;
      const bool wrap = up >= n, inrange = k < n;
      const uint32_t s = wrap ? up - n : up;
      const uint32_t d = fbc(kh, inrange ? s : sl) ^ kh;        // (past the family's size: its own key, d == 0)
      const int as_later = (d == 0 && !wrap && inrange) ? (int)s : -1;   // a later R1 of this name
      const int as_mate = d == 3 ? (int)s : -1;
      clater = as_later > clater ? as_later : clater;
      cmate = as_mate > cmate ? as_mate : cmate;
    }
    if (ty != 1) { cmate = -1; clater = -1; }
    int mate = -1;
    {
      const int other = clater >= 0 ? clater : cmate;
      const uint32_t osl = other >= 0 ? (uint32_t)other : sl;
      const uint32_t lou = fbc(lo, osl), nlo = fbc(name_len, osl);
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
      kill_old(fbal(collide) != 0);
      act = alive && sl < n;
      if (!alive) mate = -1;
    }
    // shared reference span of each pair, owned by its R1 lane
    const uint32_t msrc = mate >= 0 ? (uint32_t)mate : sl;
    const int32_t pos_b = (int32_t)fbc((uint32_t)pos, msrc), ref_b = (int32_t)fbc((uint32_t)ref_id, msrc);
    const uint32_t len_b = fbc(l_seq, msrc);
    const uint32_t dsc_a = seq_lo | (qual_lo << 16), dsc_b = fbc(dsc_a, msrc);
    uint32_t cntp = 0, off12 = 0;
    if (mate >= 0 && ref_id == ref_b) {
      const int32_t s1 = pos + 1, e1 = pos + (int32_t)l_seq, s2 = pos_b + 1, e2 = pos_b + (int32_t)len_b;
      const int32_t lox = s1 > s2 ? s1 : s2, hix = e1 < e2 ? e1 : e2;
      if (hix >= lox) { cntp = (uint32_t)(hix - lox + 1); off12 = (uint32_t)(lox - s1) | ((uint32_t)(lox - s2) << 16); }
    }
    const uint32_t om = fbal(cntp != 0);
    const uint32_t npairs = (uint32_t)__popc(om);
    if (cntp != 0) LST[__popc(om & lt)] = (uint8_t)sl;      // pair j of the family → its R1 lane
    wave_sync();
    const uint32_t maxpairs = uni(wave_max(npairs));
    for (uint32_t j = 0; j < maxpairs; j++) {
      const bool has = j < npairs;
      const uint32_t osl = has ? (uint32_t)LST[j] : sl;
      const uint32_t da = fbc(dsc_a, osl), db = fbc(dsc_b, osl), oo = fbc(off12, osl);
      const uint32_t cn_o = fbc(cntp, osl);
      const uint32_t cn = has ? cn_o : 0u;
      const uint32_t sa = da & 0xFFFF, qa0 = da >> 16, sb = db & 0xFFFF, qb0 = db >> 16;
      // lane addresses advance by whole steps (LPF positions, an even count): nibble parities are fixed per pair
      const uint32_t i1 = (oo & 0xFFFF) + sl, i2 = (oo >> 16) + sl;
      uint32_t o1 = sa + (i1 >> 1), o2 = sb + (i2 >> 1), q1 = qa0 + i1, q2 = qb0 + i2;
      const uint32_t sh1 = (~i1 & 1) << 2, sh2 = (~i2 & 1) << 2;
      for (uint32_t w = sl; w < cn; w += LPF, o1 += LPF / 2, o2 += LPF / 2, q1 += LPF, q2 += LPF) {
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
  }
  wave_sync();

  // ---- 4. source-read length per lane (vanilla_caller.rs:1129-1160; no --trim in this shape) --------------------------
  const uint32_t min_bq = P.min_input_bq;
  auto view = [&](uint32_t s_lo, uint32_t q_lo, uint32_t L, bool rv, uint32_t p, uint32_t* code, uint32_t* qual) {
    const uint32_t idx = rv ? L - 1 - p : p;
    const uint32_t bb = W[s_lo + (idx >> 1)];
    uint32_t c = (bb >> ((~idx & 1) << 2)) & 15;
    uint32_t q = W[q_lo + idx];
    if (rv) c = __builtin_bitreverse32(c) >> 28;
    if (q < min_bq) { c = 15; q = FGX_MIN_PHRED; }      // p < trim_to == L always
    *code = c; *qual = q;
  };
  uint32_t final_len = 0;
  {
    const uint32_t fl = l_seq > clip ? l_seq - clip : 0;
    bool tail_n = false;
    if (act && fl > 0) { uint32_t c, q; view(seq_lo, qual_lo, l_seq, rev, fl - 1, &c, &q); tail_n = (c == 15); }
    final_len = act ? fl : 0;
    // reads ending in N / masked bases: the family's lanes strip the run LPF positions at a time, read after read
    uint32_t tm = fbal(tail_n);
    while (__any(tm != 0)) {
      const bool work = tm != 0;
      const uint32_t r = work ? (uint32_t)__builtin_ctz(tm) : sl;
      tm &= tm - 1;
      uint32_t flr = fbc(final_len, r);
      const uint32_t s_r = fbc(seq_lo, r), q_r = fbc(qual_lo, r), L_r = fbc(l_seq, r);
      const bool rv_r = (fbc(flags, r) & bam::F_REVERSE) != 0;
      bool scanning = work;
      while (__any(scanning && flr > 0)) {
        bool real = false;
        if (scanning && sl < flr) { uint32_t c, q; view(s_r, q_r, L_r, rv_r, flr - 1 - sl, &c, &q); real = (c != 15); }
        const uint32_t bm = fbal(real);
        if (scanning) {
          if (bm) { flr -= (uint32_t)__builtin_ctz(bm); scanning = false; }
          else { flr -= flr < LPF ? flr : LPF; if (flr == 0) scanning = false; }
        }
      }
      if (work && sl == r) final_len = flr;
    }
  }

  // ---- 5. family gates (process_group :1329-1422, process_subgroup :1454-1646) ------------------------------------------
  if (alive) s_total = n;
  uint32_t my_end = 255;
  if (act) { if (!(flags & bam::F_PAIRED)) my_end = 0; else if (flags & bam::F_FIRST) my_end = 1; else my_end = 2; }
  if (sl < 4) cell[sl] = 0;
  wave_sync();
  bool ok[3] = {false, false, false};
  uint32_t mem[3] = {0, 0, 0}, surv[3] = {0, 0, 0};
  bool bites = false;
#pragma unroll
  for (uint32_t e = 0; e < 3; e++) {
    const uint32_t in_e = fbal(my_end == e);
    const uint32_t cnt = (uint32_t)__popc(in_e);
    const uint32_t kept = fbal(my_end == e && final_len > 0);
    const uint32_t rem = (uint32_t)__popc(kept), zero = cnt - rem;
    if (!alive || cnt == 0) continue;
    if (cnt < P.min_reads) { s_filtered += cnt; s_insuf += cnt; continue; }
    if (zero) { s_filtered += zero; s_zero += zero; }
    if (rem < P.min_reads) { if (rem) { s_filtered += rem; s_insuf += rem; } continue; }
    if (P.max_reads >= 0 && (long long)rem > P.max_reads) { bites = true; continue; }   // downsampling: k_family_wave<0>
    mem[e] = kept; surv[e] = rem; ok[e] = true;
  }
  kill_old(bites);
  act = alive && sl < n;
  {
    // consensus length = min_reads-th longest kept read of the end: every kept read counts the kept reads of its end that
    // are at least as long (itself included), the longest read with min_reads of them wins
    const uint32_t mymem = my_end == 0 ? mem[0] : my_end == 1 ? mem[1] : my_end == 2 ? mem[2] : 0u;
    const bool mine = act && ((mymem >> sl) & 1);
    uint32_t ge = 1;
    if (P.min_reads > 1) {
      const uint32_t v = final_len | (my_end << 16) | ((mine ? 1u : 0u) << 18);
      for (uint32_t k = 1; k < nmax; k++) {
        uint32_t s = sl + k;
        if (s >= n) s -= n;
        const bool inrange = act && k < n;
        const uint32_t ov = fbc(v, inrange ? s : sl);
        if (inrange && ((ov >> 18) & 1) && ((ov >> 16) & 3) == my_end && (ov & 0xFFFF) >= final_len) ge++;
      }
    }
    if (mine && ge >= P.min_reads) atomicMax(&cell[my_end], final_len);
  }
  wave_sync();
  const uint32_t clen0 = cell[0], clen1 = cell[1], clen2 = cell[2];
  uint32_t e_type[3], e_len[3], e_coloff[3], e_mem[3];
  const bool has_frag = ok[0], has_pair = ok[1] && ok[2];
  const uint32_t ne = alive ? (has_frag ? 1u : 0u) + (has_pair ? 2u : 0u) : 0u;
  e_type[0] = has_frag ? 0u : 1u; e_len[0] = has_frag ? clen0 : clen1; e_mem[0] = has_frag ? mem[0] : mem[1];
  e_type[1] = has_frag ? 1u : 2u; e_len[1] = has_frag ? clen1 : clen2; e_mem[1] = has_frag ? mem[1] : mem[2];
  e_type[2] = 2u; e_len[2] = clen2; e_mem[2] = mem[2];
  if (alive) {
    if (has_frag) s_cons += 1;
    if (has_pair) s_cons += 2;
    else if (ok[1]) { s_filtered += surv[1]; s_orphan += surv[1]; }
    else if (ok[2]) { s_filtered += surv[2]; s_orphan += surv[2]; }
  }
  uint32_t total_cols = 0;
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) { e_coloff[k] = total_cols; if (k < ne) total_cols += e_len[k]; }

  // UMIs of the kept reads of each end: this kernel takes ends whose UMIs are byte-identical (the usual case: n >= 2 agreeing
  // observations leave the base the strict maximum, so the consensus is the upper-cased string; N/n stays 'N'; a non-DNA
  // character shared by every string is kept — simple_umi.rs:69-103); differing UMIs → per-character columns in k_simplex_wave2
  uint32_t e_rx_cnt[3] = {0, 0, 0}, e_rx_len[3] = {0, 0, 0}, e_rx_first[3] = {0, 0, 0};
  {
    bool rx_odd = false;
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
      const uint32_t with = k < ne ? e_mem[k] & rxmask : 0u;
      const uint32_t cnt = (uint32_t)__popc(with);
      const uint32_t f = cnt ? (uint32_t)__builtin_ctz(with) : sl;
      const uint32_t f_lo = fbc(rx_lo, f), f_len = fbc(rx_len, f);
      e_rx_cnt[k] = cnt; e_rx_first[k] = f; e_rx_len[k] = cnt ? f_len : 0u;
      bool differs = false;
      if ((with >> sl) & 1) {
        if (rx_len != f_len) differs = true;
        else
          for (uint32_t i = 0; i < f_len; i += 8) {
            unsigned long long a = ld64u(W, rx_lo + i), b = ld64u(W, f_lo + i);
            if (i + 8 > f_len) { unsigned long long mk = (1ULL << (8 * (f_len - i))) - 1; a &= mk; b &= mk; }
            differs |= a != b;
          }
      }
      if (fbal(differs) != 0 || (cnt && f_len > FAST_RX_CAP)) rx_odd = true;
    }
    kill_retry(rx_odd);                                  // (the last launch of the chain is k_simplex_wave2)
    act = alive && sl < n;
  }
  const uint32_t ne_f = alive ? ne : 0u;

  // member descriptor list of the family, end after end in output order, file order inside an end:
  // d0 = seq_lo | rev << 15 | qual_lo << 16 ; d1 = l_seq | final_len << 16
  uint32_t moff[3], mcnt[3];
  {
    uint32_t run = 0;
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
      const uint32_t mk = k < ne_f ? e_mem[k] : 0u;
      moff[k] = run; mcnt[k] = (uint32_t)__popc(mk);
      if ((mk >> sl) & 1) {
        uint2 d;
        d.x = seq_lo | ((rev ? 1u : 0u) << 15) | (qual_lo << 16); d.y = l_seq | (final_len << 16);
        *(uint2*)(LST + 8 * (run + (uint32_t)__popc(mk & lt))) = d;
      }
      run += mcnt[k];
    }
  }
  wave_sync();

  // ---- 6. consensus columns: LPF columns of a family per pass, member reads in file order --------------------------------
  const DeviceTables* T = P.T;
  const uint64_t col_base = alive ? P.col_base[g] : 0ull;
  CallConst KC;
  KC.cap = (uint32_t)__builtin_amdgcn_readfirstlane((int)sT.cap);
  KC.cap_threshold = uniform_f64(sT.cap_threshold); KC.half_cerr_at_cap = uniform_f64(sT.half_cerr_at_cap);
  const uint8_t* const pairs = (const uint8_t*)&sPair[0][0];
  const uint32_t maxne = uni(wave_max(ne_f));
#pragma unroll 1
  for (uint32_t k = 0; k < maxne; k++) {
    const bool hk = k < ne_f;
    const uint32_t Lc = !hk ? 0u : k == 0 ? e_len[0] : k == 1 ? e_len[1] : e_len[2];
    const uint32_t coff = k == 0 ? e_coloff[0] : k == 1 ? e_coloff[1] : e_coloff[2];
    const uint32_t mc = !hk ? 0u : k == 0 ? mcnt[0] : k == 1 ? mcnt[1] : mcnt[2];
    const uint32_t mo = k == 0 ? moff[0] : k == 1 ? moff[1] : moff[2];
    const uint32_t maxL = uni(wave_max(Lc)), maxmc = uni(wave_max(mc));
    for (uint32_t p0 = 0; p0 < maxL; p0 += LPF) {
      const uint32_t p = p0 + sl;
      double s2, c2, s3, c3;                                 // chains 2 / 3: written when opened; until then any value will do
      FGX_UNDEF4(s2, c2, s3, c3);
      const bool incol = p < Lc;
      const uint64_t o = col_base + coff + p;
      if (incol && mc == 1) {   // single-read consensus: LUT keyed by the unclamped quality (:1677-1708)
        const uint2 d = *(const uint2*)(LST + 8 * mo);
        uint32_t code, q;
        view(d.x & 0x7FFF, d.x >> 16, d.y & 0xFFFF, (d.x >> 15) & 1, p, &code, &q);
        const uint8_t adj = q < 94 ? T->single_input_quals[q] : 0;
        uint8_t ob, oq;
        if (adj < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; } else { ob = (uint8_t)code; oq = adj; }
        P.col_code[o] = ob; P.col_qual[o] = oq; P.col_depth[o] = (uint16_t)(code != 15 ? 1 : 0); P.col_err[o] = 0;
      }
      const bool multi_read = incol && mc > 1;
      // Kahan chains by order of appearance (see k_simplex_wave2): chain 1 = first base seen, 2 / 3 = second / third distinct
      // base, R = every base not seen yet.
      double s1 = 0.0, c1 = 0.0, sR = 0.0, cR = 0.0;
      uint32_t allow = 0x116u;                              // codes the hot path still takes (see k_simplex_wave2): A C G T | 1 << code | 0
      uint32_t b1 = 0, b2 = 0, b3 = 0, n1 = 0, n2 = 0, n3 = 0, nR = 0;
      for (uint32_t j0 = 0; j0 < maxmc; j0 += FGX_V2_BATCH) {
        uint32_t q_[FGX_V2_BATCH], c_[FGX_V2_BATCH];
        bool in_[FGX_V2_BATCH];
#pragma unroll
        for (int j = 0; j < FGX_V2_BATCH; j++) {
          const bool on = multi_read && j0 + j < mc;
          const uint2 d = *(const uint2*)(LST + 8 * (on ? mo + j0 + j : 0u));
          const bool rv = (d.x >> 15) & 1;
          const uint32_t slo = d.x & 0x7FFF, qlo = d.x >> 16, Lr = d.y & 0xFFFF;
          in_[j] = on && p < (d.y >> 16);                    // inside the read's final length
          const uint32_t ix = rv ? Lr - 1 - p : p;           // (past the read: masked by in_, the LDS read is harmless)
          q_[j] = W[qlo + ix];
          uint32_t c = ((uint32_t)W[slo + (ix >> 1)] >> ((~ix & 1) << 2)) & 15;
          if (rv) c = __builtin_bitreverse32(c) >> 28;       // complement = bit reversal of the code
          c_[j] = c;
        }
        double2 pr_[FGX_V2_BATCH];
#pragma unroll
        for (int j = 0; j < FGX_V2_BATCH; j++) pr_[j] = *(const double2*)(pairs + (q_[j] << 4));
#pragma unroll
        for (int j = 0; j < FGX_V2_BATCH; j++) {
          const uint32_t q = q_[j], c = c_[j];
          const bool qok = in_[j] && q >= min_bq;
          const bool bit = __builtin_amdgcn_ubfe(allow, c, 1u) != 0;
          if (qok && bit) {                                   // nothing seen yet, or this very base only
            allow = 1u << c; n1++;
            kahan2(s1, c1, pr_[j].x); kahan2(sR, cR, pr_[j].y);
          }
          if (qok && !bit) {
            uint32_t cc = c;
            FGX_PIN("+v"(cc));                      // (the one-hot test stays in this block)
            if (__popc(cc) == 1) {
              if (allow != 0) { b1 = (uint32_t)__builtin_ctz(allow); allow = 0; }
              if (c != b1 && c != b2 && c != b3) {
                if (b2 == 0) { b2 = c; s2 = sR; c2 = cR; }
                else if (b3 == 0) { b3 = c; s3 = sR; c3 = cR; }
              }
              const bool h1 = c == b1, h2 = c == b2, h3 = c == b3;
              kahan2(s1, c1, h1 ? pr_[j].x : pr_[j].y);
              kahan2(s2, c2, h2 ? pr_[j].x : pr_[j].y);
              kahan2(s3, c3, h3 ? pr_[j].x : pr_[j].y);
              kahan2(sR, cR, (h1 || h2 || h3) ? pr_[j].y : pr_[j].x);
              n1 += h1; n2 += h2; n3 += h3; nR += !(h1 || h2 || h3);
            }
          }
        }
      }
      if (allow != 0) b1 = (uint32_t)__builtin_ctz(allow);  // one base only (nothing seen: nobody reads it)
      // ---- call ----
      bool need_full = false;
      uint32_t depth = 0, q_call = FGX_MIN_PHRED, code_call = 15, err = 0;
      bool resolved = true;
      if (multi_read) {
        depth = n1 + n2 + n3 + nR;
        if (b2 != 0) resolved = false;
        else if (n1 != 0) {
          uint32_t qq = 0;
          resolved = unanimous_call_lds(sT, P.T->t.cerr_min, KC, s1, sR, &qq);
          if (resolved) { q_call = qq; code_call = b1; err = 0; }
        }
        need_full = !resolved;
        P.col_depth[o] = (uint16_t)(depth < 32767u ? depth : 32767u);
      }
      {   // the chains as they stand; k_call_full sorts them into A, C, G, T
        const double chain[4] = {s1, s2, s3, sR};
        push_full(need_full, o, chain, n1 | (n2 << 8) | (n3 << 16) | (nR << 24), b1 | (b2 << 4) | (b3 << 8));
      }
      if (multi_read && resolved) {
        uint8_t ob, oq;
        if (depth < P.min_reads) { ob = 15; oq = 0; }
        else if (q_call < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; }
        else { ob = (uint8_t)code_call; oq = (uint8_t)q_call; }
        P.col_code[o] = ob; P.col_qual[o] = oq; P.col_err[o] = (uint16_t)err;
      }
    }
  }
  // a full call_full pool: the family is redone by the general path (its scratch columns are private, stale items are harmless)
  {
    const bool ovf = fbal(list_overflow) != 0;
    if (alive && ovf) { if (sl == 0) { uint32_t kk = atomicAdd(P.n_deferred, 1u); P.deferred[kk] = g; } alive = false; }
  }

  // ---- 7. + 8. consensus UMI (identical strings), descriptors, stats -----------------------------------------------------
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    const bool hk = alive && k < ne;
    const uint32_t slot = slot0 + e_type[k];
    EndDesc* D = &P.ends[slot];
    const uint32_t ulen = hk ? e_rx_len[k] : 0u;
    const uint32_t f_lo = fbc(rx_lo, e_rx_first[k]);
    for (uint32_t i = sl; i < ulen; i += LPF) {
      // several identical UMIs: A C G T in either case → upper case, N / n → N, anything else as it stands
      const uint32_t ch = W[f_lo + i], up = ch & 0xDFu, idx = up - 'A';
      const bool dna = e_rx_cnt[k] != 1 && idx < 26 && ((0x00082045u >> idx) & 1u);
      D->rx[i] = (char)(dna ? up : ch);
    }
    const uint32_t fk = hk ? (uint32_t)__builtin_ctz(e_mem[k]) : sl;     // first retained read (cell barcode source)
    const uint32_t fk_cb_lo = fbc(cb_lo, fk), fk_cb_len = fbc(cb_len, fk), fk_lo = fbc(lo, fk);
    const unsigned long long off_fk = (unsigned long long)fbc((uint32_t)abs_off, fk) | ((unsigned long long)fbc((uint32_t)(abs_off >> 32), fk) << 32);
    if (hk && sl == 0) {
      const uint32_t Lc = e_len[k];
      const uint32_t fk_has_cb = (cbmask >> fk) & 1;
      D->col_off = col_base + e_coloff[k];
      D->cons_len = Lc;
      D->first_off = abs_off; D->kept_off = off_fk;                               // sl == 0: this lane's record is record 0
      D->type = (uint8_t)e_type[k];
      D->mi_off = (uint16_t)(mi0_lo - lo); D->mi_len = (uint8_t)mi0_len;          // sl == 0: lo = record 0
      const bool hcb = P.cell0 && fk_has_cb;
      D->has_cb = hcb ? 1 : 0; D->cb_off = (uint16_t)(fk_cb_lo - fk_lo); D->cb_len = (uint8_t)fk_cb_len;
      D->has_rx = e_rx_cnt[k] > 0; D->rx_len = (uint8_t)e_rx_len[k];
      const uint32_t nm = P.prefix_len + 1 + mi0_len;
      const uint32_t size = 32 + nm + 1 + (Lc + 1) / 2 + Lc + (3 + P.rg_len + 1) + 4 + 4 + 7 +
                            (P.per_base_tags ? 2 * (8 + 2 * Lc) : 0) + (3 + mi0_len + 1) + (hcb ? 3 + fk_cb_len + 1 : 0) +
                            (e_rx_cnt[k] ? 3 + e_rx_len[k] + 1 : 0);
      D->rec_size = size;
      D->valid = 1;
      P.rec_sizes[slot] = (uint64_t)size + 4;
    }
  }
  if (alive) counted = true;
  {
    // batch totals: the family-uniform counters of every finished family once (its lane 0), the overlap tallies of its lanes
    const bool lead = counted && sl == 0;
    // three packed sums: a wave holds at most 64 records (8-bit fields) and at most 64 x 300 overlap positions (16-bit fields)
    const uint32_t w1 = wave_sum(lead ? (s_total | (s_cons << 8) | (s_filtered << 16) | (s_insuf << 24)) : 0u);
    const uint32_t w2 = wave_sum((lead ? (s_zero | (s_orphan << 8)) : 0u) | (counted ? (ov_agree << 16) : 0u));
    const uint32_t w3 = wave_sum(counted ? (ov_dis | (ov_corr << 16)) : 0u);
    const uint32_t t_total = w1 & 0xFF, t_cons = (w1 >> 8) & 0xFF, t_filt = (w1 >> 16) & 0xFF, t_insuf = w1 >> 24;
    const uint32_t t_zero = w2 & 0xFF, t_orph = (w2 >> 8) & 0xFF, t_oa = w2 >> 16;
    const uint32_t t_od = w3 & 0xFFFF, t_oc = w3 >> 16, t_ob = t_oa + t_od;
    if (lane == 0) {
      unsigned long long* st = P.stats + (size_t)(blockIdx.x & (STAT_SLOTS - 1)) * 32;
      if (t_total) atomicAdd(&st[0], (unsigned long long)t_total);
      if (t_cons) atomicAdd(&st[1], (unsigned long long)t_cons);
      if (t_filt) atomicAdd(&st[2], (unsigned long long)t_filt);
      if (t_insuf) atomicAdd(&st[3 + FGX_REJ_INSUFFICIENT_READS], (unsigned long long)t_insuf);
      if (t_zero) atomicAdd(&st[3 + FGX_REJ_ZERO_LENGTH_AFTER_TRIMMING], (unsigned long long)t_zero);
      if (t_orph) atomicAdd(&st[3 + FGX_REJ_ORPHAN_CONSENSUS], (unsigned long long)t_orph);
      if (t_ob) atomicAdd(&st[24], (unsigned long long)t_ob);
      if (t_oa) atomicAdd(&st[25], (unsigned long long)t_oa);
      if (t_od) atomicAdd(&st[26], (unsigned long long)t_od);
      if (t_oc) atomicAdd(&st[27], (unsigned long long)t_oc);
    }
  }
}
