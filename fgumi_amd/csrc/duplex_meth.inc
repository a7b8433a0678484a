// duplex_meth.inc — the methylation tags of a duplex consensus record in the device-resident pipeline (methylation-aware mode: EM-Seq / TAPs).
// Included by fastpath.hip inside `namespace fgx { namespace {` after simplex_deep.inc (meth_chunk_skip, meth_digits) and the duplex record writers
// (duplex_call).
//
// What comes before: k_family_wave<1, 1> left, per scratch column of each of the molecule's four read sets, "the reference shows a cytosine of the
// call's strand" and the unconverted / converted counts (FastParams::meth_flag / meth_u / meth_t), called the NORMALISED reads, and said in
// DuplexDesc::meth which strands of a record carry an annotation; k_call_full has made the single-strand bases final.
//
// What is written behind RX, in the reference's order (duplex_read_into, duplex_caller.rs:1338-1398):
//   the AB-side strand, when annotated:  am (its MM string, no ML)  au  at      — bm bu bt and the G-m strand when the record is a BA strand alone (is_ba_only)
//   the BA-side strand, when annotated:  bm bu bt                               — two-strand records only
//   the combined annotation:            MM ML cu ct                              — combine_methylation_annotations (methylation.rs:404-427): flags OR-ed, counts
//                                                                                  added, over the duplex length; one strand's alone when the other has none
// and nothing at all when no strand of the record is annotated.  An MM string (build_mm_ml_tags, methylation.rs:264-343) lists, for every base of the
// sequence that is the strand's cytosine (C on C+m, G on G-m) and has evidence (reference cytosine, unconverted + converted > 0), how many such bases
// without evidence were skipped since the previous entry; a string without an entry is not written (its count arrays still are).  The duplex MM is
// built from the duplex bases: duplex_call, the same function the record writers call.
//
// Two kernels in the shape of k_meth_sizes / k_meth_tail (simplex_deep.inc), a wavefront per record, 64 columns per step: k_duplex_meth_sizes after
// k_call_full and before the scan of the record sizes (the strings depend on final bases), k_duplex_meth_tail after the record writers.

// one column of one of the record's three annotated sequences: 0 the AB-side strand, 1 the BA-side strand, 2 the duplex read
struct DMethCol { uint32_t code, flag, u, t; };
__device__ __forceinline__ DMethCol duplex_meth_col(const FastParams& P, uint64_t a_off, uint64_t b_off, bool has_ba, uint32_t which, uint32_t i) {
  DMethCol c;
  if (which == 0 || !has_ba) { const uint64_t o = a_off + i; c.code = P.col_code[o]; c.flag = P.meth_flag[o]; c.u = P.meth_u[o]; c.t = P.meth_t[o]; return c; }
  if (which == 1) { const uint64_t o = b_off + i; c.code = P.col_code[o]; c.flag = P.meth_flag[o]; c.u = P.meth_u[o]; c.t = P.meth_t[o]; return c; }
  const uint64_t oa = a_off + i, ob = b_off + i;
  const uint32_t ca = P.col_code[oa], cb = P.col_code[ob], qa = P.col_qual[oa], qb = P.col_qual[ob];
  c.flag = (uint32_t)(P.meth_flag[oa] | P.meth_flag[ob]);            // (a strand without an annotation has no flag set and no count)
  c.u = (uint32_t)P.meth_u[oa] + P.meth_u[ob]; c.t = (uint32_t)P.meth_t[oa] + P.meth_t[ob];   // (at most 64 reads per strand: no saturation to apply)
  c.code = duplex_call<1>(ca, qa, cb, qb, c.flag != 0).oc;
  return c;
}
// which sequences of a record carry tags: bit 0 the AB-side strand, bit 1 the BA-side strand, bit 2 the combined annotation
__device__ __forceinline__ uint32_t duplex_meth_parts(const DuplexDesc& D) {
  const uint32_t m = D.meth;
  if (!D.has_ba) return (m & 1u) ? 5u : 0u;
  return (m & 3u) ? ((m & 3u) | 4u) : 0u;
}

__global__ __launch_bounds__(256) void k_duplex_meth_sizes(FastParams P, uint32_t n_slots, DuplexMethSlot* __restrict__ ms) {
  const uint32_t slot = uni((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (slot >= n_slots) return;
  DuplexMethSlot r;
  r.std_size = 0; r._pad = 0;
  for (int w = 0; w < 3; w++) { r.n_hit[w] = 0; r.mm_len[w] = 0; }
  if (P.rec_sizes[slot] != 0) {
    DuplexDesc* const D = &P.dends[slot];
    r.std_size = uni(D->rec_size);
    const uint32_t parts = uni(D->valid) ? uni(duplex_meth_parts(*D)) : 0u;
    if (parts) {
      const uint32_t n = uni(D->len);
      const bool has_ba = uni(D->has_ba) != 0, ba_only = (uni(D->meth) & 4u) != 0;
      const uint64_t a_off = uniform_u64(D->a_off), b_off = uniform_u64(D->b_off);
      uint32_t extra = 0;
      for (uint32_t w = 0; w < 3; w++) {
        if (!((parts >> w) & 1u)) continue;
        const uint32_t track = (w == 1 || ba_only) ? 4u : 2u;                  // G on the G-m strand, C on C+m
        uint32_t carry = 0, mm = 0, hits = 0;
        for (uint32_t i0 = 0; i0 < n; i0 += 64) {
          const uint32_t i = i0 + lane;
          const bool in = i < n;
          const DMethCol c = duplex_meth_col(P, a_off, b_off, has_ba, w, in ? i : 0u);
          const bool tracked = in && c.code == track;
          const bool hit = tracked && c.flag && (c.u + c.t) > 0;
          unsigned long long mh;
          const uint32_t skip = meth_chunk_skip(lane, tracked, hit, carry, mh);
          hits += (uint32_t)__popcll(mh);
          mm += hit ? 1u + meth_digits(skip) : 0u;
        }
        r.n_hit[w] = hits; r.mm_len[w] = uni(wave_sum(mm));
        extra += 2u * (8u + 2u * n);                                             // the count arrays: B:s
        if (hits) extra += 3u + 3u + r.mm_len[w] + 1u + 1u;                      // am / bm / MM :Z: <C+m|G-m> entries ; NUL
        if (hits && w == 2) extra += 8u + hits;                                  // ML:B:C
      }
      if (lane == 0) { D->rec_size = r.std_size + extra; P.rec_sizes[slot] = (uint64_t)(r.std_size + extra) + 4; }
    }
  }
  if (lane == 0) ms[slot] = r;
}

__global__ __launch_bounds__(256) void k_duplex_meth_tail(FastParams P, uint32_t n_slots, const DuplexMethSlot* __restrict__ ms, const uint64_t* __restrict__ out_off, uint8_t* __restrict__ out) {
  const uint32_t slot = uni((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (slot >= n_slots || P.rec_sizes[slot] == 0) return;
  const DuplexDesc& D = P.dends[slot];
  const uint32_t parts = uni(D.valid) ? uni(duplex_meth_parts(D)) : 0u;
  if (!parts) return;
  const uint32_t n = uni(D.len);
  const bool has_ba = uni(D.has_ba) != 0, ba_only = (uni(D.meth) & 4u) != 0;
  const uint64_t a_off = uniform_u64(D.a_off), b_off = uniform_u64(D.b_off);
  uint8_t* q = out + uniform_u64(out_off[slot]) + 4 + uni(ms[slot].std_size);
  for (uint32_t w = 0; w < 3; w++) {
    if (!((parts >> w) & 1u)) continue;
    const bool top = !(w == 1 || ba_only);
    const uint32_t track = top ? 2u : 4u;
    const uint32_t n_hit = uni(ms[slot].n_hit[w]), mm_len = uni(ms[slot].mm_len[w]);
    // tag names: the AB-side strand a*, the BA side (and a BA strand alone) b*, the combined annotation MM / ML / cu / ct
    const uint8_t s0 = w == 2 ? (uint8_t)'c' : (w == 1 || ba_only) ? (uint8_t)'b' : (uint8_t)'a';
    if (n_hit) {
      uint8_t* const mmq = q + 6;                                                // the entries
      uint8_t* const ml = q + 3 + 3 + mm_len + 2;                                // behind the string's ";" and NUL: ML (the combined annotation only)
      const uint8_t t0 = w == 2 ? (uint8_t)'M' : s0, t1 = w == 2 ? (uint8_t)'M' : (uint8_t)'m';
      if (lane < 6) q[lane] = lane == 0 ? t0 : lane == 1 ? t1 : lane == 2 ? (uint8_t)'Z' : lane == 3 ? (uint8_t)(top ? 'C' : 'G') : lane == 4 ? (uint8_t)(top ? '+' : '-') : (uint8_t)'m';
      if (w == 2 && lane < 8) ml[lane] = lane == 0 ? 'M' : lane == 1 ? 'L' : lane == 2 ? 'B' : lane == 3 ? 'C' : (uint8_t)(n_hit >> (8 * (lane - 4)));
      uint32_t carry = 0, ml_base = 0, mm_base = 0;
      for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        const bool in = i < n;
        const DMethCol c = duplex_meth_col(P, a_off, b_off, has_ba, w, in ? i : 0u);
        const bool tracked = in && c.code == track;
        const bool hit = tracked && c.flag && (c.u + c.t) > 0;
        unsigned long long mh;
        const uint32_t skip = meth_chunk_skip(lane, tracked, hit, carry, mh);
        const uint32_t nd = meth_digits(skip), mine = hit ? 1u + nd : 0u;
        uint32_t incl = mine;                                                     // inclusive prefix sum of the entries' lengths over the wavefront
        for (int o = 1; o < 64; o <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)incl, o); if ((int)lane >= o) incl += v; }
        if (hit) {
          if (w == 2) {
            const uint32_t total = c.u + c.t, num = P.meth_mode == FGX_METHYLATION_EM_SEQ ? c.u : c.t;     // EM-Seq: unconverted / total; TAPs: converted / total
            const uint32_t pr = num * 255u / total;
            ml[8 + ml_base + (uint32_t)__popcll(mh & ((1ull << lane) - 1ull))] = (uint8_t)(pr > 255u ? 255u : pr);
          }
          uint8_t* e = mmq + mm_base + (incl - mine);
          *e++ = ',';
          uint32_t v = skip;
          for (uint32_t d = nd; d-- > 0;) { e[d] = (uint8_t)('0' + v % 10u); v /= 10u; }
        }
        ml_base += (uint32_t)__popcll(mh);
        mm_base += uni((uint32_t)__shfl((int)incl, 63));
      }
      if (lane == 0) { mmq[mm_len] = ';'; mmq[mm_len + 1] = 0; }
      q = w == 2 ? ml + 8 + n_hit : ml;
    }
    for (int a = 0; a < 2; a++) {                                                 // <s>u, <s>t: the counts as B:s
      if (lane < 8) q[lane] = lane == 0 ? s0 : lane == 1 ? (uint8_t)(a == 0 ? 'u' : 't') : lane == 2 ? (uint8_t)'B' : lane == 3 ? (uint8_t)'s' : (uint8_t)(n >> (8 * (lane - 4)));
      for (uint32_t i = lane; i < n; i += 64) {
        const DMethCol c = duplex_meth_col(P, a_off, b_off, has_ba, w, i);
        const uint32_t v = a == 0 ? c.u : c.t;
        q[8 + 2 * i] = (uint8_t)v; q[9 + 2 * i] = (uint8_t)(v >> 8);
      }
      q += 8 + 2 * n;
    }
  }
}
