// simplex_wide.inc — simplex families the streaming kernels of simplex_deep.inc refuse for SIZE alone (FGX_DEEP_WIDE=1; default off): more than
// DEEP_MAX records without a cap, more than DEEP_CAP_MAX under --max-reads, or an end that keeps more than 255 reads — up to WIDE_MAX records.
// Included by fastpath.hip inside `namespace fgx { namespace {` after simplex_deep.inc, whose DeepRow / DeepFam / deep_correct it shares.
//
// What fixes the 255 of simplex_deep.inc is a counter's width: the observation counts of a FullItem are a byte each (fastpath.h), and k_deep_cols keeps
// its four per-chain counts in one word.  Here the counts are a word each, and a column the unanimous gate does not answer is called in the column
// kernel itself (call_full, consensus_math.h): in a family this deep nearly every column shows a second base, so every lane needs the chain anyway, and
// FullItem and k_call_full stay as they are.
//
//   k_wide_parse   a workgroup per family: k_deep_parse<.., .., 0>'s phases in its order (the parse is the same function, deep_parse_records), with its counters and refusals.  The per-record state lies
//                  in a global scratch (struct of arrays; a family's slice starts at the scan of the listed families' record counts, where its rows
//                  start too); LDS holds only what the inner loops read again for every record: the pairing keys, the end bits and the final lengths
//                  (7 bytes per record, dynamic, sized by the largest listed family: 112 KB at WIDE_MAX, of the CU's 160 KB).  The O(n^2) loops
//                  stay — pairing, the rank under the cap, the min_reads-th-longest rule, the row index —: their trip counts are functions of n alone.
//   k_wide_cols    a wavefront per (family, end, 64-column pass).  The Kahan chains of a column are summed in file order (base_builder.rs:836-868),
//                  so the rows of an end cannot be split; its columns can: a 2 x 150-column family gives six wavefronts where k_deep_cols's layout
//                  would walk 16 384 rows six times in one.  The scan of the families' pass counts maps a wavefront to its item.
//   k_wide_finish  a wavefront per family: consensus UMI (k_deep_cols's block, unresolved characters called here), the items' depth extremes,
//                  record sizes, EndDescs, counters.  A launch of its own: no hand-shake with k_wide_cols.
//
// An end keeps at most WIDE_MAX = 16 384 reads, below 32 767: the reference's clamps of depth and errors to i16::MAX (vanilla_caller.rs:1730-1739)
// never apply inside these kernels and are not implemented; a family above WIDE_MAX leaves for k_family as it did.
// Out of this path's shape, as of k_deep_parse<.., .., 0>: indel / clipped reads, an end of mapped AND unmapped records, a fragment consensus
// beside a pair, RX of unequal length or above FAST_RX_CAP; and the methylation-aware mode, --trim (the host does not launch these kernels then).

constexpr uint32_t WIDE_MAX = 16384;         // records per family
constexpr uint32_t WIDE_NT = 512;            // threads of k_wide_parse
constexpr uint32_t WIDE_LDS_PER_REC = 7;     // key (4) + final length (2) + bits (1)
constexpr uint32_t WIDE_LDS_BYTES = WIDE_MAX * WIDE_LDS_PER_REC;
constexpr uint32_t WIDE_REC_BYTES = 40;      // global scratch per record (WideRecs)
static_assert(WIDE_LDS_BYTES + 1024 <= 160 * 1024, "k_wide_parse: the CU's LDS");
static_assert(WIDE_MAX / WIDE_NT <= 32, "k_wide_parse: the dropped reads of a thread are bits of one word");
static_assert(WIDE_MAX <= 32767 && WIDE_MAX <= 65535, "no i16 clamp inside the wide kernels; DeepFam::m_a / m_b are 16 bits");

struct WideParams {
  const uint32_t* list; uint32_t n_list;     // what the streaming kernels left
  const uint64_t* row0;                      // per list entry: first DeepRow = first scratch record (exclusive scan of the record counts)
  uint64_t n_rows;                           // records of all listed families, rounded up to a multiple of 8 (the scratch arrays' stride)
  uint8_t* scratch;                          // WIDE_REC_BYTES * n_rows
  DeepRow* rows; DeepFam* fams;
  uint32_t* out_list; uint32_t* n_out;       // not this path's → k_family
  uint64_t* passes;                          // per list entry: 64-column passes of its ends (0: not taken); zeroed before k_wide_parse
  const uint64_t* pass0;                     // ... their exclusive scan (k_wide_cols, k_wide_finish)
  uint32_t n_items;                          // all passes
  uint32_t lds_recs;                         // records k_wide_parse's LDS arrays hold: the largest listed family it takes, in sixty-fours
  uint2* item_depth;                         // per item: max / min depth of its columns
};

// the per-record state of k_wide_parse, named as DeepLds names it: global scratch, beside the three LDS arrays
struct WideRecs {
  unsigned long long* off;
  int32_t* pos; int32_t* ref_id;
  uint32_t* partner;                         // the mate this read shares positions with; 0xFFFFFFFF: none
  uint16_t* l_seq; uint16_t* seq_rel; uint16_t* name_len; uint16_t* clip; uint16_t* wo; uint16_t* mo; uint16_t* wc; uint16_t* rx_rel; uint16_t* cb_rel;
  uint8_t* rx_len; uint8_t* cb_len;
  uint32_t* key; uint16_t* final_len; uint8_t* bits;      // LDS
};
struct WideCnt {
  uint32_t bad, cnt[3], rem[3], fmin[3], fmax[3], rxcnt[3], rxfirst[3], rxbad, ov_agree, ov_dis, ov_corr;
  uint32_t clen[3];
};

// n of each listed family (k_deep_sizes), and the largest n that is not above WIDE_MAX: what k_wide_parse's LDS arrays must hold
__global__ void k_wide_sizes(const uint32_t* __restrict__ list, uint32_t n_list, const uint32_t* __restrict__ grp_first, uint64_t* __restrict__ sizes, uint32_t* __restrict__ n_max) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t n = 0;
  if (i < n_list) { const uint32_t g = list[i]; n = grp_first[g + 1] - grp_first[g]; sizes[i] = n; }
  const uint32_t m = wave_max(n <= WIDE_MAX ? n : 0u);
  if ((threadIdx.x & 63) == 0 && m) atomicMax(n_max, m);
}

__global__ __launch_bounds__(WIDE_NT) void k_wide_parse(FastParams P, WideParams D) {
  constexpr uint32_t DEEP_NT = WIDE_NT;
  FGX_DYN_LDS(lds);
  __shared__ WideCnt C;
  __shared__ __align__(16) uint8_t sTagCls[256];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t li = blockIdx.x;
  const uint32_t g = D.list[li];
  const uint32_t r0 = P.grp_first[g], n = P.grp_first[g + 1] - r0;
  DeepFam* const F = &D.fams[li];
  fill_tag_classes(sTagCls);
  if (tid == 0) {
    C.bad = 0; C.rxbad = 0; C.ov_agree = C.ov_dis = C.ov_corr = 0;
    for (int e = 0; e < 3; e++) { C.cnt[e] = C.rem[e] = 0; C.fmin[e] = 0xFFFFFFFFu; C.fmax[e] = 0; C.rxcnt[e] = 0; C.rxfirst[e] = 0xFFFFFFFFu; C.clen[e] = 0; }
  }
  // not this path's: k_family decides (and defers what no device kernel takes)
  auto leave = [&]() {
    if (tid == 0) { F->status = 0; const uint32_t k = atomicAdd(D.n_out, 1u); D.out_list[k] = g; }
  };
  if (tid < 3) { P.ends[3 * g + tid].valid = 0; P.rec_sizes[3 * g + tid] = 0; }
  if (n > WIDE_MAX || n > D.lds_recs || n == 0 || n < P.min_reads) { leave(); return; }   // (uniform; lds_recs: the host sized it from these very counts)
  __syncthreads();
  // A family the DEEP_MAX build can hold, none of whose ends has more than 255 RECORDS, was not refused for size: it goes on as it came, without a
  // second parse (one flag word per record)
  if (n <= DEEP_MAX) {
    for (uint32_t r = tid; r < n; r += DEEP_NT) {
      const unsigned long long off = P.rec_off[r0 + r];
      const uint32_t len = P.rec_len[r0 + r];
      if (len < 36u || len > 0xFFFFu || off > P.blob_len || (unsigned long long)len > P.blob_len - off) atomicOr(&C.bad, 1u);
      else { const uint32_t flags = gld32(P.blob + off + 12) >> 16; atomicAdd(&C.cnt[!(flags & bam::F_PAIRED) ? 0u : (flags & bam::F_FIRST) ? 1u : 2u], 1u); }
    }
    __syncthreads();
    const bool pass = (C.bad & 1u) || (C.cnt[0] <= 255u && C.cnt[1] <= 255u && C.cnt[2] <= 255u);
    __syncthreads();
    if (pass) { leave(); return; }
    if (tid < 3) C.cnt[tid] = 0;
    __syncthreads();
  }
  WideRecs S;
  {
    const unsigned long long N = D.n_rows, b = D.row0[li];
    uint8_t* const w = D.scratch;
    S.off = (unsigned long long*)w + b;
    S.pos = (int32_t*)(w + 8 * N) + b; S.ref_id = (int32_t*)(w + 12 * N) + b; S.partner = (uint32_t*)(w + 16 * N) + b;
    uint16_t* const h = (uint16_t*)(w + 20 * N);
    S.l_seq = h + b; S.seq_rel = h + N + b; S.name_len = h + 2 * N + b; S.clip = h + 3 * N + b; S.wo = h + 4 * N + b; S.mo = h + 5 * N + b; S.wc = h + 6 * N + b;
    S.rx_rel = h + 7 * N + b; S.cb_rel = h + 8 * N + b;
    S.rx_len = w + 38 * N + b; S.cb_len = w + 39 * N + b;
    S.key = (uint32_t*)lds; S.final_len = (uint16_t*)(lds + 4 * D.lds_recs); S.bits = lds + 6 * D.lds_recs;
  }
  const uint32_t min_bq = P.min_input_bq & 0xFFu;

  // ---- 1. parse: thread = record (deep_parse_records, simplex_deep.inc) ---------------------------------------------------------------
  deep_parse_records<0>(P, S, C, r0, n, tid, DEEP_NT, sTagCls, true);
  __syncthreads();
  if (C.bad & 1u) { leave(); return; }
  if (C.bad >> 1) {
    // some record is unmapped (workgroup-uniform): bits 4 - 6, the end holds a mapped record.  An end with both is not this path's
    for (uint32_t r = tid; r < n; r += DEEP_NT) if (!(S.bits[r] & 64u)) atomicOr(&C.bad, 16u << (S.bits[r] & 3u));
    __syncthreads();
    const uint32_t b = C.bad;
    if ((b >> 1) & (b >> 4) & 7u) { leave(); return; }
  }

  // ---- 2. pairs (pair map: per name the LAST R1-type and the LAST R2-type primary record; an R1 is paired unless a later R1 has its
  //         name) and the reference span each pair shares ----------------------------------------------------------------------------------
  if (P.overlap) {
    for (uint32_t a = tid; a < n; a += DEEP_NT) {
      const uint32_t ka = S.key[a];
      if ((ka & 3u) != 1u) continue;
      uint32_t cmate = 0xFFFFFFFFu, clater = 0xFFFFFFFFu;
      for (uint32_t j = 0; j < n; j++) {
        const uint32_t d = S.key[j] ^ ka;
        if (d == 0 && j > a) clater = j;
        if (d == 3) cmate = j;
      }
      const uint32_t other = clater != 0xFFFFFFFFu ? clater : cmate;
      if (other == 0xFFFFFFFFu) continue;
      const uint32_t nl = S.name_len[a];
      bool same = S.name_len[other] == nl;
      const uint8_t* const na = P.blob + S.off[a] + 32;
      const uint8_t* const nb = P.blob + S.off[other] + 32;
      for (uint32_t i = 0; i < nl && same; i += 8) {
        unsigned long long wa = gld64(na + i), wb = gld64(nb + i);
        if (i + 8 > nl) { const unsigned long long mk = (1ULL << (8 * (nl - i))) - 1; wa &= mk; wb &= mk; }
        if (wa != wb) same = false;
      }
      if (!same) { atomicOr(&C.bad, 1u); continue; }        // equal hashes, different names: the exact rules live in k_family
      if (clater != 0xFFFFFFFFu) continue;                  // a later R1 carries the name: this one is not paired
      const uint32_t b = cmate;
      if (S.ref_id[a] != S.ref_id[b]) continue;
      const int32_t s1 = S.pos[a] + 1, e1 = S.pos[a] + (int32_t)S.l_seq[a], s2 = S.pos[b] + 1, e2 = S.pos[b] + (int32_t)S.l_seq[b];
      const int32_t lox = s1 > s2 ? s1 : s2, hix = e1 < e2 ? e1 : e2;
      if (hix < lox) continue;
      const uint32_t cnt = (uint32_t)(hix - lox + 1), o1 = (uint32_t)(lox - s1), o2 = (uint32_t)(lox - s2);
      S.wo[a] = (uint16_t)o1; S.mo[a] = (uint16_t)o2; S.wc[a] = (uint16_t)cnt; S.partner[a] = b;
      S.wo[b] = (uint16_t)o2; S.mo[b] = (uint16_t)o1; S.wc[b] = (uint16_t)cnt; S.partner[b] = a;
    }
    __syncthreads();
    if (C.bad & 1u) { leave(); return; }
    // the overlapping-bases counters (overlapping.rs:51-60): a wavefront per pair, lane = shared position
    uint32_t ov_agree = 0, ov_dis = 0, ov_corr = 0;
    for (uint32_t a = wv; a < n; a += DEEP_NT / 64) {
      if ((S.key[a] & 3u) != 1u || S.wc[a] == 0) continue;   // (uniform per wavefront)
      const uint32_t b = S.partner[a];
      const uint8_t* const sa = P.blob + S.off[a] + S.seq_rel[a];
      const uint8_t* const sb = P.blob + S.off[b] + S.seq_rel[b];
      const uint32_t qa0 = ((uint32_t)S.l_seq[a] + 1u) >> 1, qb0 = ((uint32_t)S.l_seq[b] + 1u) >> 1;
      const uint32_t cn = S.wc[a], o1 = S.wo[a], o2 = S.mo[a];
      for (uint32_t x = lane; x < cn; x += 64) {
        const uint32_t i1 = o1 + x, i2 = o2 + x;
        const uint32_t c1 = ((uint32_t)sa[i1 >> 1] >> ((~i1 & 1u) << 2)) & 15u, c2 = ((uint32_t)sb[i2 >> 1] >> ((~i2 & 1u) << 2)) & 15u;
        if (c1 == 15u || c2 == 15u) continue;
        const uint32_t qa = sa[qa0 + i1], qb = sb[qb0 + i2];
        if (c1 == c2) { const uint32_t sm = qa + qb, nq = sm < 93u ? sm : 93u; ov_agree++; ov_corr += (nq != qa || nq != qb) ? 1u : 0u; }
        else { ov_dis++; ov_corr += 2u; }
      }
    }
    ov_agree = wave_sum(ov_agree); ov_dis = wave_sum(ov_dis); ov_corr = wave_sum(ov_corr);
    if (lane == 0) { if (ov_agree) atomicAdd(&C.ov_agree, ov_agree); if (ov_dis) atomicAdd(&C.ov_dis, ov_dis); if (ov_corr) atomicAdd(&C.ov_corr, ov_corr); }
  }
  __syncthreads();

  // ---- 3. final length per read: up to the mate clip, without its trailing N / masked bases — of what the pre-correction leaves
  //         there (vanilla_caller.rs:1129-1160; no --trim in this shape) ---------------------------------------------------------------
  for (uint32_t r = tid; r < n; r += DEEP_NT) {
    const uint32_t l_seq = S.l_seq[r], clip = S.clip[r];
    const bool rev = (S.bits[r] & 4u) != 0;
    const uint8_t* const sq = P.blob + S.off[r] + S.seq_rel[r];
    const uint32_t q0 = (l_seq + 1u) >> 1;
    const uint32_t wc = S.wc[r], wo = S.wo[r], mo = S.mo[r];
    const uint8_t* sm = sq;
    uint32_t mq0 = 0;
    if (wc) { const uint32_t b = S.partner[r]; sm = P.blob + S.off[b] + S.seq_rel[b]; mq0 = ((uint32_t)S.l_seq[b] + 1u) >> 1; }
    uint32_t flr = l_seq > clip ? l_seq - clip : 0u;
    while (flr > 0) {
      const uint32_t idx = rev ? l_seq - flr : flr - 1u;
      uint32_t cc = ((uint32_t)sq[idx >> 1] >> ((~idx & 1u) << 2)) & 15u, qq = sq[q0 + idx];
      if (idx - wo < wc) {
        const uint32_t j = mo + (idx - wo);
        deep_correct(cc, qq, ((uint32_t)sm[j >> 1] >> ((~j & 1u) << 2)) & 15u, sm[mq0 + j]);
      }
      if (cc != 15u && qq >= min_bq) break;
      flr--;
    }
    S.final_len[r] = (uint16_t)flr;
    const uint32_t e = S.bits[r] & 3u;
    atomicAdd(&C.cnt[e], 1u);
    if (flr > 0) { atomicAdd(&C.rem[e], 1u); atomicMin(&C.fmin[e], flr); atomicMax(&C.fmax[e], flr); }
  }
  __syncthreads();

  // ---- 4. family gates (process_group :1329-1422, process_subgroup :1454-1646), as k_deep_parse takes them ---------------------------
  bool ok[3] = {false, false, false};
  uint32_t rej_insuf = 0, rej_zero = 0, rej_orphan = 0, rej_down = 0;
  bool rank_rule = false;
  bool cand[3] = {false, false, false}, cut[3] = {false, false, false};   // the end reaches the cap / the cap bites on it
  uint32_t rem0[3] = {0, 0, 0};                              // retained reads of the end before the cut
  bool capped = false;
  for (uint32_t e = 0; e < 3; e++) {
    const uint32_t cnt = C.cnt[e], rem = C.rem[e];
    if (cnt == 0) continue;
    if (cnt < P.min_reads) { rej_insuf += cnt; continue; }
    rej_zero += cnt - rem;
    if (rem < P.min_reads) { rej_insuf += rem; continue; }
    if (rem == 0) continue;
    cand[e] = true; rem0[e] = rem;
    if (P.max_reads >= 0 && (long long)rem > P.max_reads) { cut[e] = true; capped = true; }
  }
  // --max-reads (downsample_filtered_source_reads :902-932): of an end above the cap the max_reads lowest fgbio name ranks stay, ties in file
  // order, and the survivors keep their file order.  A dropped read becomes a read of final length 0.  (Workgroup-uniform.)
  if (capped) {
    for (uint32_t r = tid; r < n; r += DEEP_NT)              // (the pairing hash is done with: `key` holds the rank from here on)
      if (cut[S.bits[r] & 3u] && S.final_len[r] > 0) S.key[r] = (uint32_t)name_rank(P.blob + S.off[r] + 32, S.name_len[r]);
    __syncthreads();
    uint32_t drop = 0;                                       // bit k: record tid + k * DEEP_NT is dropped
    for (uint32_t r = tid, k = 0; r < n; r += DEEP_NT, k++) {
      const uint32_t e = S.bits[r] & 3u;
      if (!cut[e] || S.final_len[r] == 0) continue;
      const int32_t rk = (int32_t)S.key[r];
      uint32_t before = 0;
      for (uint32_t j = 0; j < n; j++) {
        if ((S.bits[j] & 3u) != e || S.final_len[j] == 0) continue;
        const int32_t rj = (int32_t)S.key[j];
        before += (rj < rk || (rj == rk && j < r)) ? 1u : 0u;
      }
      if ((long long)before >= P.max_reads) drop |= 1u << k;
    }
    if (tid == 0)                                            // (every thread read them for the gates above, a barrier ago)
      for (uint32_t e = 0; e < 3; e++) if (cut[e]) { C.rem[e] = 0; C.fmin[e] = 0xFFFFFFFFu; C.fmax[e] = 0; }
    __syncthreads();
    for (uint32_t r = tid, k = 0; r < n; r += DEEP_NT, k++) {
      const uint32_t e = S.bits[r] & 3u, fl = S.final_len[r];
      if (!cut[e] || fl == 0) continue;
      if ((drop >> k) & 1u) S.final_len[r] = 0;
      else { atomicAdd(&C.rem[e], 1u); atomicMin(&C.fmin[e], fl); atomicMax(&C.fmax[e], fl); }
    }
    __syncthreads();
  }
  for (uint32_t e = 0; e < 3; e++) {
    if (!cand[e]) continue;
    const uint32_t rem = C.rem[e];
    if (cut[e]) {
      rej_down += rem0[e] - rem;
      if (rem < P.min_reads) { rej_insuf += rem; continue; }   // (a cap below --min-reads)
      if (rem == 0) continue;
    }
    ok[e] = true;                                            // (up to WIDE_MAX reads: the counts below are words)
    if (C.fmin[e] != C.fmax[e] && P.min_reads > 1) rank_rule = true;
  }
  // consensus length of an end: one final length → that; --min-reads 1 → the longest; else the min_reads-th longest (:1661-1669)
  if (rank_rule) {
    for (uint32_t r = tid; r < n; r += DEEP_NT) {
      const uint32_t e = S.bits[r] & 3u, fl = S.final_len[r];
      if (!ok[e] || fl == 0 || C.fmin[e] == C.fmax[e]) continue;
      uint32_t ge = 0;
      for (uint32_t j = 0; j < n; j++) ge += ((S.bits[j] & 3u) == e && S.final_len[j] >= fl) ? 1u : 0u;
      if (ge >= P.min_reads) atomicMax(&C.clen[e], fl);
    }
    __syncthreads();
  }
  uint32_t clen[3];
  for (uint32_t e = 0; e < 3; e++) clen[e] = !ok[e] ? 0u : (C.fmin[e] == C.fmax[e] || P.min_reads <= 1) ? C.fmax[e] : C.clen[e];
  const bool has_frag = ok[0], has_pair = ok[1] && ok[2];
  if (has_frag && has_pair) { leave(); return; }             // three consensus reads from one family: k_family
  if (!has_pair) { if (ok[1]) rej_orphan += C.rem[1]; else if (ok[2]) rej_orphan += C.rem[2]; }
  const uint32_t ne = has_frag ? 1u : has_pair ? 2u : 0u;
  const uint32_t type_a = has_frag ? 0u : 1u, end_a = has_frag ? 0u : 1u;
  const uint32_t m_a = ne ? C.rem[end_a] : 0u, m_b = ne == 2u ? C.rem[2] : 0u;
  // ---- 5. member rows: end A's retained reads, then end B's, file order inside an end; the UMIs they carry -------------------------
  const unsigned long long row0 = D.row0[li];
  for (uint32_t r = tid; r < n; r += DEEP_NT) {
    const uint32_t e = S.bits[r] & 3u, fl = S.final_len[r];
    const bool mine = ne != 0 && fl > 0 && (e == end_a || (ne == 2u && e == 2u));
    if (!mine) continue;
    uint32_t rank = 0;
    for (uint32_t j = 0; j < r; j++) rank += ((S.bits[j] & 3u) == e && S.final_len[j] > 0) ? 1u : 0u;
    const uint32_t row = (e == end_a ? 0u : m_a) + rank;
    DeepRow R;
    const unsigned long long so = S.off[r] + S.seq_rel[r];
    unsigned long long mso = so;
    uint32_t ml = S.l_seq[r];
    if (S.wc[r]) { const uint32_t b = S.partner[r]; mso = S.off[b] + S.seq_rel[b]; ml = S.l_seq[b]; }
    const bool hrx = (S.bits[r] & 8u) != 0;
    R.w[0] = (uint32_t)so; R.w[1] = (uint32_t)(so >> 32); R.w[2] = (uint32_t)mso; R.w[3] = (uint32_t)(mso >> 32);
    R.w[4] = (uint32_t)S.l_seq[r] | (fl << 16);
    R.w[5] = ml | ((uint32_t)S.wo[r] << 16);
    R.w[6] = (uint32_t)S.mo[r] | ((uint32_t)S.wc[r] << 16);
    R.w[7] = ((hrx ? (uint32_t)S.rx_rel[r] - (uint32_t)S.seq_rel[r] : 0u) & 0xFFFFu) | ((((S.bits[r] & 4u) ? 1u : 0u) | (hrx ? 2u : 0u)) << 16) | ((uint32_t)S.rx_len[r] << 24);
    D.rows[row0 + row] = R;
    if (hrx) { atomicAdd(&C.rxcnt[e], 1u); atomicMin(&C.rxfirst[e], r); }
  }
  __syncthreads();
  // UMIs of unequal length → consensus_umis panics → the general path reports it (vanilla_caller.rs:1842-1856)
  for (uint32_t r = tid; r < n; r += DEEP_NT) {
    const uint32_t e = S.bits[r] & 3u;
    if (!(S.bits[r] & 8u) || S.final_len[r] == 0 || C.rxfirst[e] == 0xFFFFFFFFu) continue;
    if (S.rx_len[r] != S.rx_len[C.rxfirst[e]]) C.rxbad = 1;
  }
  __syncthreads();
  if (tid == 0 && ne) {
    if (C.rxcnt[end_a] && S.rx_len[C.rxfirst[end_a]] > FAST_RX_CAP) C.rxbad = 1;
    if (ne == 2u && C.rxcnt[2] && S.rx_len[C.rxfirst[2]] > FAST_RX_CAP) C.rxbad = 1;
  }
  __syncthreads();
  if (C.rxbad) { leave(); return; }

  // ---- 6. the family's descriptor, its pass count, and what the EndDescs hold that does not depend on the columns -------------------
  if (tid == 0) {
    DeepFam f;
    __builtin_memset(&f, 0, sizeof(f));
    f.status = 1; f.n = n; f.row0 = (uint32_t)row0;
    f.m_a = (uint16_t)m_a; f.m_b = (uint16_t)m_b; f.lc_a = (uint16_t)(ne ? clen[end_a] : 0u); f.lc_b = (uint16_t)(ne == 2u ? clen[2] : 0u);
    f.ne = (uint8_t)ne; f.type_a = (uint8_t)type_a;
    f.rx_cnt_a = (uint16_t)(ne ? C.rxcnt[end_a] : 0u); f.rx_cnt_b = (uint16_t)(ne == 2u ? C.rxcnt[2] : 0u);
    f.rx_len_a = (uint8_t)((ne && C.rxcnt[end_a]) ? S.rx_len[C.rxfirst[end_a]] : 0u);
    f.rx_len_b = (uint8_t)((ne == 2u && C.rxcnt[2]) ? S.rx_len[C.rxfirst[2]] : 0u);
    f.rej_insuf = rej_insuf; f.rej_zero = rej_zero; f.rej_orphan = rej_orphan; f.rej_down = rej_down;
    f.ov_agree = C.ov_agree; f.ov_dis = C.ov_dis; f.ov_corr = C.ov_corr;
    *F = f;
    D.passes[li] = (uint64_t)(((uint32_t)f.lc_a + 63u) >> 6) + (((uint32_t)f.lc_b + 63u) >> 6);
  }
  if (tid < ne) {
    const uint32_t k = tid, e = k == 0 ? end_a : 2u;
    uint32_t fk = 0;                                         // first retained read of the end: cell-barcode source
    while (fk < n && !((S.bits[fk] & 3u) == e && S.final_len[fk] > 0)) fk++;
    EndDesc* const E = &P.ends[3 * g + e];
    // mi of record 0: its tag walk again (one thread; the value offset was not kept per record)
    const uint8_t* const rec0 = P.blob + S.off[0];
    AuxTags ax;
    {
      const uint32_t l_seq0 = S.l_seq[0];
      const uint32_t aux_off = (uint32_t)S.seq_rel[0] + ((l_seq0 + 1u) >> 1) + l_seq0;
      aux_walk(rec0, sTagCls, aux_off, P.rec_len[r0] - aux_off, P, ax);
    }
    E->col_off = P.col_base[g] + (k == 0 ? 0u : clen[end_a]);
    E->cons_len = clen[e];
    E->first_off = S.off[0]; E->kept_off = S.off[fk];
    E->type = (uint8_t)e;
    E->mi_off = (uint16_t)(ax.pk_mi & 0xFFFF); E->mi_len = (uint8_t)(ax.pk_mi >> 16);
    const bool hcb = P.cell0 && (S.bits[fk] & 16u);
    E->has_cb = hcb ? 1 : 0; E->cb_off = S.cb_rel[fk]; E->cb_len = S.cb_len[fk];
    E->has_rx = C.rxcnt[e] > 0; E->rx_len = (uint8_t)(C.rxcnt[e] ? S.rx_len[C.rxfirst[e]] : 0u);
    E->rec_size = 0; E->valid = 0;                           // k_wide_finish: the sizes of the cD / cM values depend on the depths
    E->meth = 0;
  }
}

// the list entry whose passes hold item `it`: the last one whose first pass is not behind it (entries without passes share their successor's start)
__device__ __forceinline__ uint32_t wide_family_of(const uint64_t* __restrict__ pass0, uint32_t n_list, uint32_t it) {
  uint32_t lo = 0, hi = n_list;
  while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (pass0[mid] <= (uint64_t)it) lo = mid; else hi = mid; }
  return lo;
}

// -----------------------------------------------------------------------------------------------------------------------------
// k_wide_cols — wavefront = 64 columns of one end of one family, lane = column, the rows streamed from global memory in file order
// -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_wide_cols(FastParams P, WideParams D) {
  __shared__ __align__(16) S2Lds sL;
  GateTables& sT = sL.g;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  {
    constexpr uint32_t IMG_V = (uint32_t)(sizeof(S2Lds) / 16);
    const u32x4* const src = (const u32x4*)P.s2_image;
    u32x4* const dst = (u32x4*)&sL;
    for (uint32_t i = threadIdx.x; i < IMG_V; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  const uint32_t item = blockIdx.x * (blockDim.x >> 6) + wv;
  if (item >= D.n_items) return;
  const uint32_t li = uni(wide_family_of(D.pass0, D.n_list, item));
  const DeepFam* const Fp = &D.fams[li];
  if (uni(Fp->status) != 1u) return;                         // (an item belongs to a family that was taken: its passes were counted)
  const uint32_t g = uni(D.list[li]);
  const uint32_t lc_a = uni(Fp->lc_a), lc_b = uni(Fp->lc_b), m_a = uni(Fp->m_a), m_b = uni(Fp->m_b);
  const uint32_t ps = uni(item - (uint32_t)D.pass0[li]), na = (lc_a + 63u) >> 6;
  const bool second = ps >= na;
  const uint32_t m = second ? m_b : m_a, Lc = second ? lc_b : lc_a, coff = second ? lc_a : 0u;
  const uint32_t p0s = uni((second ? ps - na : ps) << 6);
  if (p0s >= Lc) return;                                     // (never: the pass count is the ends' columns in sixty-fours)
  const DeepRow* const rows = D.rows + uni(Fp->row0) + (second ? m_a : 0u);
  const uint64_t col_base = uniform_u64(P.col_base[g]);
  uint8_t* const fam_code = P.col_code + col_base;
  uint8_t* const fam_qual = P.col_qual + col_base;
  uint16_t* const fam_depth = P.col_depth + col_base;
  uint16_t* const fam_err = P.col_err + col_base;
  const uint8_t* const pairs = (const uint8_t*)&sL.pair[0][0];
  const uint8_t* const blob = P.blob;
  const uint32_t min_bq = uni((uint32_t)P.min_input_bq & 0xFFu);
  const DeviceTables* T = P.T;
  // the rows through the scalar unit (k_deep_cols's: k_wide_parse wrote them, a kernel boundary ago)
  typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
  typedef const FGX_CONST_AS u32x8* RowPtr;
  auto row_seq = [&](const u32x8& r) { return blob + (((unsigned long long)r[1] << 32) | r[0]); };
  auto row_mate = [&](const u32x8& r) { return blob + (((unsigned long long)r[3] << 32) | r[2]); };
  const RowPtr er = (RowPtr)rows;
  const uint32_t p = p0s + lane;
  const bool incol = p < Lc;
  const uint32_t oc = coff + p;
  uint32_t lmax = 0, lmin = 0xFFFFFFFFu;
  if (m == 1) {   // single-read consensus: LUT keyed by the unclamped quality (:1677-1708)
    const u32x8 R = er[0];
    const uint32_t L = R[4] & 0xFFFFu, fin = R[4] >> 16, wo = R[5] >> 16, mo = R[6] & 0xFFFFu, wc = R[6] >> 16, mL = R[5] & 0xFFFFu;
    const bool rv = ((R[7] >> 16) & 1u) != 0;
    const uint8_t* const sq = row_seq(R);
    const uint8_t* const sm = row_mate(R);
    if (incol) {
      const bool in = p < fin;
      const uint32_t idx = in ? (rv ? L - 1u - p : p) : 0u;
      uint32_t code = ((uint32_t)sq[idx >> 1] >> ((~idx & 1u) << 2)) & 15u, qq = sq[((L + 1u) >> 1) + idx];
      if (in && idx - wo < wc) { const uint32_t j = mo + (idx - wo); deep_correct(code, qq, ((uint32_t)sm[j >> 1] >> ((~j & 1u) << 2)) & 15u, sm[((mL + 1u) >> 1) + j]); }
      if (rv) code = __builtin_bitreverse32(code) >> 28;
      if (!in) { code = 15; qq = FGX_MIN_PHRED; }
      if (qq < min_bq) { code = 15; qq = FGX_MIN_PHRED; }
      const uint8_t adj = qq < 94 ? T->single_input_quals[qq] : 0;
      uint8_t ob, oq;
      if (adj < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; } else { ob = (uint8_t)code; oq = adj; }
      const uint32_t dd = code != 15 ? 1u : 0u;
      fam_code[oc] = ob; fam_qual[oc] = oq; fam_depth[oc] = (uint16_t)dd; fam_err[oc] = 0;
      lmax = dd; lmin = dd;
    }
  } else {
    const uint32_t shp = (~p & 1u) << 2;                     // nibble shift of an even / odd index (a reverse read of even length flips it)
    // Kahan chains by order of appearance (ChainAcc, consensus_math.h), all four updated by every observation, as k_deep_cols keeps them;
    // their observation counts a word each
    double s1 = 0.0, c1 = 0.0, s2 = 0.0, c2k = 0.0, s3 = 0.0, c3 = 0.0, sR = 0.0, cR = 0.0;
    uint32_t b1 = 0, b2 = 0, b3 = 0, n1 = 0, n2 = 0, n3 = 0, nR = 0;
    constexpr int NB = FGX_DEEP_BATCH;
    for (uint32_t j0 = 0; j0 < m; j0 += NB) {
      u32x8 R_[NB];
#pragma unroll
      for (int t = 0; t < NB; t++) R_[t] = er[uni(j0 + t < m ? j0 + t : m - 1u)];   // (past the end: the last row again, not observed)
      uint32_t b_[NB], q_[NB], b2_[NB], q2_[NB], d_[NB];
      bool in_[NB];
      // every load of the batch is issued before the first of them is used
#pragma unroll
      for (int t = 0; t < NB; t++) {
        const u32x8& R = R_[t];
        const uint32_t L = R[4] & 0xFFFFu, fin = R[4] >> 16;
        const bool rv = ((R[7] >> 16) & 1u) != 0;
        const uint32_t lim = fin < Lc ? fin : Lc;            // inside the read's final length AND a column of the consensus
        in_[t] = p < lim && (j0 + t < m);
        const uint32_t xm = rv ? ~0u : 0u, xk = rv ? L : 0u;  // index into the read: forward p, reverse L - 1 - p = (p ^ ~0) + L
        const uint32_t ix = in_[t] ? (p ^ xm) + xk : 0u;
        const uint8_t* const sq = row_seq(R);
        b_[t] = sq[ix >> 1]; q_[t] = sq[((L + 1u) >> 1) + ix];
        b2_[t] = 0; q2_[t] = 0; d_[t] = 0xFFFFFFFFu;
        const uint32_t wo = R[5] >> 16, wc = R[6] >> 16;
        // the row shares positions with its mate inside THIS pass's window of indices (all scalar)
        const int32_t lo = rv ? (int32_t)L - 64 - (int32_t)p0s : (int32_t)p0s;
        if (wc != 0 && lo < (int32_t)(wo + wc) && lo + 63 >= (int32_t)wo) {
          const uint32_t d = ix - wo, mo = R[6] & 0xFFFFu, mL = R[5] & 0xFFFFu;
          const bool hit = in_[t] && d < wc;
          const uint32_t j = hit ? mo + d : 0u;
          const uint8_t* const sm = row_mate(R);
          b2_[t] = sm[j >> 1]; q2_[t] = sm[((mL + 1u) >> 1) + j];
          d_[t] = hit ? j : 0xFFFFFFFFu;                    // (the mate's index: its parity picks the nibble)
        }
      }
#pragma unroll
      for (int t = 0; t < NB; t++) {
        const u32x8& R = R_[t];
        const bool rv = ((R[7] >> 16) & 1u) != 0;
        const uint32_t L = R[4] & 0xFFFFu;
        uint32_t c = __builtin_amdgcn_ubfe(b_[t], shp ^ ((rv && !(L & 1u)) ? 4u : 0u), 4u), q = q_[t];   // parity of L - 1 - p = parity of p when L is odd
        if (d_[t] != 0xFFFFFFFFu) deep_correct(c, q, __builtin_amdgcn_ubfe(b2_[t], (~d_[t] & 1u) << 2, 4u), q2_[t]);
        if (rv) c = __builtin_bitreverse32(c) >> 28;         // complement = bit reversal of the code
        const bool valid = in_[t] && q >= min_bq && __builtin_amdgcn_ubfe(0x116u, c, 1u) != 0;   // inside the read, not masked, one of A C G T
        const double2 pr = *(const double2*)(pairs + S2_PAIR_OFF(q & 0xFFu));
        if (valid) {
          if (b1 == 0) b1 = c;
          else if (c != b1 && c != b2 && c != b3) {
            if (b2 == 0) { b2 = c; s2 = sR; c2k = cR; }
            else if (b3 == 0) { b3 = c; s3 = sR; c3 = cR; }
          }
          const bool h1 = c == b1, h2 = c == b2, h3 = c == b3;
          kahan2(s1, c1, h1 ? pr.x : pr.y);
          kahan2(s2, c2k, h2 ? pr.x : pr.y);
          kahan2(s3, c3, h3 ? pr.x : pr.y);
          kahan2(sR, cR, (h1 || h2 || h3) ? pr.y : pr.x);
          n1 += h1 ? 1u : 0u; n2 += (!h1 && h2) ? 1u : 0u; n3 += (!h1 && !h2 && h3) ? 1u : 0u; nR += (h1 || h2 || h3) ? 0u : 1u;
        }
      }
    }
    // ---- call: the unanimous gate; what it does not answer, here (k_call_full's arrangement of the chains by base, call_full, its `finish`) ----
    const uint32_t depth = n1 + n2 + n3 + nR;
    bool resolved = true;
    uint32_t q_call = FGX_MIN_PHRED, code_call = 15, err = 0;
    if (incol) {
      if (b2 != 0) resolved = false;                         // two or more distinct bases: never the unanimous fast path
      else if (n1 != 0) {
        uint32_t qq = 0;
        CallConst KC;
        KC.cap = sT.cap; KC.cap_threshold = sT.cap_threshold; KC.half_cerr_at_cap = sT.half_cerr_at_cap;
        resolved = unanimous_call_lds(sT, P.T->t.cerr_min, KC, s1, sR, &qq);
        if (resolved) { q_call = qq; code_call = b1; }
      }
      if (!resolved) {
        double ll[4];
        uint32_t hit = 0;                                    // observations of the called base
        uint32_t obk[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
          const uint32_t code = 1u << k;
          ll[k] = code == b1 ? s1 : code == b2 ? s2 : code == b3 ? s3 : sR;
          obk[k] = code == b1 ? n1 : code == b2 ? n2 : code == b3 ? n3 : nR;
        }
        int bi;
        uint8_t q;
        call_full(P.T->t, ll, &bi, &q);
        hit = bi == 0 ? obk[0] : bi == 1 ? obk[1] : bi == 2 ? obk[2] : bi == 3 ? obk[3] : 0u;
        code_call = bi >= 0 ? 1u << bi : 15u; q_call = q; err = depth - hit;
      }
      uint8_t ob, oq;
      if (depth < P.min_reads) { ob = 15; oq = 0; }
      else if (q_call < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; }
      else { ob = (uint8_t)code_call; oq = (uint8_t)q_call; }
      fam_code[oc] = ob; fam_qual[oc] = oq; fam_err[oc] = (uint16_t)err; fam_depth[oc] = (uint16_t)depth;   // (at most WIDE_MAX: no clamp to apply)
      lmax = depth; lmin = depth;
    }
  }
  lmax = uni(wave_max(lmax)); lmin = uni(wave_min(lmin));
  if (lane == 0) D.item_depth[item] = make_uint2(lmax, lmin);
}

// -----------------------------------------------------------------------------------------------------------------------------
// k_wide_finish — wavefront = family: consensus UMI, depth extremes, record sizes, counters (k_deep_cols's tail)
// -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_wide_finish(FastParams P, WideParams D) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t li = blockIdx.x * (blockDim.x >> 6) + wv;
  if (li >= D.n_list) return;
  const DeepFam* const Fp = &D.fams[li];
  if (uni(Fp->status) != 1u) return;
  const uint32_t g = uni(D.list[li]);
  const uint32_t n = uni(Fp->n), ne = uni(Fp->ne), type_a = uni(Fp->type_a);
  const uint32_t m_k[2] = {uni(Fp->m_a), uni(Fp->m_b)}, lc_k[2] = {uni(Fp->lc_a), uni(Fp->lc_b)};
  const uint32_t rxc_k[2] = {uni(Fp->rx_cnt_a), uni(Fp->rx_cnt_b)}, rxl_k[2] = {uni(Fp->rx_len_a), uni(Fp->rx_len_b)};
  const DeepRow* const rows = D.rows + uni(Fp->row0);
  const uint32_t slot0 = 3 * g;
  const uint8_t* const blob = P.blob;
  typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
  typedef const FGX_CONST_AS u32x8* RowPtr;
  auto row_seq = [&](const u32x8& r) { return blob + (((unsigned long long)r[1] << 32) | r[0]); };

  // ---- consensus UMI per end (simple_umi.rs:46-117): lane = character; the counts are words, an unresolved character is called here ----
  const DeviceTables* TU = P.TU;
  char my_rx[2] = {0, 0};
  bool rx_bad = false;
  uint32_t row_base = 0;
#pragma unroll 1
  for (uint32_t k = 0; k < ne; k++) {
    const uint32_t m = m_k[k], rx_cnt = rxc_k[k], ulen = rxl_k[k];
    const RowPtr er = (RowPtr)(rows + row_base);
    row_base += m;
    if (rx_cnt == 0) continue;
    const bool mychar = lane < ulen;
    ColumnAcc acc;
    acc.reset();
    uint32_t non_dna = 0, seenu = 0;
    uint8_t fc = 0;
    bool mixed = false, all_same = true;
    const double uc = TU->t.correct[20], ue = TU->t.error_per_alt[20];
    for (uint32_t j = 0; j < m; j++) {
      const u32x8 R = er[uni(j)];
      if (!((R[7] >> 17) & 1u)) continue;                    // (uniform: the read carries no RX)
      const uint8_t ch = mychar ? row_seq(R)[(R[7] & 0xFFFFu) + lane] : (uint8_t)'A';
      if (seenu == 0) fc = ch;
      else if (ch != fc) all_same = false;
      seenu++;
      const uint8_t up = (ch >= 'a' && ch <= 'z') ? (uint8_t)(ch - 32) : ch;
      const bool dna = up == 'A' || up == 'C' || up == 'G' || up == 'T' || up == 'N';
      if (dna) { const int bl = bam::ascii_to_lane(ch); if (bl != 255) acc.add(bl, uc, ue); }
      else { non_dna++; if (ch != fc) mixed = true; }
    }
    if (rx_cnt == 1) { if (mychar) my_rx[k] = (char)fc; }    // one read = its bytes
    else if (!__any(mychar && !all_same)) {                  // every retained read carries the same value: normalised (A C G T N upper case)
      if (mychar) { const uint32_t ch = fc, up = ch & 0xDFu, idx = up - 'A'; const bool dna = idx < 26 && ((0x00082045u >> idx) & 1u); my_rx[k] = (char)(dna ? up : ch); }
    } else if (mychar) {
      if (non_dna == 0) {
        int bi; uint8_t q;
        CallConst KU;
        KU.cap = TU->t.cap; KU.cap_threshold = TU->t.cap_threshold; KU.half_cerr_at_cap = TU->t.half_cerr_at_cap;
        if (!column_call_fast_lds(TU->t, KU, acc.s, acc.obs, &bi, &q)) call_full(TU->t, acc.s, &bi, &q);
        my_rx[k] = bi >= 0 ? "ACGT"[bi] : 'N';
      } else if (non_dna == seenu && !mixed) my_rx[k] = (char)fc;
      else rx_bad = true;
    }
  }
  if (__any(rx_bad)) {                                       // the general path redoes the family (nothing was counted, no record size is set)
    if (lane == 0) { const uint32_t kk = atomicAdd(P.n_deferred, 1u); P.deferred[kk] = g; }
    return;
  }
  // ---- the items' depth extremes: end A's passes, then end B's --------------------------------------------------------------------
  uint32_t maxd[2] = {0, 0}, mind[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
  {
    const uint32_t it0 = uni((uint32_t)D.pass0[li]);
    uint32_t base = 0;
    for (uint32_t k = 0; k < ne; k++) {
      const uint32_t np = (lc_k[k] + 63u) >> 6;
      uint32_t mx = 0, mn = 0xFFFFFFFFu;
      for (uint32_t i = lane; i < np; i += 64) { const uint2 d = D.item_depth[it0 + base + i]; mx = d.x > mx ? d.x : mx; mn = d.y < mn ? d.y : mn; }
      maxd[k] = uni(wave_max(mx)); mind[k] = uni(wave_min(mn));
      base += np;
    }
  }
  // ---- record sizes (vanilla_caller.rs:1767-1881), counters ----------------------------------------------------------------------
  for (uint32_t k = 0; k < ne; k++) {
    const uint32_t e = k == 0 ? type_a : 2u, slot = slot0 + e, Lc = lc_k[k];
    EndDesc* const E = &P.ends[slot];
    if (lane < rxl_k[k] && rxc_k[k]) E->rx[lane] = my_rx[k];
    if (lane == 0) {
      const uint32_t mi_len = E->mi_len, nm = P.prefix_len + 1 + mi_len;
      const uint32_t mx = Lc ? maxd[k] : 0u, mn = Lc ? mind[k] : 0u;
      const uint32_t size = 32 + nm + 1 + (Lc + 1) / 2 + Lc + (3 + P.rg_len + 1) + (3 + int_tag_width(mx)) + (3 + int_tag_width(mn)) + 7 +
                            (P.per_base_tags ? 2 * (8 + 2 * Lc) : 0) + (3 + mi_len + 1) + (E->has_cb ? 3 + E->cb_len + 1 : 0) + (E->has_rx ? 3 + E->rx_len + 1 : 0);
      E->rec_size = size; E->valid = 1;
      P.rec_sizes[slot] = (uint64_t)size + 4;
    }
  }
  if (lane == 0) {
    unsigned long long* st = P.stats + (size_t)(blockIdx.x & (STAT_SLOTS - 1)) * 32;
    const uint32_t s_insuf = Fp->rej_insuf, s_zero = Fp->rej_zero, s_orphan = Fp->rej_orphan, s_down = Fp->rej_down;
    const uint32_t ov_agree = Fp->ov_agree, ov_dis = Fp->ov_dis, ov_corr = Fp->ov_corr;
    atomicAdd(&st[0], (unsigned long long)n);
    if (ne) atomicAdd(&st[1], (unsigned long long)ne);
    if (s_insuf + s_zero + s_orphan + s_down) atomicAdd(&st[2], (unsigned long long)(s_insuf + s_zero + s_orphan + s_down));
    if (s_insuf) atomicAdd(&st[3 + FGX_REJ_INSUFFICIENT_READS], (unsigned long long)s_insuf);
    if (s_zero) atomicAdd(&st[3 + FGX_REJ_ZERO_LENGTH_AFTER_TRIMMING], (unsigned long long)s_zero);
    if (s_orphan) atomicAdd(&st[3 + FGX_REJ_ORPHAN_CONSENSUS], (unsigned long long)s_orphan);
    if (s_down) atomicAdd(&st[3 + FGX_REJ_DOWNSAMPLED], (unsigned long long)s_down);
    if (ov_agree + ov_dis) atomicAdd(&st[24], (unsigned long long)(ov_agree + ov_dis));
    if (ov_agree) atomicAdd(&st[25], (unsigned long long)ov_agree);
    if (ov_dis) atomicAdd(&st[26], (unsigned long long)ov_dis);
    if (ov_corr) atomicAdd(&st[27], (unsigned long long)ov_corr);
  }
}
