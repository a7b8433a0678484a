// codec_deep.inc — deep CODEC molecules (65 .. CODEC_DEEP_MAX records): k_codec_deep_parse (a workgroup per molecule, thread = record) + k_codec_deep_cols
// (a wavefront per molecule, lane = column, the member reads of the two single-strand read sets STREAMED from global memory).  Included by fastpath.hip
// inside `namespace fgx { namespace {` after duplex_deep.inc; it shares simplex_deep.inc's DeepRow / DeepLds / deep_parse_records / k_deep_sizes and
// fastpath.hip's ChainAcc / column_call_fast_lds / push_full_global, as duplex_deep.inc does.
//
// Why: k_family_wave<2> holds a molecule in one wavefront — a lane per record, the records in an LDS slice — and defers what has more than 64 records to
// the general path (codec_host.cpp).  Nothing of a CODEC molecule's column phase needs the tile: the two read sets are streamed as a duplex molecule's four.
//
//   k_codec_deep_parse   phases 2 and 5C of k_family_wave<2> for a workgroup: the record shape through deep_parse_records (a primary record with one M/=/X
//                        op over l_seq, pos and l_seq inside the closed form's ranges, qualities present, the first record's MI and read-name length rule)
//                        and the CODEC rules on top — every record paired, the mate position inside the closed form's range, exactly two records per read
//                        name, mates adjacent (records 2k and 2k + 1), exactly one of them FIRST, the names verified and not only their hashes —, then per
//                        template is_primary_fr_pair_raw (NotPrimaryFrPair), the overlap clip against the mate in hand, the clipped length and the adjusted
//                        start, the cmin_reads gate, the equal-length rule per strand, --max-reads-per-strand (the CAP builds), the longest R1 / R2, the
//                        geometry checks (InsufficientOverlap, IndelErrorBetweenStrands, ClipOverlapFailed), one DeepRow per surviving read (set 0 = R1s,
//                        set 1 = R2s, file order), the list of the RX values of EVERY record in file order, and the molecule's descriptor.
//                        Reference: codec_caller.rs:625-1004, 1006-1072; overlap.rs:21-108, 223-357; cigar.rs:461-500.
//   k_codec_deep_cols    per set and 64-column pass the rows in file order, four at a time; Kahan chains by order of appearance (ChainAcc), the unanimous
//                        gate (column_call_fast_lds) or an item for k_call_full; the single-strand caller's rules for CODEC (min_reads 1, minimum consensus
//                        base quality 0); col_code / col_qual / col_depth / col_err at col_base and col_base + len1; a set of one read through the
//                        single-read quality table.  Then 7C and 8C of k_family_wave<2>: the consensus UMI over every record of the molecule that carries
//                        RX, the CodecDesc, rec_size and rec_sizes.  The record writers (k_emit_codec_fast, k_emit_codec) take the descriptor as they
//                        take k_family_wave<2>'s.
//
// A CODEC source read has none of the simplex source-read rules (codec_caller.rs:504-568): no masking of qualities below min_input_base_quality, no
// trailing-N strip, no overlapping-bases pre-correction.  Its length is the clipped length, a reverse read is indexed from l_seq - 1 down.  So the rows
// carry no shared span with a mate (wc = 0: the column loop has no correction step at all), the final length is the clipped length as it is, and the column
// loop does not look at min_input_bq.  deep_parse_records' MC-derived clip is not used.
//
// The bound.  A molecule holds at most CODEC_DEEP_MAX = 254 records (127 templates).  What fixes it is a byte, three times over:
//   * an observation count of a column is a byte of FullItem::obs (fastpath.h), and k_emit_codec_fast writes a strand's per-base depth and error count
//     (ad bd ae be) as one byte with a zero above it — a strand holds at most 127 reads;
//   * cD / cM are the two strands' depths added, at most 254, with aD aM bD bM below them: every integer tag of the record is ONE value byte wide (type c
//     up to 127, C above: int_tag_byte, record_writers.inc) — what FieldWriterFlat::scalars writes and the `3 * (4 + 4 + 7)` term of the record size assumes;
//   * a consensus UMI character counts every record of the molecule that carries RX — at most 254, whatever a cap leaves for the columns: its four counts
//     are bytes of an item too.  So a --max-reads-per-strand does not move the bound.
// No tighter byte was found: col_depth and col_err are 16 bits wide, the descriptor's lengths are 16 bits or more.
//
// --max-reads-per-strand (the CAP builds k_codec_deep_parse<NT, MAXR, 1>, launched in place of the others for a caller with a cap > 0, as k_family_wave<2, 0, 1>
// is): after the min-reads gate the R1 list and the R2 list each keep their `cap` lowest fgbio name ranks (as int32_t, ties in file order); the survivors
// stay in file order, what is dropped is counted as Downsampled, and everything downstream sees the survivors only — except the consensus UMI.  A cap of 0
// rejects the strand reads as InsufficientReads.  A molecule the cap does not bite runs none of it.  The column kernel has one build: it sees survivors' rows.
//
// Outside the shape — the molecule leaves for the deferred list, as it did from k_family_wave<2>: more than CODEC_DEEP_MAX records, an indel or a clip (more
// than one CIGAR op), a secondary or supplementary record, a fragment, an unmapped read, absent qualities, an MC the closed form does not read
// (deep_parse_records' rule; k_family_wave<2> does not look at MC), singletons, triples, interleaved mates, both mates FIRST or neither, unequal read lengths
// within a strand, a cap that bites in a build without it, prp + rl_n < nrp, RX of unequal length or above FAST_RX_CAP, an IUPAC code in a lone read, an
// overflow of the FullItem pool.  The host launches nothing of this under --trim, --rejects or in the canonical second pass, and only under FGX_CODEC_DEEP=1.

constexpr uint32_t CODEC_DEEP_MAX = 254;   // records of a molecule (see "The bound" above)
static_assert(CODEC_DEEP_MAX / 2 <= 255, "a strand's observation counts are bytes (FullItem::obs, the per-base depths of k_emit_codec_fast)");
static_assert(CODEC_DEEP_MAX <= 255, "cD = the two strands' depths added and the consensus UMI's counts over every record are one byte wide");
static_assert(CODEC_DEEP_MAX % 2 == 0 && CODEC_DEEP_MAX <= 256, "whole templates; a molecule at the bound fits the record kernel's arrays");

struct CodecDeepMol {       // 64 bytes: what k_codec_deep_parse hands to k_codec_deep_cols
  uint32_t status;          // 0: not this path's (on the deferred list); 1: decided by the gates, counters only; 2: the column kernel decides
  uint32_t n, row0;         // records; first DeepRow (set 0's rows, then set 1's; file order inside a set) and first entry of the RX list
  uint16_t m[2];            // surviving R1s / R2s
  uint16_t len[2];          // length of a set: its longest clipped read
  uint32_t cons_len;
  uint32_t n_notfr, rj_insuf, rj_overlap, rj_indel, rj_clipfail, rj_down;   // NotPrimaryFrPair; what a gate rejected; what the cap dropped
  uint32_t fc;              // the record the cell barcode comes from, index inside the molecule
  uint16_t mi_off, cb_off;  // the first record's MI value and record fc's cell barcode: offsets inside the record body
  uint8_t mi_len, cb_len, has_cb, neg;   // neg: bit 0 the longest R1 is on the reverse strand, bit 1 the longest R2
  uint16_t rx_cnt;          // records that carry RX (entries of the RX list)
  uint8_t ulen, capped;     // their common RX length; the cap dropped a read
};
static_assert(sizeof(CodecDeepMol) == 64, "CODEC deep descriptor");

struct CodecDeepParams {
  const uint32_t* list; uint32_t n_list;     // the molecules of more than 64 records
  const uint64_t* row0;                      // per list entry: first DeepRow / RX entry (exclusive scan of the record counts)
  DeepRow* rows; CodecDeepMol* mols;         // mols: per list entry
  unsigned long long* umi;                   // blob offset of the RX value of every record that carries one, file order, at the molecule's row0
  uint32_t* n_done;                          // molecules these kernels decided (fgx_debug_last_codec_deep); [1]: of which the cap dropped a read
};

template <uint32_t MAXR>
struct CodecDeepLds : DeepLds<MAXR> {
  uint32_t adj[MAXR];                    // adjusted 1-based start of the clipped read (pos < 2^30 and a clip <= 65 535: 32 bits hold it)
  uint8_t cf[MAXR];                      // bit 0: is_fr_pair_raw of THIS record; bit 1: its MATE_UNMAPPED flag
  uint8_t sv[MAXR];                      // 0: not an FR template's read; 1: a strand read; 2: a strand read the cap dropped
  uint32_t bad_rule, bad_len;            // (a flag per phase: no thread sets one that another may still be reading for the phase before)
  uint32_t c_notfr, c_set[2], c_first[2], c_long[2], c_cb[2];
  uint32_t c_rx, c_rxmin, c_rxmax;
  uint32_t mi_rel, mi_len;               // the first record's MI value
};

// <NT, MAXR>: <128, 128> takes the listed molecules of up to 128 records, <256, 256> the larger ones — both are launched over the whole list and a workgroup
// whose molecule is the other build's returns at once, as in duplex_deep.inc.  Every loop with a barrier behind it has a workgroup-uniform trip count, and
// every early exit is decided from LDS words all threads read alike behind a barrier.
template <uint32_t NT, uint32_t MAXR, int CAP = 0>
__global__ __launch_bounds__(NT) void k_codec_deep_parse(FastParams P, CodecDeepParams D) {
  static_assert((MAXR == 128 || MAXR == 256) && CODEC_DEEP_MAX <= 256, "the two builds");
  __shared__ CodecDeepLds<MAXR> S;
  __shared__ __align__(16) uint8_t sTagCls[256];
  const uint32_t tid = threadIdx.x;
  const uint32_t li = blockIdx.x;
  const uint32_t g = D.list[li];
  const uint32_t r0 = P.grp_first[g], n = P.grp_first[g + 1] - r0;
  if (MAXR == 128 ? n > 128u : n <= 128u) return;            // the other build's (uniform; ahead of every barrier)
  CodecDeepMol* const M = &D.mols[li];
  fill_tag_classes(sTagCls);
  if (tid == 0) {
    S.bad = 0; S.bad_rule = 0; S.bad_len = 0; S.c_notfr = 0; S.c_rx = 0; S.c_rxmin = 0xFFFFFFFFu; S.c_rxmax = 0; S.mi_rel = 0; S.mi_len = 0;
    for (int k = 0; k < 2; k++) { S.c_set[k] = 0; S.c_first[k] = 0xFFFFFFFFu; S.c_long[k] = 0; S.c_cb[k] = 0xFFFFFFFFu; }
  }
  auto leave = [&]() { if (tid == 0) { M->status = 0; const uint32_t k = atomicAdd(P.n_deferred, 1u); P.deferred[k] = g; } };
  if (tid < 3) { P.cends[3 * g + tid].valid = 0; P.rec_sizes[3 * g + tid] = 0; }
  if (n > CODEC_DEEP_MAX || (n & 1u)) { leave(); return; }   // above the bound; an odd count holds a singleton
  __syncthreads();

  // ---- 1. parse: thread = record (k_simplex_wave2's record shape; an unmapped record is not in it here: a CODEC template needs both positions) ---------------
  deep_parse_records<0>(P, S, S, r0, n, tid, NT, sTagCls, false);
  __syncthreads();
  if (S.bad) { leave(); return; }

  // ---- 2. the CODEC rules of k_family_wave<2> phase 2 and the templates of 5C: every record paired, the mate's position in the closed form's range,
  //         is_fr_pair_raw of THIS record (overlap.rs:21-69); exactly two records per name, adjacent, one of them FIRST ----------------------------------------
  for (uint32_t r = tid; r < n; r += NT) {
    const uint8_t* const rec = P.blob + S.off[r];
    const uint32_t b = S.bits[r], flags = gld32(rec + 12) >> 16, l_seq = S.l_seq[r];
    const int32_t mref = (int32_t)gld32(rec + 20), mpos = (int32_t)gld32(rec + 24), pos = S.pos[r];
    bool bad = (b & 3u) == 0u || mpos < -1 || mpos >= record::POS_LIMIT;                 // a fragment; (pos itself: deep_parse_records)
    const bool rv = (b & 4u) != 0, mrv = (flags & bam::F_MATE_REVERSE) != 0, mu = (flags & bam::F_MATE_UNMAPPED) != 0;
    const bool okp = !mu && S.ref_id[r] == mref && rv != mrv;
    const bool frself = okp && ((long long)mpos + 1 < (long long)pos + 1 + ((long long)l_seq - 1));
    S.cf[r] = (uint8_t)((frself ? 1u : 0u) | (mu ? 2u : 0u));
    const uint32_t ka = S.key[r] >> 2, nl = S.name_len[r];
    const uint8_t* const na = rec + 32;
    uint32_t n_same = 0;
    bool neighbour = false;
    for (uint32_t j = 0; j < n; j++) {
      if (j == r || (S.key[j] >> 2) != ka || S.name_len[j] != nl) continue;
      const uint8_t* const nb = P.blob + S.off[j] + 32;
      bool same = true;
      for (uint32_t i = 0; i < nl && same; i += 8) {
        unsigned long long wa = gld64(na + i), wb = gld64(nb + i);
        if (i + 8 > nl) { const unsigned long long mk = (1ULL << (8 * (nl - i))) - 1; wa &= mk; wb &= mk; }
        if (wa != wb) same = false;
      }
      if (same) { n_same++; neighbour |= j == (r ^ 1u); }
    }
    // singletons, triples, interleaved pairs; both mates FIRST or neither: the general path's
    if (n_same != 1 || !neighbour) bad = true;
    else if (((b & 3u) == 1u) == ((S.bits[r ^ 1u] & 3u) == 1u)) bad = true;
    if (bad) S.bad_rule = 1;
    if (r == 0) {   // the first record's MI value (deep_parse_records checked that it is there and gives a legal read name; it keeps no MI)
      const uint32_t aux_off = (uint32_t)S.seq_rel[0] + ((l_seq + 1u) >> 1) + l_seq;
      AuxTags ax;
      aux_walk(rec, sTagCls, aux_off, P.rec_len[r0] - aux_off, P, ax);
      const record::TagFields tg = record::unpack_tags(ax);
      S.mi_rel = tg.mi_lo; S.mi_len = tg.mi_len;
    }
  }
  __syncthreads();
  if (S.bad_rule) { leave(); return; }

  // ---- 3. per template is_primary_fr_pair_raw (overlap.rs:83-108), the overlap clip against the mate in hand (overlap.rs:223-357 for two single-M
  //         alignments), ClippedRecordInfo (codec_caller.rs:1006-1040): the clipped length, and a reverse read loses its start and moves right -------------------
  for (uint32_t r = tid; r < n; r += NT) {
    const uint32_t mt = r ^ 1u, b = S.bits[r], mb = S.bits[mt], cf = S.cf[r], mcf = S.cf[mt], l_seq = S.l_seq[r];
    const bool first = (b & 3u) == 1u, rev = (b & 4u) != 0, m_rev = (mb & 4u) != 0;
    const bool fr = !(cf & 2u) && !(mcf & 2u) && S.ref_id[r] == S.ref_id[mt] && rev != m_rev && (((rev ? cf : mcf) & 1u) != 0);
    uint32_t clip = 0;
    if (fr) clip = record::single_m_overlap_clip(rev, S.pos[r], (int32_t)l_seq, S.pos[mt], (int32_t)S.l_seq[mt]);   // (both records inside the closed form's ranges)
    const uint32_t clen = fr ? (l_seq > clip ? l_seq - clip : 0u) : 0u;
    S.adj[r] = (uint32_t)(S.pos[r] + 1) + (rev ? (clip < l_seq ? clip : l_seq) : 0u);
    S.final_len[r] = (uint16_t)clen;
    S.sv[r] = fr ? 1 : 0;
    if (!fr) atomicAdd(&S.c_notfr, 1u);
    else { const uint32_t k = first ? 0u : 1u; atomicAdd(&S.c_set[k], 1u); atomicMin(&S.c_first[k], r); }
  }
  __syncthreads();

  // ---- 4. the gates (every thread decides the same from LDS) ---------------------------------------------------------------------------------------------------
  const uint32_t n_notfr = S.c_notfr, n1 = S.c_set[0], n2 = S.c_set[1], n_strand = n1 + n2;
  // a molecule the gates decide: counters only (status 1); `what`: 0 nothing, 1 InsufficientReads, 2 InsufficientOverlap, 3 IndelErrorBetweenStrands, 4 ClipOverlapFailed
  auto decided = [&](uint32_t what, uint32_t n_reads, uint32_t rj_down) {
    if (tid == 0) {
      CodecDeepMol f;
      __builtin_memset(&f, 0, sizeof(f));
      f.status = 1; f.n = n; f.n_notfr = n_notfr; f.rj_down = rj_down; f.capped = rj_down ? 1 : 0;
      if (what == 1) f.rj_insuf = n_reads; else if (what == 2) f.rj_overlap = n_reads; else if (what == 3) f.rj_indel = n_reads; else if (what == 4) f.rj_clipfail = n_reads;
      *M = f;
    }
  };
  if (n1 == 0) { decided(0, 0, 0); return; }
  if (n1 < P.cmin_reads) { decided(1, n_strand, 0); return; }
  // most common alignment: with one M op per read the simplified clipped CIGAR is (M, l_seq) — equal read lengths make one group; otherwise the general path
  {
    const uint32_t l1ref = S.l_seq[S.c_first[0]], l2ref = n2 ? S.l_seq[S.c_first[1]] : 0u;
    for (uint32_t r = tid; r < n; r += NT)
      if (S.sv[r] && S.l_seq[r] != (((S.bits[r] & 3u) == 1u) ? l1ref : l2ref)) S.bad_len = 1;
  }
  __syncthreads();
  if (S.bad_len) { leave(); return; }
  // --max-reads-per-strand (codec_caller.rs:765-802, cap_infos_to_lowest_ranking :1060-1072; k_family_wave<2, 0, 1> restates it for a wavefront): the R1
  // list and the R2 list each keep their `cap` lowest name ranks, ties in file order.  `key` is done with as the pairing hash: it holds the ranks.
  // (Workgroup-uniform: n1, n2 and the cap are the same in every thread; a molecule the cap does not bite runs nothing of this.)
  uint32_t m1 = n1, m2 = n2, rj_down = 0;
  if (P.cmax_reads >= 0) {
    if (P.cmax_reads == 0) { decided(1, n_strand, 0); return; }
    if ((long long)n1 > P.cmax_reads || (long long)n2 > P.cmax_reads) {
      if constexpr (CAP == 0) { leave(); return; }             // (the launch pairs a cap with the CAP builds; if this build ever sees one, the general path decides)
      else {
        const uint32_t cap = (uint32_t)P.cmax_reads;
        for (uint32_t r = tid; r < n; r += NT)
          if (S.sv[r]) S.key[r] = (uint32_t)name_rank(P.blob + S.off[r] + 32, S.name_len[r]);
        __syncthreads();
        for (uint32_t r = tid; r < n; r += NT) {
          if (!S.sv[r]) continue;
          const uint32_t ty = S.bits[r] & 3u;
          const int32_t rk = (int32_t)S.key[r];
          uint32_t before = 0;
          for (uint32_t j = 0; j < n; j++) {                   // (sv != 0: a read of the list, dropped by now or not)
            if (!S.sv[j] || (S.bits[j] & 3u) != ty) continue;
            const int32_t rj = (int32_t)S.key[j];
            before += (rj < rk || (rj == rk && j < r)) ? 1u : 0u;
          }
          if (before >= cap) { S.sv[r] = 2; atomicAdd(&S.c_set[ty == 1u ? 0 : 1], 0xFFFFFFFFu); }   // (one fewer)
        }
        __syncthreads();
        m1 = S.c_set[0]; m2 = S.c_set[1];
        rj_down = n_strand - (m1 + m2);
      }
    }
  }
  if (m1 == 0 || m2 == 0) { leave(); return; }                 // (not reachable: a template gives one read to each list, and a cap leaves at least one)
  const uint32_t n_surv = m1 + m2;

  // ---- 5. the longest R1 / R2 by clipped reference length (first maximum), the cell barcode's record (first record, R1s then R2s, that carries a non-empty
  //         value, :1708-1722), the records that carry RX (EVERY record of the molecule, :1725-1744) --------------------------------------------------------------
  for (uint32_t r = tid; r < n; r += NT) {
    const uint32_t b = S.bits[r];
    if (S.sv[r] == 1) {
      const uint32_t k = (b & 3u) == 1u ? 0u : 1u;
      atomicMax(&S.c_long[k], (((uint32_t)S.final_len[r] + 1u) << 8) | (255u - r));
      if ((b & 16u) && S.cb_len[r] > 0) atomicMin(&S.c_cb[k], r);
    }
    if (b & 8u) { atomicAdd(&S.c_rx, 1u); atomicMin(&S.c_rxmin, (uint32_t)S.rx_len[r]); atomicMax(&S.c_rxmax, (uint32_t)S.rx_len[r]); }
  }
  __syncthreads();
  const uint32_t L1 = 255u - (S.c_long[0] & 255u), L2 = 255u - (S.c_long[1] & 255u);
  const bool r1_neg = (S.bits[L1] & 4u) != 0, r2_neg = (S.bits[L2] & 4u) != 0;
  const uint32_t Lp = r1_neg ? L2 : L1, Ln = r1_neg ? L1 : L2;
  const unsigned long long adj_p = S.adj[Lp], adj_n = S.adj[Ln], adj_1 = S.adj[L1], adj_2 = S.adj[L2];
  const uint32_t rl_p = S.final_len[Lp], rl_n = S.final_len[Ln], rl_1 = S.final_len[L1], rl_2 = S.final_len[L2];
  const unsigned long long pos_end = adj_p + (rl_p ? rl_p - 1 : 0), neg_end = adj_n + (rl_n ? rl_n - 1 : 0);
  const unsigned long long ov_s = adj_n > adj_p ? adj_n : adj_p, ov_e = pos_end < neg_end ? pos_end : neg_end;
  const long long duplex_len = (long long)ov_e - (long long)ov_s + 1;
  if (duplex_len < (long long)P.cmin_duplex_len) { decided(2, n_surv, rj_down); return; }
  // read_pos_at_ref_pos_raw (cigar.rs:461-500) on [H?] M [H?]: 1-based query position, 0 = htsjdk's out-of-range sentinel
  auto read_pos = [](unsigned long long a, uint32_t rl, unsigned long long p) -> long long { return (p >= a && rl && p <= a + rl - 1) ? (long long)(p - a + 1) : 0; };
  if (read_pos(adj_1, rl_1, ov_s) - read_pos(adj_2, rl_2, ov_s) != read_pos(adj_1, rl_1, ov_e) - read_pos(adj_2, rl_2, ov_e)) { decided(3, n_surv, rj_down); return; }
  const long long prp = read_pos(adj_p, rl_p, ov_e), nrp = read_pos(adj_n, rl_n, ov_e);
  if (prp == 0 || nrp == 0) { decided(3, n_surv, rj_down); return; }
  if (prp + (long long)rl_n < nrp) { leave(); return; }                          // the general path raises the error
  const uint32_t cons_len = (uint32_t)(prp + (long long)rl_n - nrp);
  const uint32_t len1 = rl_1, len2 = rl_2;                                        // (the longest read IS the set's length)
  if (cons_len < len1 || cons_len < len2) { decided(4, n_surv, rj_down); return; }
  // the consensus UMI's reads: RX of unequal length or above FAST_RX_CAP is the general path's (7C)
  const uint32_t rx_cnt = S.c_rx, ulen = rx_cnt ? S.c_rxmin : 0u;
  if (rx_cnt && (S.c_rxmin != S.c_rxmax || ulen > (uint32_t)FAST_RX_CAP)) { leave(); return; }

  // ---- 6. member rows — the surviving R1s, then the surviving R2s, file order inside a set — and the RX list ------------------------------------------------
  const unsigned long long row0 = D.row0[li];
  for (uint32_t r = tid; r < n; r += NT) {
    const uint32_t b = S.bits[r];
    const bool mine = S.sv[r] == 1, hrx = (b & 8u) != 0;
    if (!mine && !hrx) continue;
    const uint32_t ty = b & 3u;
    uint32_t rank = 0, urank = 0;
    for (uint32_t j = 0; j < r; j++) { rank += (S.sv[j] == 1 && (S.bits[j] & 3u) == ty) ? 1u : 0u; urank += (S.bits[j] & 8u) ? 1u : 0u; }
    const unsigned long long so = S.off[r] + S.seq_rel[r];
    if (hrx) D.umi[row0 + urank] = S.off[r] + S.rx_rel[r];
    if (mine) {
      DeepRow R;   // (no mate, no shared span: w[2,3] repeat the read, wo = mo = wc = 0)
      R.w[0] = (uint32_t)so; R.w[1] = (uint32_t)(so >> 32); R.w[2] = R.w[0]; R.w[3] = R.w[1];
      R.w[4] = (uint32_t)S.l_seq[r] | ((uint32_t)S.final_len[r] << 16);
      R.w[5] = (uint32_t)S.l_seq[r]; R.w[6] = 0;
      R.w[7] = ((hrx ? (uint32_t)S.rx_rel[r] - (uint32_t)S.seq_rel[r] : 0u) & 0xFFFFu) | ((((b & 4u) ? 1u : 0u) | (hrx ? 2u : 0u)) << 16) | ((uint32_t)S.rx_len[r] << 24);
      D.rows[row0 + (ty == 1u ? 0u : m1) + rank] = R;
    }
  }

  // ---- 7. the molecule's descriptor ---------------------------------------------------------------------------------------------------------------------------
  if (tid == 0) {
    CodecDeepMol f;
    __builtin_memset(&f, 0, sizeof(f));
    f.status = 2; f.n = n; f.row0 = (uint32_t)row0;
    f.m[0] = (uint16_t)m1; f.m[1] = (uint16_t)m2; f.len[0] = (uint16_t)len1; f.len[1] = (uint16_t)len2; f.cons_len = cons_len;
    f.n_notfr = n_notfr; f.rj_down = rj_down; f.capped = rj_down ? 1 : 0;
    const uint32_t c1 = S.c_cb[0], c2 = S.c_cb[1];
    const bool any_cb = P.cell0 && (c1 != 0xFFFFFFFFu || c2 != 0xFFFFFFFFu);
    const uint32_t fc = c1 != 0xFFFFFFFFu ? c1 : c2 != 0xFFFFFFFFu ? c2 : 0u;
    f.fc = fc; f.has_cb = any_cb ? 1 : 0; f.cb_off = S.cb_rel[fc]; f.cb_len = S.cb_len[fc];
    f.mi_off = (uint16_t)S.mi_rel; f.mi_len = (uint8_t)S.mi_len;
    f.neg = (uint8_t)((r1_neg ? 1u : 0u) | (r2_neg ? 2u : 0u));
    f.rx_cnt = (uint16_t)rx_cnt; f.ulen = (uint8_t)ulen;
    *M = f;
  }
}

// -----------------------------------------------------------------------------------------------------------------------------
// k_codec_deep_cols — wavefront = molecule, lane = column, rows streamed from global memory
// -----------------------------------------------------------------------------------------------------------------------------
#ifndef FGX_CODEC_DEEP_OCC
#define FGX_CODEC_DEEP_OCC 8
#endif
__global__ __launch_bounds__(256, FGX_CODEC_DEEP_OCC) void k_codec_deep_cols(FastParams P, CodecDeepParams D) {
  __shared__ __align__(16) FwLds sL;
  ConsensusTables& sT = sL.t;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  {
    constexpr uint32_t IMG_V = (uint32_t)(sizeof(FwLds) / 16);
    const u32x4* const src = (const u32x4*)P.fw_image;
    u32x4* const dst = (u32x4*)&sL;
    for (uint32_t i = threadIdx.x; i < IMG_V; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  const uint32_t li = blockIdx.x * (blockDim.x >> 6) + wv;
  if (li >= D.n_list) return;
  const CodecDeepMol* const Mp = &D.mols[li];
  const uint32_t status = uni(Mp->status);
  if (status == 0u) return;
  const uint32_t g = uni(D.list[li]);
  const uint32_t n = uni(Mp->n), n_notfr = uni(Mp->n_notfr), rj_down = uni(Mp->rj_down);
  const uint32_t r0 = uni(P.grp_first[g]);
  const uint32_t slot = 3 * g + 1;
  unsigned long long* const st = P.stats + (size_t)(blockIdx.x & (STAT_SLOTS - 1)) * 32;
  uint32_t s_cons = 0;
  auto flush_stats = [&]() {
    if (lane == 0) {
      const uint32_t rj_insuf = Mp->rj_insuf, rj_overlap = Mp->rj_overlap, rj_indel = Mp->rj_indel, rj_clipfail = Mp->rj_clipfail;
      const uint32_t s_filtered = n_notfr + rj_down + rj_insuf + rj_overlap + rj_indel + rj_clipfail;
      atomicAdd(&st[0], (unsigned long long)n);
      if (s_cons) atomicAdd(&st[1], (unsigned long long)s_cons);
      if (s_filtered) atomicAdd(&st[2], (unsigned long long)s_filtered);
      if (n_notfr) atomicAdd(&st[3 + FGX_REJ_NOT_PRIMARY_FR_PAIR], (unsigned long long)n_notfr);
      if (rj_insuf) atomicAdd(&st[3 + FGX_REJ_INSUFFICIENT_READS], (unsigned long long)rj_insuf);
      if (rj_overlap) atomicAdd(&st[3 + FGX_REJ_INSUFFICIENT_OVERLAP], (unsigned long long)rj_overlap);
      if (rj_indel) atomicAdd(&st[3 + FGX_REJ_INDEL_ERROR_BETWEEN_STRANDS], (unsigned long long)rj_indel);
      if (rj_clipfail) atomicAdd(&st[3 + FGX_REJ_CLIP_OVERLAP_FAILED], (unsigned long long)rj_clipfail);
      if (rj_down) atomicAdd(&st[3 + FGX_REJ_DOWNSAMPLED], (unsigned long long)rj_down);
      atomicAdd(D.n_done, 1u);
      if (Mp->capped) atomicAdd(D.n_done + 1, 1u);
    }
  };
  auto to_defer = [&]() { if (lane == 0) { const uint32_t k = atomicAdd(P.n_deferred, 1u); P.deferred[k] = g; } };
  if (status == 1u) { flush_stats(); return; }   // the gates of the record kernel decided: nothing comes out
  const uint32_t ms0 = uni(Mp->m[0]), ms1 = uni(Mp->m[1]), len1 = uni(Mp->len[0]), len2 = uni(Mp->len[1]);
  const unsigned long long row0 = uniform_u64((unsigned long long)Mp->row0);
  const DeepRow* const rows = D.rows + row0;
  const uint64_t col_base = uniform_u64(P.col_base[g]);
  const uint8_t* const blob = P.blob;
  const DeviceTables* T = P.T;
  const uint32_t my_list = blockIdx.x & (N_LISTS - 1);
  bool list_overflow = false;
  auto push_full = [&](bool need, uint64_t dest, const double* ll, const uint32_t* obs) {
    list_overflow |= push_full_global(P, lane, my_list, need, dest, ll, obs[0] | (obs[1] << 8) | (obs[2] << 16) | (obs[3] << 24), 0u);   // (a strand holds at most 127 reads, the molecule 254 RX values: bytes)
  };
  // the rows through the scalar unit, as k_deep_cols reads them (k_codec_deep_parse wrote them, a kernel boundary ago)
  typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
  typedef const FGX_CONST_AS u32x8* RowPtr;
  auto row_seq = [&](const u32x8& r) { return blob + (((unsigned long long)r[1] << 32) | r[0]); };
  CallConst KC;
  KC.cap = uni(sT.cap);
  KC.cap_threshold = uniform_f64(sT.cap_threshold); KC.half_cerr_at_cap = uniform_f64(sT.half_cerr_at_cap);

  // ---- 6C. the two single-strand column sets (ss caller: min_reads 1, no quality masking, min consensus base quality 0).  A CODEC source read is its
  //          clipped bases as they are: no mask below min_input_bq, no trailing-N strip, no overlapping-bases pre-correction --------------------------------
  bool odd_base = false;
#pragma unroll 1
  for (uint32_t k = 0; k < 2; k++) {
    const uint32_t m = k == 0 ? ms0 : ms1, Lc = k == 0 ? len1 : len2, coff = k == 0 ? 0u : len1;
    const RowPtr er = (RowPtr)(rows + (k == 0 ? 0u : ms0));
    if (m == 1) {   // single-read consensus: LUT keyed by the unclamped quality (vanilla_caller.rs:1677-1708)
      const u32x8 R = er[0];
      const uint32_t L = R[4] & 0xFFFFu, fin = R[4] >> 16;
      const bool rv = ((R[7] >> 16) & 1u) != 0;
      const uint8_t* const sq = row_seq(R);
      for (uint32_t p = lane; p < Lc; p += 64) {                // (Lc = fin: the set's length is its one read's)
        const uint32_t idx = p < fin ? (rv ? L - 1u - p : p) : 0u;
        uint32_t code = ((uint32_t)sq[idx >> 1] >> ((~idx & 1u) << 2)) & 15u;
        const uint32_t qq = sq[((L + 1u) >> 1) + idx];
        if (rv) code = __builtin_bitreverse32(code) >> 28;     // complement = bit reversal of the code
        const uint8_t adjq = qq < 94 ? T->single_input_quals[qq] : 0;
        const uint64_t o = col_base + coff + p;
        P.col_code[o] = (uint8_t)code; P.col_qual[o] = adjq; P.col_depth[o] = code != 15 ? 1 : 0; P.col_err[o] = 0;
        if (code != 15 && code != 1 && code != 2 && code != 4 && code != 8) odd_base = true;   // IUPAC code in a lone read: general path
      }
    } else if (m > 1) {
      for (uint32_t p0 = 0; p0 < Lc; p0 += 64) {                // (uniform trip counts: m and Lc are scalars)
        const uint32_t p = uni(p0) + lane;
        const bool incol = p < Lc;
        const uint32_t shp = (~p & 1u) << 2;                   // nibble shift of an even / odd index (a reverse read of even length flips it)
        ChainAcc acc;                                          // Kahan chains by order of appearance (consensus_math.h)
        acc.reset();
        constexpr int NB = FGX_DEEP_BATCH;
        for (uint32_t j0 = 0; j0 < m; j0 += NB) {
          u32x8 R_[NB];
#pragma unroll
          for (int t = 0; t < NB; t++) R_[t] = er[uni(j0 + t < m ? j0 + t : m - 1u)];   // (past the end: the last row again, not observed)
          uint32_t b_[NB], q_[NB];
          bool in_[NB];
          // every load of the batch is issued before the first of them is used
#pragma unroll
          for (int t = 0; t < NB; t++) {
            const u32x8& R = R_[t];
            const uint32_t L = R[4] & 0xFFFFu, fin = R[4] >> 16;
            const bool rv = ((R[7] >> 16) & 1u) != 0;
            in_[t] = incol && p < fin && (j0 + t < m);          // inside the read's clipped length
            const uint32_t xm = rv ? ~0u : 0u, xk = rv ? L : 0u;    // index into the read: forward p, reverse L - 1 - p = (p ^ ~0) + L
            const uint32_t ix = in_[t] ? (p ^ xm) + xk : 0u;
            const uint8_t* const sq = row_seq(R);
            b_[t] = sq[ix >> 1]; q_[t] = sq[((L + 1u) >> 1) + ix];
          }
#pragma unroll
          for (int t = 0; t < NB; t++) {
            const u32x8& R = R_[t];
            const bool rv = ((R[7] >> 16) & 1u) != 0;
            const uint32_t L = R[4] & 0xFFFFu;
            uint32_t c = __builtin_amdgcn_ubfe(b_[t], shp ^ ((rv && !(L & 1u)) ? 4u : 0u), 4u);   // parity of L - 1 - p = parity of p when L is odd
            if (rv) c = __builtin_bitreverse32(c) >> 28;       // complement = bit reversal of the code
            const bool valid = in_[t] && __builtin_amdgcn_ubfe(0x116u, c, 1u) != 0;   // inside the read, one of A C G T (whatever its quality)
            const uint32_t q = q_[t], qq = q < FGX_MAX_PHRED ? q : FGX_MAX_PHRED;
            const double2 pr = *(const double2*)&sL.pair[qq][0];
            acc.add(valid, c, pr.x, pr.y);
          }
        }
        double ll[4];
        uint32_t obs[4];
        acc.finish(ll, obs);
        const uint64_t o = col_base + coff + p;
        int bi = -1;
        uint8_t q = 0;
        const bool resolved = !incol || column_call_fast_lds(sT, KC, ll, obs, &bi, &q);
        const uint32_t depth = obs[0] + obs[1] + obs[2] + obs[3];
        if (incol) P.col_depth[o] = (uint16_t)depth;
        push_full(!resolved, o, ll, obs);
        if (resolved && incol) {
          const uint32_t err = depth - (bi == 0 ? obs[0] : bi == 1 ? obs[1] : bi == 2 ? obs[2] : bi == 3 ? obs[3] : 0u);
          P.col_code[o] = depth < 1 ? (uint8_t)15 : bi >= 0 ? (uint8_t)(1u << bi) : (uint8_t)15;
          P.col_qual[o] = depth < 1 ? (uint8_t)0 : q;
          P.col_err[o] = (uint16_t)err;
        }
      }
    }
  }
  if (__any(odd_base)) { to_defer(); return; }

  // ---- 7C. consensus UMI over EVERY record of the molecule that carries RX (codec_caller.rs:1725-1744): the RX list in file order, lane = character ----------
  const DeviceTables* TU = P.TU;
  const uint32_t rx_cnt = uni(Mp->rx_cnt), ulen = uni(Mp->ulen);     // (k_codec_deep_parse: the values are of one length, at most FAST_RX_CAP)
  char my_ch = 0;
  bool rx_fail = false;
  if (rx_cnt) {
    typedef const FGX_CONST_AS unsigned long long* UmiPtr;
    const UmiPtr ul = (UmiPtr)(D.umi + row0);
    const bool mychar = lane < ulen;
    ColumnAcc acc;
    acc.reset();
    uint32_t non_dna = 0, seen = 0;
    uint8_t fch = 0;
    bool mixed = false, differs = false;
    const double uc = TU->t.correct[20], ue = TU->t.error_per_alt[20];
    constexpr int NB = FGX_DEEP_BATCH;
    for (uint32_t j0 = 0; j0 < rx_cnt; j0 += NB) {
      uint8_t ch_[NB];
#pragma unroll
      for (int t = 0; t < NB; t++) {
        const unsigned long long o = uniform_u64(ul[uni(j0 + t < rx_cnt ? j0 + t : rx_cnt - 1u)]);
        ch_[t] = mychar ? blob[o + lane] : (uint8_t)'A';
      }
#pragma unroll
      for (int t = 0; t < NB; t++) {
        if (j0 + t >= rx_cnt) continue;                        // (uniform)
        const uint8_t ch = ch_[t];
        if (seen == 0) fch = ch;
        else if (ch != fch) differs = true;
        seen++;
        const uint8_t up = (ch >= 'a' && ch <= 'z') ? (uint8_t)(ch - 32) : ch;
        const bool dna = up == 'A' || up == 'C' || up == 'G' || up == 'T' || up == 'N';
        if (dna) { const int bl = bam::ascii_to_lane(ch); if (bl != 255) acc.add(bl, uc, ue); }
        else { non_dna++; if (ch != fch) mixed = true; }
      }
    }
    bool need_full = false, bad_col = false;
    if (rx_cnt == 1 || !__any(mychar && differs)) {
      const int bl = bam::ascii_to_lane(fch);
      my_ch = rx_cnt == 1 ? (char)fch : bl != 255 ? "ACGT"[bl] : (fch == 'N' || fch == 'n') ? 'N' : (char)fch;
    } else {
      if (non_dna == 0) {
        CallConst KU;
        KU.cap = TU->t.cap; KU.cap_threshold = TU->t.cap_threshold; KU.half_cerr_at_cap = TU->t.half_cerr_at_cap;
        int bi; uint8_t q;
        const bool resolved = column_call_fast_lds(TU->t, KU, acc.s, acc.obs, &bi, &q);
        my_ch = bi >= 0 ? "ACGT"[bi] : 'N';
        need_full = !resolved;
      } else if (non_dna == seen && !mixed) my_ch = (char)fch;
      else bad_col = true;
      if (!mychar) { need_full = false; bad_col = false; }
      if (__any(bad_col)) rx_fail = true;
    }
    push_full(need_full, (1ull << 63) | ((uint64_t)slot << 8) | lane, acc.s, acc.obs);   // (at most CODEC_DEEP_MAX records: the counts are bytes)
  }
  // an RX failure or a full FullItem pool: the general path owns this molecule (nothing of the descriptor is written yet: valid stays 0, rec_sizes 0)
  if (rx_fail || __any(list_overflow)) { to_defer(); return; }

  // ---- 8C. descriptor --------------------------------------------------------------------------------------------------------------------------------------------
  {
    CodecDesc* const Dd = &P.cends[slot];
    const bool rx_empty = !(rx_cnt && ulen);                  // an all-empty consensus UMI is not written (:1740-1743)
    if (lane < ulen && rx_cnt) Dd->rx[lane] = my_ch;
    if (lane == 0) {
      const uint32_t C = Mp->cons_len, mi_len = Mp->mi_len, fc = Mp->fc, fc_cb_len = Mp->cb_len;
      const bool any_cb = Mp->has_cb != 0;
      Dd->s1_off = col_base; Dd->s2_off = col_base + len1; Dd->l1 = len1; Dd->l2 = len2; Dd->cons_len = C;
      Dd->first_rec = r0; Dd->cb_rec = r0 + fc;
      Dd->mi_off = Mp->mi_off; Dd->mi_len = (uint8_t)mi_len;
      Dd->has_cb = any_cb ? 1 : 0; Dd->cb_off = Mp->cb_off; Dd->cb_len = (uint8_t)fc_cb_len;
      Dd->has_rx = rx_empty ? 0 : 1; Dd->rx_len = (uint8_t)ulen; Dd->flags = Mp->neg;
      const uint32_t nm = P.prefix_len + 1 + mi_len;
      // every int tag holds a depth <= CODEC_DEEP_MAX (a byte: c or C): 4 bytes each
      const uint32_t size = 32 + nm + 1 + (C + 1) / 2 + C + (3 + P.rg_len + 1) + (3 + mi_len + 1) + 3 * (4 + 4 + 7) +
                            (P.per_base_tags ? 4 * (8 + 2 * C) + 4 * (3 + C + 1) : 0) + (any_cb ? 3 + fc_cb_len + 1 : 0) + (rx_empty ? 0 : 3 + ulen + 1);
      Dd->rec_size = size;
      Dd->valid = 1;
      P.rec_sizes[slot] = (uint64_t)size + 4;
    }
  }
  s_cons = 1;
  flush_stats();
}
