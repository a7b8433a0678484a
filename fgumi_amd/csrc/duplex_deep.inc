// duplex_deep.inc — deep duplex molecules (65 .. DEEP_MAX records): k_duplex_deep_parse (a workgroup per molecule, thread = record) +
// k_duplex_deep_cols (a wavefront per molecule, lane = column, the member reads of the four single-strand read sets STREAMED from global memory).
// Included by fastpath.hip inside `namespace fgx { namespace {` after simplex_deep.inc, whose DeepRow / DeepLds / deep_parse_records / deep_correct /
// k_deep_sizes it shares.
//
// Why: k_family_wave<1> holds a molecule in one wavefront — a lane per record, the records in an LDS slice — and defers what has more than 64 records to
// the general path (duplex_host.cpp).  Nothing of a duplex molecule's column phase needs the tile (simplex_deep.inc says why for a family's ends): the
// four read sets are streamed the same way, the overlapping-bases pre-correction applied where a byte is loaded.
//
//   k_duplex_deep_parse  phases 2 - 5D of k_family_wave<1> for a workgroup: the record rules of record_core.h through deep_parse_records, the duplex rules
//                        on top (the strand from the MI suffix, `/A` or `/B` on every paired record, the read-name length rule), mate pairing by name hash
//                        with the names verified, the shared span of each pair and the overlapping-bases counters, the final length of each read, fragments
//                        out, the strand partition with its gates (has_minimum_number_of_reads on the R1 counts, the strand-orientation collision check),
//                        the four read sets in file order (0 = AB-R1, 1 = AB-R2, 2 = BA-R1, 3 = BA-R2; one DeepRow per retained read) and the molecule's
//                        descriptor.  Reference: duplex_caller.rs:664-725, 824-862, 1944-2182; vanilla_caller.rs:1080-1190; overlapping.rs:236-336.
//   k_duplex_deep_cols   per set and 64-column pass the rows in file order, four at a time; Kahan chains by order of appearance (ChainAcc), the unanimous
//                        gate (column_call_fast_lds) or an item for k_call_full; the single-strand caller's rules (min_reads 1, minimum consensus base quality
//                        2); col_code / col_qual / col_err / col_obs; a set of one read through the single-read quality table; per set the depth maxima over
//                        the paired span and over the whole strand.  Then 7D and 8D of k_family_wave<1>: which records come out, the statistics with their
//                        re-attribution, the consensus UMI of each record, the two DuplexDescs and rec_sizes, the undo-and-defer on an RX failure or a
//                        list overflow.  The record writers (k_emit_duplex_fast, k_emit_duplex) take the descriptors as they take k_family_wave<1>'s.
//
// The bound.  Each of the two record sides — AB-R1 with BA-R2 (the R1 record), AB-R2 with BA-R1 (the R2 record) — holds at most DUPLEX_DEEP_SIDE_MAX = 255
// retained (non-zero-length) reads.  What fixes the 255 is a byte, three times over:
//   * every observation count of a column is a byte of col_obs and of FullItem::obs (fastpath.h) — a set is part of a side, so no count passes 255;
//   * aD aM bD bM are depths of one set and cD cM depths of the two sets of a side added: all <= 255, so every integer tag of a record is ONE byte wide
//     (type c up to 127, C above: int_tag_byte, record_writers.inc) — what the existing writers write and the `3 * (4 + 7 + 4)` term of the record size
//     assumes; no new record writer is needed;
//   * a consensus UMI character sees the reads of one side that carry RX: its four counts are bytes of an item too.
// A molecule holds at most DEEP_MAX = 512 records (510 retained reads at the bound; the LDS arrays of the record kernel).
// A --max-reads-per-strand does not move the bound: the 255 count ALL retained reads of a side, scoring or not — col_obs_all (the recount of a capped
// molecule) and the consensus UMI's item counts are bytes over every source read, whatever the cap leaves for the columns.  DEEP_MAX stays 512.
//
// --max-reads-per-strand (the CAP builds, k_duplex_deep_parse<NT, MAXR, 1> + k_duplex_deep_cols<1>; launched for a caller with a cap > 0 under
// FGX_DUPLEX_DEEP_CAP=1): a set above the cap is scored over its `cap` lowest fgbio name ranks, ties in file order, and the scoring reads enter a column in
// that order.  The record kernel keeps the rows of every retained read in file order and adds, for a capped set, COPIES of its scoring rows in walk order
// (DuplexDeepParams::rows_walk, at the set's place) — copies, not a list of indices into the file-order rows: the column loop's row loads are scalar loads
// of 32 consecutive bytes at `base + 32 j`, issued a batch ahead of their use, and an index list would put a second, dependent scalar load in front of each
// of them (load the index, wait, load the row), while the copies cost one more 32-byte store per scoring read in a kernel that already writes the row.
//
// Outside the shape — the molecule leaves for the deferred list, as it did from k_family_wave<1>: an indel (any I D N P op), a clip without the CLIPS builds (more than one CIGAR op; with them more than WG_CIG_OPS ops or no aligned block), a secondary or
// supplementary record, an unmapped read, an MC the closed-form mate clip does not take, no `/A` | `/B` on a paired record, absent qualities, a paired
// record that is FIRST and LAST, a --max-reads-per-strand that bites a set (without the CAP builds, and a cap of 0 with them), a side above the bound, more than DEEP_MAX records, RX of unequal length or
// above FAST_RX_CAP, an IUPAC code in a lone read, an overflow of the FullItem pool.  The host launches nothing of this under --trim, --rejects, in the
// methylation-aware mode or in the canonical second pass.

constexpr uint32_t DUPLEX_DEEP_SIDE_MAX = 255;   // retained reads of a record side (see "The bound" above)
static_assert(DUPLEX_DEEP_SIDE_MAX <= 255, "observation counts are bytes (col_obs, FullItem::obs) and the integer tags of a duplex record one byte wide");
static_assert(2 * DUPLEX_DEEP_SIDE_MAX <= DEEP_MAX, "a molecule at the bound fits the record kernel's arrays");

struct DuplexDeepMol {      // 96 bytes: what k_duplex_deep_parse hands to k_duplex_deep_cols
  uint32_t status;          // 0: not this path's (on the deferred list); 1: decided by the gates, counters only; 2: the column kernel decides
  uint32_t n, row0;         // records; first DeepRow (set 0's rows, then set 1's, 2's, 3's; file order inside a set)
  uint16_t m[4];            // retained reads of the four sets
  uint16_t elen[4];         // length of a set: its longest retained read
  uint32_t n_frag, n_ab;    // fragment records (FragmentRead); paired records
  uint32_t n_zero;          // paired records of final length 0 (ZeroLengthAfterTrimming)
  uint32_t rj_insuf, rj_coll;   // status 1: the reads the R1-count gate (InsufficientReads) / the collision check (PotentialCollision) rejected
  uint32_t ov_agree, ov_dis, ov_corr;
  uint32_t fp, fc;          // first paired record (MI -> read name, MI tag) and first /A (else /B) paired record (cell barcode), indices inside the molecule
  uint16_t mi_off, cb_off;  // ... their values' offsets inside the record body
  uint8_t mi_len, cb_len, has_cb, _pad0;   // mi_len: without the `/A` | `/B`
  // the CAP builds (--max-reads-per-strand; zero from the others): the SCORING reads of each set — the whole set unless the cap bites it
  uint16_t sc[4];           // how many: min(m, cap)
  uint16_t slen[4];         // the longest of them: the length of the set's consensus
  uint32_t capped;          // bit k: the cap bites set k (its scoring rows, in walk order, are in DuplexDeepParams::rows_walk)
};
static_assert(sizeof(DuplexDeepMol) == 96, "duplex deep descriptor");

struct DuplexDeepParams {
  const uint32_t* list; uint32_t n_list;     // the molecules of more than 64 records
  const uint64_t* row0;                      // per list entry: first DeepRow (exclusive scan of the record counts)
  DeepRow* rows; DuplexDeepMol* mols;        // mols: per list entry
  uint32_t* n_done;                          // molecules these kernels decided (fgx_debug_last_duplex_deep); [1]: of which the cap bit (fgx_debug_last_duplex_deep_capped)
  DeepRow* rows_walk;                        // the CAP builds: copies of a capped set's scoring rows in (rank, file order), at the set's place in `rows`
};

// DeepRow::w[7] of a duplex row: bit 2 of the flags byte = the read's FIRST flag (the halves of a paired UMI are flipped for reads whose FIRST flag differs
// from the record's); bits 0 / 1 as in simplex_deep.inc (reverse strand, carries RX)
// <CLIPS>: on DeepClipLds (lead / aln / tot per record and `multi`) for the clip-taking build of the record kernel
template <uint32_t MAXR, int CLIPS = 0>
struct DuplexDeepLds : DeepLdsOf<MAXR, CLIPS>::type {
  uint16_t mi_rel[MAXR];                 // MI value offset inside the record body
  uint8_t mi_len[MAXR];
  uint8_t dup[MAXR];                     // strand (0 none, 1 /A, 2 /B) | paired << 2 | FIRST << 3
  uint32_t n_paired, any_strand[2];      // any_strand: some record — a fragment too — ends its MI in /A, /B (duplex.rs:786-795)
  uint32_t pair_cnt[2], r1_cnt[2];       // paired records of strand A / B; of which R1
  uint32_t grp_n[2], grp_rev[2];         // A-R1 with B-R2 / A-R2 with B-R1: records, of which on the reverse strand
  uint32_t set_rem[4], set_len[4], n_zero, first_paired, first_of[2];
};

// <NT, MAXR>: <128, 128> takes the listed molecules of up to 128 records, <256, DEEP_MAX> the larger ones — both are launched over the whole list and a
// workgroup whose molecule is the other build's returns at once (no hand-over list, no host synchronisation between them).  Thread = record: a 66-record
// molecule in the 256-thread build would leave three of its four wavefronts without a record (DESIGN.md §4 has the figures).
//
// <CLIPS> 1 (launched under FGX_DEEP_CLIPS=1 in place of the CLIPS 0 build): reads with soft / hard clips around one aligned block (H* S* (M|=|X)+ S* H*, up to
// WG_CIG_OPS ops) are in the shape.  The reference calls such a read in query space like any other, so the rows and the column kernel see no difference; what
// the clips change is deep_parse_records<1>'s — the mate clip by the general rule on the ops — and the shared span of a pair in step 2: the ALIGNED blocks
// overlap, the leading clip goes into both query offsets (k_deep_parse<.., .., 1> step 2; k_family_wave<1, 1> restates the same for a wavefront).  A molecule
// with a multi-op record that this kernel accepts counts into deep_clipped_counter (fgx_debug_last_deep_clipped: "accepted by the record kernel" — the column
// kernel may still hand the molecule on for an RX failure or a full item pool).  CLIPS 0 is the kernel without any of it.
template <uint32_t NT, uint32_t MAXR, int CAP = 0, int CLIPS = 0>
__global__ __launch_bounds__(NT) void k_duplex_deep_parse(FastParams P, DuplexDeepParams D) {
  __shared__ DuplexDeepLds<MAXR, CLIPS> S;
  __shared__ __align__(16) uint8_t sTagCls[256];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t li = blockIdx.x;
  const uint32_t g = D.list[li];
  const uint32_t r0 = P.grp_first[g], n = P.grp_first[g + 1] - r0;
  if (MAXR < DEEP_MAX ? n > MAXR : n <= 128u) return;        // the other build's (uniform; ahead of every barrier)
  DuplexDeepMol* const M = &D.mols[li];
  fill_tag_classes(sTagCls);
  if (tid == 0) {
    S.bad = 0; S.ov_agree = S.ov_dis = S.ov_corr = 0;
    if constexpr (CLIPS != 0) S.multi = 0;
    S.n_paired = 0; S.n_zero = 0; S.first_paired = 0xFFFFFFFFu;
    for (int e = 0; e < 2; e++) { S.any_strand[e] = S.pair_cnt[e] = S.r1_cnt[e] = S.grp_n[e] = S.grp_rev[e] = 0; S.first_of[e] = 0xFFFFFFFFu; }
    for (int k = 0; k < 4; k++) { S.set_rem[k] = 0; S.set_len[k] = 0; }
  }
  auto leave = [&]() { if (tid == 0) { M->status = 0; const uint32_t k = atomicAdd(P.n_deferred, 1u); P.deferred[k] = g; } };
  if (tid < 3) { P.dends[3 * g + tid].valid = 0; P.rec_sizes[3 * g + tid] = 0; }
  if (n > MAXR) { leave(); return; }
  __syncthreads();
  const uint32_t min_bq = P.min_input_bq & 0xFFu;

  // ---- 1. parse: thread = record (k_simplex_wave2's record shape; an unmapped record is not in it here: the duplex caller needs a strand for every read) ----
  deep_parse_records<CLIPS>(P, S, S, r0, n, tid, NT, sTagCls, false);
  __syncthreads();
  if (S.bad) { leave(); return; }
  // the duplex rules of k_family_wave<1> phase 2: the strand from the MI suffix; every paired record needs `<id>/A` or `<id>/B` (duplex_caller.rs:2557-2566)
  // and a legal consensus read name; FIRST and LAST both set is the general path's.  (the tag walk once more: deep_parse_records keeps no MI per record)
  for (uint32_t r = tid; r < n; r += NT) {
    const uint8_t* const rec = P.blob + S.off[r];
    const uint32_t l_seq = S.l_seq[r], aux_off = (uint32_t)S.seq_rel[r] + ((l_seq + 1u) >> 1) + l_seq;
    AuxTags ax;
    aux_walk(rec, sTagCls, aux_off, P.rec_len[r0 + r] - aux_off, P, ax);
    const record::TagFields tg = record::unpack_tags(ax);
    uint32_t strand = 0;
    if (tg.has_mi && tg.mi_len >= 2 && rec[tg.mi_lo + tg.mi_len - 2] == '/') { const uint8_t sc = rec[tg.mi_lo + tg.mi_len - 1]; strand = sc == 'A' ? 1u : sc == 'B' ? 2u : 0u; }
    const uint32_t b = S.bits[r];
    const bool paired = (b & 3u) != 0, first = (b & 3u) == 1u, last = (b & 32u) != 0, rev = (b & 4u) != 0;
    if (paired && (strand == 0 || P.prefix_len + 1 + (tg.mi_len - 2) >= 255 || (first && last))) S.bad = 1;
    S.mi_rel[r] = (uint16_t)tg.mi_lo; S.mi_len[r] = (uint8_t)tg.mi_len;
    S.dup[r] = (uint8_t)(strand | (paired ? 4u : 0u) | (first ? 8u : 0u));
    if (strand) atomicOr(&S.any_strand[strand - 1], 1u);
    if (paired && strand) {
      const uint32_t sx = strand - 1, grp = ((strand == 1) == first) ? 0u : 1u;
      atomicAdd(&S.n_paired, 1u); atomicAdd(&S.pair_cnt[sx], 1u);
      if (first) atomicAdd(&S.r1_cnt[sx], 1u);
      atomicAdd(&S.grp_n[grp], 1u);
      if (rev) atomicAdd(&S.grp_rev[grp], 1u);
      atomicMin(&S.first_paired, r); atomicMin(&S.first_of[sx], r);
    }
  }
  __syncthreads();
  if (S.bad) { leave(); return; }

  // ---- 2. pairs and the reference span each pair shares (k_deep_parse's phase 2; every record of the molecule — fragments and both strands — takes part,
  //         as in k_family_wave<1> phase 3).  duplex.rs:786-795: only molecules with both strands when single-strand output is off ---------------------
  const bool do_overlap = P.overlap != 0 && (P.dmin_yx == 0 || (S.any_strand[0] && S.any_strand[1]));
  if (do_overlap) {
    for (uint32_t a = tid; a < n; a += NT) {
      const uint32_t ka = S.key[a];
      if ((ka & 3u) != 1u) continue;
      int cmate = -1, clater = -1;
      for (uint32_t j = 0; j < n; j++) {
        const uint32_t d = S.key[j] ^ ka;
        if (d == 0 && j > a) clater = (int)j;
        if (d == 3) cmate = (int)j;
      }
      const int other = clater >= 0 ? clater : cmate;
      if (other < 0) continue;
      const uint32_t nl = S.name_len[a];
      bool same = S.name_len[other] == nl;
      const uint8_t* const na = P.blob + S.off[a] + 32;
      const uint8_t* const nb = P.blob + S.off[other] + 32;
      for (uint32_t i = 0; i < nl && same; i += 8) {
        unsigned long long wa = gld64(na + i), wb = gld64(nb + i);
        if (i + 8 > nl) { const unsigned long long mk = (1ULL << (8 * (nl - i))) - 1; wa &= mk; wb &= mk; }
        if (wa != wb) same = false;
      }
      if (!same) { atomicOr(&S.bad, 1u); continue; }        // equal hashes, different names: the exact rules live in the general path
      if (clater >= 0) continue;                            // a later R1 carries the name: this one is not paired
      const uint32_t b = (uint32_t)cmate;
      if (S.ref_id[a] != S.ref_id[b]) continue;
      // (CLIPS: the aligned blocks share reference positions; a leading clip shifts the block's query offset.  The CLIPS 0 build has no aln / lead
      // arrays: it reads l_seq in a statement of its own)
      int32_t s1, e1, s2, e2;
      uint32_t qa = 0, qb = 0;
      if constexpr (CLIPS != 0) {
        s1 = S.pos[a] + 1; e1 = S.pos[a] + (int32_t)S.aln[a]; s2 = S.pos[b] + 1; e2 = S.pos[b] + (int32_t)S.aln[b];
        qa = S.lead[a]; qb = S.lead[b];
      } else { s1 = S.pos[a] + 1; e1 = S.pos[a] + (int32_t)S.l_seq[a]; s2 = S.pos[b] + 1; e2 = S.pos[b] + (int32_t)S.l_seq[b]; }
      const int32_t lox = s1 > s2 ? s1 : s2, hix = e1 < e2 ? e1 : e2;
      if (hix < lox) continue;
      const uint32_t cnt = (uint32_t)(hix - lox + 1), o1 = (uint32_t)(lox - s1) + qa, o2 = (uint32_t)(lox - s2) + qb;
      S.wo[a] = (uint16_t)o1; S.mo[a] = (uint16_t)o2; S.wc[a] = (uint16_t)cnt; S.partner[a] = (int16_t)b;
      S.wo[b] = (uint16_t)o2; S.mo[b] = (uint16_t)o1; S.wc[b] = (uint16_t)cnt; S.partner[b] = (int16_t)a;
    }
    __syncthreads();
    if (S.bad) { leave(); return; }
    // the overlapping-bases counters (overlapping.rs:51-60): a wavefront per pair, lane = shared position
    uint32_t ov_agree = 0, ov_dis = 0, ov_corr = 0;
    for (uint32_t a = wv; a < n; a += NT / 64) {
      if ((S.key[a] & 3u) != 1u || S.wc[a] == 0) continue;   // (uniform per wavefront)
      const uint32_t b = (uint32_t)S.partner[a];
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
    if (lane == 0) { if (ov_agree) atomicAdd(&S.ov_agree, ov_agree); if (ov_dis) atomicAdd(&S.ov_dis, ov_dis); if (ov_corr) atomicAdd(&S.ov_corr, ov_corr); }
  }
  __syncthreads();

  // ---- 3. final length per read: up to the mate clip, without its trailing N / masked bases — of what the pre-correction leaves there
  //         (vanilla_caller.rs:1129-1160; no --trim in this shape); the sets' sizes and lengths ------------------------------------------------------
  for (uint32_t r = tid; r < n; r += NT) {
    const uint32_t l_seq = S.l_seq[r], clip = S.clip[r];
    const bool rev = (S.bits[r] & 4u) != 0;
    const uint8_t* const sq = P.blob + S.off[r] + S.seq_rel[r];
    const uint32_t q0 = (l_seq + 1u) >> 1;
    const uint32_t wc = S.wc[r], wo = S.wo[r], mo = S.mo[r];
    const uint8_t* sm = sq;
    uint32_t mq0 = 0;
    if (wc) { const uint32_t b = (uint32_t)S.partner[r]; sm = P.blob + S.off[b] + S.seq_rel[b]; mq0 = ((uint32_t)S.l_seq[b] + 1u) >> 1; }
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
    const uint32_t d = S.dup[r];
    if (d & 4u) {
      const uint32_t k = ((d & 3u) - 1u) * 2u + ((d & 8u) ? 0u : 1u);
      if (flr > 0) { atomicAdd(&S.set_rem[k], 1u); atomicMax(&S.set_len[k], flr); }
      else atomicAdd(&S.n_zero, 1u);
    }
  }
  __syncthreads();

  // ---- 4. fragments out, the strand partition's gates (k_family_wave<1> 5D; every thread decides the same from LDS) -------------------------------------
  const uint32_t n_ab = S.n_paired, n_frag = n - n_ab;
  auto min_ok = [&](uint32_t x, uint32_t y) {                             // has_minimum_number_of_reads :824-862
    const uint32_t xy = x > y ? x : y, yx = x > y ? y : x;
    return P.dmin_total <= xy + yx && P.dmin_xy <= xy && P.dmin_yx <= yx;
  };
  uint32_t status = 2, rj_insuf = 0, rj_coll = 0;
  if (n_ab == 0) status = 1;                                             // nothing but fragments: no MI to work from
  else if (!min_ok(S.r1_cnt[0], S.r1_cnt[1])) { status = 1; rj_insuf = n_ab; }
  else if (S.pair_cnt[0] && S.pair_cnt[1]) {                             // /A R1 with /B R2 (and /A R2 with /B R1) must share a strand
    const bool same1 = S.grp_rev[0] == 0 || S.grp_rev[0] == S.grp_n[0], same2 = S.grp_rev[1] == 0 || S.grp_rev[1] == S.grp_n[1];
    if (!same1 || !same2) { status = 1; rj_coll = n_ab; }
  }
  const uint32_t m0 = S.set_rem[0], m1 = S.set_rem[1], m2 = S.set_rem[2], m3 = S.set_rem[3];
  uint32_t cutm = 0;                                                     // (CAP) bit k: the cap bites set k
  uint32_t la0 = 0, la1 = 0, la2 = 0, la3 = 0;                           // (CAP) the longest retained read of each set, ahead of the cap
  if (status == 2) {
    // a --max-reads-per-strand that bites a set: the general path without the CAP build, and with a cap of 0 (no set has a consensus); a cap that does
    // not bite changes nothing.  A side above the bound likewise — whatever the cap: the bound counts ALL retained reads ("The bound" above)
    const uint32_t mx = (m0 > m1 ? m0 : m1) > (m2 > m3 ? m2 : m3) ? (m0 > m1 ? m0 : m1) : (m2 > m3 ? m2 : m3);
    if (P.dmax_reads >= 0 && (long long)mx > P.dmax_reads) {
      if (CAP == 0 || P.dmax_reads == 0) { leave(); return; }
      const uint32_t cap = (uint32_t)P.dmax_reads;
      cutm = (m0 > cap ? 1u : 0u) | (m1 > cap ? 2u : 0u) | (m2 > cap ? 4u : 0u) | (m3 > cap ? 8u : 0u);
    }
    if (m0 + m3 > DUPLEX_DEEP_SIDE_MAX || m1 + m2 > DUPLEX_DEEP_SIDE_MAX) { leave(); return; }
  }
  // --max-reads-per-strand (consensus_call, vanilla_caller.rs:706-779 with downsample_source_reads :970-980; k_family_wave<1, 0, 1> restates it for a
  // wavefront, k_deep_parse's ranks for a workgroup): a set above the cap is SCORED over its `cap` lowest fgbio name ranks, ties in file order, and the
  // scoring reads enter a column in that order.  `key` is done with as the pairing hash: it holds the rank of each retained read of a capped set, then the
  // read's place in the walk order (a place >= cap: not a scoring read).  set_len of a capped set becomes the longest SCORING read.  Everything else of the
  // molecule keeps the whole set and file order — the rows below, and through them the consensus UMI and the recount's all-reads counts.
  // (Workgroup-uniform — cutm comes from LDS every thread read alike; a molecule the cap does not bite runs nothing of this.)
  if constexpr (CAP != 0) {
    la0 = S.set_len[0]; la1 = S.set_len[1]; la2 = S.set_len[2]; la3 = S.set_len[3];
    if (cutm) {
      const uint32_t cap = (uint32_t)P.dmax_reads;
      auto cut_set = [&](uint32_t r) -> int {                            // the capped set record r is a retained read of, or -1
        const uint32_t d = S.dup[r];
        if (!(d & 4u) || S.final_len[r] == 0) return -1;
        const uint32_t k = ((d & 3u) - 1u) * 2u + ((d & 8u) ? 0u : 1u);
        return ((cutm >> k) & 1u) ? (int)k : -1;
      };
      for (uint32_t r = tid; r < n; r += NT)
        if (cut_set(r) >= 0) S.key[r] = (uint32_t)name_rank(P.blob + S.off[r] + 32, S.name_len[r]);
      __syncthreads();
      uint32_t place[MAXR / NT];                                         // of record tid + i * NT
#pragma unroll
      for (uint32_t i = 0; i < MAXR / NT; i++) {
        const uint32_t r = tid + i * NT;
        place[i] = 0xFFFFFFFFu;
        if (r >= n || cut_set(r) < 0) continue;
        const uint32_t dk = S.dup[r] & 15u;                              // (strand, paired, FIRST): the set
        const int32_t rk = (int32_t)S.key[r];
        uint32_t before = 0;
        for (uint32_t j = 0; j < n; j++) {
          if ((S.dup[j] & 15u) != dk || S.final_len[j] == 0) continue;
          const int32_t rj = (int32_t)S.key[j];
          before += (rj < rk || (rj == rk && j < r)) ? 1u : 0u;
        }
        place[i] = before;
      }
      __syncthreads();
      if (tid < 4 && ((cutm >> tid) & 1u)) S.set_len[tid] = 0;           // (every thread read them, barriers ago)
#pragma unroll
      for (uint32_t i = 0; i < MAXR / NT; i++) { const uint32_t r = tid + i * NT; if (r < n && place[i] != 0xFFFFFFFFu) S.key[r] = place[i]; }
      __syncthreads();
      for (uint32_t r = tid; r < n; r += NT) { const int k = cut_set(r); if (k >= 0 && S.key[r] < cap) atomicMax(&S.set_len[k], (uint32_t)S.final_len[r]); }
      __syncthreads();
    }
  }

  // ---- 5. member rows: set 0's retained reads, then set 1's, 2's, 3's, file order inside a set -----------------------------------------------------------
  const unsigned long long row0 = D.row0[li];
  if (status == 2) {
    for (uint32_t r = tid; r < n; r += NT) {
      const uint32_t d = S.dup[r], fl = S.final_len[r];
      if (!(d & 4u) || fl == 0) continue;
      const uint32_t dk = d & 15u;                                       // (strand, paired, FIRST): the set
      const uint32_t k = ((d & 3u) - 1u) * 2u + ((d & 8u) ? 0u : 1u);
      uint32_t rank = 0;
      for (uint32_t j = 0; j < r; j++) rank += ((S.dup[j] & 15u) == dk && S.final_len[j] > 0) ? 1u : 0u;
      const uint32_t row = (k > 0 ? m0 : 0u) + (k > 1 ? m1 : 0u) + (k > 2 ? m2 : 0u) + rank;
      DeepRow R;
      const unsigned long long so = S.off[r] + S.seq_rel[r];
      unsigned long long mso = so;
      uint32_t ml = S.l_seq[r];
      if (S.wc[r]) { const uint32_t b = (uint32_t)S.partner[r]; mso = S.off[b] + S.seq_rel[b]; ml = S.l_seq[b]; }
      const bool hrx = (S.bits[r] & 8u) != 0;
      R.w[0] = (uint32_t)so; R.w[1] = (uint32_t)(so >> 32); R.w[2] = (uint32_t)mso; R.w[3] = (uint32_t)(mso >> 32);
      R.w[4] = (uint32_t)S.l_seq[r] | (fl << 16);
      R.w[5] = ml | ((uint32_t)S.wo[r] << 16);
      R.w[6] = (uint32_t)S.mo[r] | ((uint32_t)S.wc[r] << 16);
      R.w[7] = ((hrx ? (uint32_t)S.rx_rel[r] - (uint32_t)S.seq_rel[r] : 0u) & 0xFFFFu) |
               ((((S.bits[r] & 4u) ? 1u : 0u) | (hrx ? 2u : 0u) | ((d & 8u) ? 4u : 0u)) << 16) | ((uint32_t)S.rx_len[r] << 24);
      D.rows[row0 + row] = R;
      if constexpr (CAP != 0) { if (((cutm >> k) & 1u) && S.key[r] < (uint32_t)P.dmax_reads) D.rows_walk[row0 + (row - rank) + S.key[r]] = R; }
    }
  }

  // ---- 6. the molecule's descriptor ---------------------------------------------------------------------------------------------------------------------
  if (tid == 0) {
    DuplexDeepMol f;
    __builtin_memset(&f, 0, sizeof(f));
    f.status = status; f.n = n; f.row0 = (uint32_t)row0;
    f.m[0] = (uint16_t)m0; f.m[1] = (uint16_t)m1; f.m[2] = (uint16_t)m2; f.m[3] = (uint16_t)m3;
    for (int k = 0; k < 4; k++) f.elen[k] = (uint16_t)S.set_len[k];
    if constexpr (CAP != 0) {
      const uint32_t cap = (uint32_t)P.dmax_reads;
      for (int k = 0; k < 4; k++) { f.slen[k] = f.elen[k]; f.sc[k] = ((cutm >> k) & 1u) ? (uint16_t)cap : f.m[k]; }
      f.elen[0] = (uint16_t)la0; f.elen[1] = (uint16_t)la1; f.elen[2] = (uint16_t)la2; f.elen[3] = (uint16_t)la3;
      f.capped = cutm;
    }
    f.n_frag = n_frag; f.n_ab = n_ab; f.n_zero = S.n_zero; f.rj_insuf = rj_insuf; f.rj_coll = rj_coll;
    f.ov_agree = S.ov_agree; f.ov_dis = S.ov_dis; f.ov_corr = S.ov_corr;
    if (n_ab) {
      const uint32_t fp = S.first_paired, fc = S.first_of[0] != 0xFFFFFFFFu ? S.first_of[0] : S.first_of[1];
      f.fp = fp; f.fc = fc;
      f.mi_off = S.mi_rel[fp]; f.mi_len = (uint8_t)(S.mi_len[fp] - 2u);
      f.has_cb = (P.cell0 && (S.bits[fc] & 16u)) ? 1 : 0; f.cb_off = S.cb_rel[fc]; f.cb_len = S.cb_len[fc];
    }
    *M = f;
    if constexpr (CLIPS != 0) { if (S.multi) atomicAdd(deep_clipped_counter(P), 1u); }   // (no leave() behind this point)
  }
}

// -----------------------------------------------------------------------------------------------------------------------------
// k_duplex_deep_cols — wavefront = molecule, lane = column, rows streamed from global memory
// -----------------------------------------------------------------------------------------------------------------------------
#ifndef FGX_DUPLEX_DEEP_OCC
#define FGX_DUPLEX_DEEP_OCC 8
#endif
// <CAP>: the build for a caller with --max-reads-per-strand.  A capped set's columns come from its SCORING rows in walk order (rows_walk) — bases, qualities,
// col_err, col_obs, the depth maxima, the set's length and so the lengths of the records; a scoring set of one read takes the single-read table —, then its
// columns once more over EVERY row of the set, counting only (col_obs_all: the duplex error recount works from source_reads, which the cap does not touch);
// an uncapped set of such a molecule copies col_obs there.  The consensus UMI keeps all rows of a side in file order.  CAP 0: none of it.
template <int CAP>
__global__ __launch_bounds__(256, FGX_DUPLEX_DEEP_OCC) void k_duplex_deep_cols(FastParams P, DuplexDeepParams D) {
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
  const DuplexDeepMol* const Mp = &D.mols[li];
  const uint32_t status = uni(Mp->status);
  if (status == 0u) return;
  const uint32_t g = uni(D.list[li]);
  const uint32_t n = uni(Mp->n), n_frag = uni(Mp->n_frag), n_ab = uni(Mp->n_ab), n_zero = uni(Mp->n_zero);
  const uint32_t r0 = uni(P.grp_first[g]);
  const uint32_t slot0 = 3 * g;
  uint32_t cmask = 0;                                                     // bit k: the cap bites set k
  if constexpr (CAP != 0) cmask = uni(Mp->capped);
  unsigned long long* const st = P.stats + (size_t)(blockIdx.x & (STAT_SLOTS - 1)) * 32;
  uint32_t s_cons = 0, s_filtered = n_frag, rj_insuf = 0, rj_coll = 0, rj_zero = 0;
  auto flush_stats = [&]() {
    if (lane == 0) {
      const uint32_t ov_agree = Mp->ov_agree, ov_dis = Mp->ov_dis, ov_corr = Mp->ov_corr;
      atomicAdd(&st[0], (unsigned long long)n);
      if (s_cons) atomicAdd(&st[1], (unsigned long long)s_cons);
      if (s_filtered) atomicAdd(&st[2], (unsigned long long)s_filtered);
      if (n_frag) atomicAdd(&st[3 + FGX_REJ_FRAGMENT_READ], (unsigned long long)n_frag);
      if (rj_insuf) atomicAdd(&st[3 + FGX_REJ_INSUFFICIENT_READS], (unsigned long long)rj_insuf);
      if (rj_coll) atomicAdd(&st[3 + FGX_REJ_POTENTIAL_COLLISION], (unsigned long long)rj_coll);
      if (rj_zero) atomicAdd(&st[3 + FGX_REJ_ZERO_LENGTH_AFTER_TRIMMING], (unsigned long long)rj_zero);
      if (ov_agree + ov_dis) atomicAdd(&st[24], (unsigned long long)(ov_agree + ov_dis));
      if (ov_agree) atomicAdd(&st[25], (unsigned long long)ov_agree);
      if (ov_dis) atomicAdd(&st[26], (unsigned long long)ov_dis);
      if (ov_corr) atomicAdd(&st[27], (unsigned long long)ov_corr);
      atomicAdd(D.n_done, 1u);
      if constexpr (CAP != 0) { if (cmask) atomicAdd(D.n_done + 1, 1u); }
    }
  };
  auto to_defer = [&]() { if (lane == 0) { const uint32_t k = atomicAdd(P.n_deferred, 1u); P.deferred[k] = g; } };
  if (status == 1u) {   // the gates of the record kernel decided: nothing comes out
    rj_insuf = uni(Mp->rj_insuf); rj_coll = uni(Mp->rj_coll); s_filtered += rj_insuf + rj_coll;
    flush_stats();
    return;
  }
  const uint32_t ms0 = uni(Mp->m[0]), ms1 = uni(Mp->m[1]), ms2 = uni(Mp->m[2]), ms3 = uni(Mp->m[3]);
  // the scoring reads of each set and the length of its consensus, their longest (CAP: k_duplex_deep_parse<.., 1> fills sc / slen for every molecule)
  const uint32_t sc0 = CAP != 0 ? uni(Mp->sc[0]) : ms0, sc1 = CAP != 0 ? uni(Mp->sc[1]) : ms1, sc2 = CAP != 0 ? uni(Mp->sc[2]) : ms2, sc3 = CAP != 0 ? uni(Mp->sc[3]) : ms3;
  const uint32_t el0 = uni(CAP != 0 ? Mp->slen[0] : Mp->elen[0]), el1 = uni(CAP != 0 ? Mp->slen[1] : Mp->elen[1]), el2 = uni(CAP != 0 ? Mp->slen[2] : Mp->elen[2]),
                 el3 = uni(CAP != 0 ? Mp->slen[3] : Mp->elen[3]);
  auto pick = [](uint32_t k, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return k == 0 ? a : k == 1 ? b : k == 2 ? c : d; };
  const uint32_t plen1 = (ms0 && ms3) ? (el0 < el3 ? el0 : el3) : 0;    // R1 duplex: AB-R1 with BA-R2
  const uint32_t plen2 = (ms1 && ms2) ? (el1 < el2 ? el1 : el2) : 0;    // R2 duplex: AB-R2 with BA-R1
  const DeepRow* const rows = D.rows + uni(Mp->row0);
  const uint64_t col_base = uniform_u64(P.col_base[g]);
  const uint8_t* const blob = P.blob;
  const uint32_t min_bq = uni((uint32_t)P.min_input_bq & 0xFFu);
  const DeviceTables* T = P.T;
  const uint32_t my_list = blockIdx.x & (N_LISTS - 1);
  bool list_overflow = false;
  auto push_full = [&](bool need, uint64_t dest, const double* ll, const uint32_t* obs) {
    list_overflow |= push_full_global(P, lane, my_list, need, dest, ll, obs[0] | (obs[1] << 8) | (obs[2] << 16) | (obs[3] << 24), 0u);
  };
  // the rows through the scalar unit, as k_deep_cols reads them (k_duplex_deep_parse wrote them, a kernel boundary ago)
  typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
  typedef const FGX_CONST_AS u32x8* RowPtr;
  auto row_seq = [&](const u32x8& r) { return blob + (((unsigned long long)r[1] << 32) | r[0]); };
  auto row_mate = [&](const u32x8& r) { return blob + (((unsigned long long)r[3] << 32) | r[2]); };
  CallConst KC;
  KC.cap = uni(sT.cap);
  KC.cap_threshold = uniform_f64(sT.cap_threshold); KC.half_cerr_at_cap = uniform_f64(sT.half_cerr_at_cap);

  // ---- 6D. the four single-strand column sets (ss caller: min_reads 1, min consensus base quality 2) -----------------------------------------------------
  uint32_t dtr0 = 0, dtr1 = 0, dtr2 = 0, dtr3 = 0, dfu0 = 0, dfu1 = 0, dfu2 = 0, dfu3 = 0;   // max depth over the paired span / the whole strand, per set
  bool odd_base = false;
  uint32_t row_base = 0, coff = 0;
  // (CAP) the count-only pass of a capped set: one 64-column pass (columns p0s .. p0s + 63 of a set of length Lc) over the `m` rows at `er`, FGX_DEEP_BATCH at a
  // time; `see(valid, code)` once per row and lane — valid: inside the read's final length, not masked, one of A C G T, after the overlapping-bases
  // pre-correction and the strand complement.  It is the batch of the column loop below, loads and masking rule, without the chains: the column loop keeps
  // its own copy, because handing it the batch through this lambda cost the CAP 0 build registers (DESIGN.md §3 has the figures).
  auto stream_rows = [&](const RowPtr er, const uint32_t m, const uint32_t p0s, const uint32_t p, const uint32_t Lc, auto&& see) {
    const uint32_t shp = (~p & 1u) << 2;                       // nibble shift of an even / odd index (a reverse read of even length flips it)
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
        const uint32_t lim = fin < Lc ? fin : Lc;          // inside the read's final length AND a column of the set
        in_[t] = p < lim && (j0 + t < m);
        const uint32_t xm = rv ? ~0u : 0u, xk = rv ? L : 0u;    // index into the read: forward p, reverse L - 1 - p = (p ^ ~0) + L
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
          d_[t] = hit ? j : 0xFFFFFFFFu;                  // (the mate's index: its parity picks the nibble)
        }
      }
#pragma unroll
      for (int t = 0; t < NB; t++) {
        const u32x8& R = R_[t];
        const bool rv = ((R[7] >> 16) & 1u) != 0;
        const uint32_t L = R[4] & 0xFFFFu;
        uint32_t c = __builtin_amdgcn_ubfe(b_[t], shp ^ ((rv && !(L & 1u)) ? 4u : 0u), 4u), q = q_[t];   // parity of L - 1 - p = parity of p when L is odd
        if (d_[t] != 0xFFFFFFFFu) deep_correct(c, q, __builtin_amdgcn_ubfe(b2_[t], (~d_[t] & 1u) << 2, 4u), q2_[t]);
        if (rv) c = __builtin_bitreverse32(c) >> 28;       // complement = bit reversal of the code
        const bool valid = in_[t] && q >= min_bq && __builtin_amdgcn_ubfe(0x116u, c, 1u) != 0;   // inside the read, not masked, one of A C G T
        see(valid, c);
      }
    }
  };
#pragma unroll 1
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t m = pick(k, sc0, sc1, sc2, sc3), Lc = pick(k, el0, el1, el2, el3);      // the SCORING reads (CAP 0: sc is ms)
    const uint32_t plen = (k == 0 || k == 3) ? plen1 : plen2;
    const bool by_rank = CAP != 0 && ((cmask >> k) & 1u) != 0;     // a capped set: its scoring rows in (rank, file order), from rows_walk
    const bool copy_all = CAP != 0 && cmask != 0 && !by_rank;      // an uncapped set beside a capped one: col_obs IS the count over every source read
    const RowPtr er = (RowPtr)((by_rank ? D.rows_walk + uni(Mp->row0) : rows) + row_base);
    uint32_t lfu = 0, ltr = 0;
    if (m == 1) {   // single-read consensus: LUT keyed by the unclamped quality (vanilla_caller.rs:1677-1708)
      const u32x8 R = er[0];
      const uint32_t L = R[4] & 0xFFFFu, fin = R[4] >> 16, wo = R[5] >> 16, mo = R[6] & 0xFFFFu, wc = R[6] >> 16, mL = R[5] & 0xFFFFu;
      const bool rv = ((R[7] >> 16) & 1u) != 0;
      const uint8_t* const sq = row_seq(R);
      const uint8_t* const sm = row_mate(R);
      for (uint32_t p = lane; p < Lc; p += 64) {
        const bool in = p < fin;
        const uint32_t idx = in ? (rv ? L - 1u - p : p) : 0u;
        uint32_t code = ((uint32_t)sq[idx >> 1] >> ((~idx & 1u) << 2)) & 15u, qq = sq[((L + 1u) >> 1) + idx];
        if (in && idx - wo < wc) { const uint32_t j = mo + (idx - wo); deep_correct(code, qq, ((uint32_t)sm[j >> 1] >> ((~j & 1u) << 2)) & 15u, sm[((mL + 1u) >> 1) + j]); }
        if (rv) code = __builtin_bitreverse32(code) >> 28;
        if (!in) { code = 15; qq = FGX_MIN_PHRED; }
        if (qq < min_bq) { code = 15; qq = FGX_MIN_PHRED; }
        const uint8_t adj = qq < 94 ? T->single_input_quals[qq] : 0;
        const bool low = adj < FGX_MIN_PHRED;
        const uint64_t o = col_base + coff + p;
        P.col_code[o] = low ? (uint8_t)15 : (uint8_t)code; P.col_qual[o] = low ? (uint8_t)FGX_MIN_PHRED : adj; P.col_err[o] = 0;
        const uint32_t o0 = code == 1, o1 = code == 2, o2 = code == 4, o3 = code == 8;
        const uint32_t depth = code != 15 ? 1u : 0u;
        if (depth && !(o0 | o1 | o2 | o3)) odd_base = true;               // IUPAC code in a lone read: general path
        P.col_obs[o] = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24);
        if constexpr (CAP != 0) { if (copy_all) P.col_obs_all[o] = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24); }
        lfu = depth > lfu ? depth : lfu;
        if (p < plen) ltr = depth > ltr ? depth : ltr;
      }
    } else if (m > 1) {
      for (uint32_t p0 = 0; p0 < Lc; p0 += 64) {
        const uint32_t p0s = uni(p0);
        const uint32_t p = p0s + lane;
        const bool incol = p < Lc;
        const uint32_t shp = (~p & 1u) << 2;                   // nibble shift of an even / odd index (a reverse read of even length flips it)
        ChainAcc acc;                                          // Kahan chains by order of appearance (consensus_math.h)
        acc.reset();
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
            const uint32_t lim = fin < Lc ? fin : Lc;          // inside the read's final length AND a column of the set
            in_[t] = p < lim && (j0 + t < m);
            const uint32_t xm = rv ? ~0u : 0u, xk = rv ? L : 0u;    // index into the read: forward p, reverse L - 1 - p = (p ^ ~0) + L
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
              d_[t] = hit ? j : 0xFFFFFFFFu;                  // (the mate's index: its parity picks the nibble)
            }
          }
#pragma unroll
          for (int t = 0; t < NB; t++) {
            const u32x8& R = R_[t];
            const bool rv = ((R[7] >> 16) & 1u) != 0;
            const uint32_t L = R[4] & 0xFFFFu;
            uint32_t c = __builtin_amdgcn_ubfe(b_[t], shp ^ ((rv && !(L & 1u)) ? 4u : 0u), 4u), q = q_[t];   // parity of L - 1 - p = parity of p when L is odd
            if (d_[t] != 0xFFFFFFFFu) deep_correct(c, q, __builtin_amdgcn_ubfe(b2_[t], (~d_[t] & 1u) << 2, 4u), q2_[t]);
            if (rv) c = __builtin_bitreverse32(c) >> 28;       // complement = bit reversal of the code
            const bool valid = in_[t] && q >= min_bq && __builtin_amdgcn_ubfe(0x116u, c, 1u) != 0;   // inside the read, not masked, one of A C G T
            const uint32_t qq = q < FGX_MAX_PHRED ? q : FGX_MAX_PHRED;
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
        const bool resolved = incol ? column_call_fast_lds(sT, KC, ll, obs, &bi, &q) : true;
        const uint32_t depth = obs[0] + obs[1] + obs[2] + obs[3];
        push_full(incol && !resolved, o, ll, obs);
        if (incol) {
          if (resolved) {
            const uint32_t err = depth - (bi == 0 ? obs[0] : bi == 1 ? obs[1] : bi == 2 ? obs[2] : bi == 3 ? obs[3] : 0u);
            uint8_t ob, oq;
            if (depth < 1) { ob = 15; oq = 0; }
            else if (q < FGX_MIN_PHRED) { ob = 15; oq = FGX_MIN_PHRED; }
            else { ob = bi >= 0 ? (uint8_t)(1u << bi) : (uint8_t)15; oq = q; }
            P.col_code[o] = ob; P.col_qual[o] = oq; P.col_err[o] = (uint16_t)err;
          }
          P.col_obs[o] = obs[0] | (obs[1] << 8) | (obs[2] << 16) | (obs[3] << 24);     // (a set is part of a side: every count <= 255)
          if constexpr (CAP != 0) { if (copy_all) P.col_obs_all[o] = obs[0] | (obs[1] << 8) | (obs[2] << 16) | (obs[3] << 24); }
          lfu = depth > lfu ? depth : lfu;
          if (p < plen) ltr = depth > ltr ? depth : ltr;
        }
      }
    }
    // A capped set's columns once more, counting only: the observations of EVERY retained read of the set (the scoring ones included; file order, which
    // a count does not see) — what the duplex error recount of the record writers works from.  (uniform trip counts: m_all and Lc are scalars)
    if constexpr (CAP != 0) {
      if (by_rank) {
        const uint32_t m_all = pick(k, ms0, ms1, ms2, ms3);
        const RowPtr ar = (RowPtr)(rows + row_base);
        for (uint32_t p0 = 0; p0 < Lc; p0 += 64) {
          const uint32_t p0s = uni(p0);
          const uint32_t p = p0s + lane;
          uint32_t cnt = 0;
          stream_rows(ar, m_all, p0s, p, Lc, [&](bool valid, uint32_t c) { cnt += valid ? 1u << (c == 1u ? 0u : c == 2u ? 8u : c == 4u ? 16u : 24u) : 0u; });
          if (p < Lc) P.col_obs_all[col_base + coff + p] = cnt;
        }
      }
    }
    lfu = uni(wave_max(lfu)); ltr = uni(wave_max(ltr));
    if (k == 0) { dfu0 = lfu; dtr0 = ltr; } else if (k == 1) { dfu1 = lfu; dtr1 = ltr; } else if (k == 2) { dfu2 = lfu; dtr2 = ltr; } else { dfu3 = lfu; dtr3 = ltr; }
    row_base += pick(k, ms0, ms1, ms2, ms3); coff += Lc;            // (the rows of a set: ALL its retained reads)
  }
  if (__any(odd_base)) { to_defer(); return; }

  // ---- 7D. which records come out (duplex_consensus :931-1108, process_group :2400-2540) ------------------------------------------------------------------
  auto min_ok = [&](uint32_t x, uint32_t y) {                             // has_minimum_number_of_reads :824-862
    const uint32_t xy = x > y ? x : y, yx = x > y ? y : x;
    return P.dmin_total <= xy + yx && P.dmin_xy <= xy && P.dmin_yx <= yx;
  };
  auto dm_tr = [&](uint32_t k) { return pick(k, dtr0, dtr1, dtr2, dtr3); };
  auto dm_fu = [&](uint32_t k) { return pick(k, dfu0, dfu1, dfu2, dfu3); };
  auto elen = [&](uint32_t k) { return pick(k, el0, el1, el2, el3); };
  auto eoff = [&](uint32_t k) { return (k > 0 ? el0 : 0u) + (k > 1 ? el1 : 0u) + (k > 2 ? el2 : 0u); };
  auto rbase = [&](uint32_t k) { return (k > 0 ? ms0 : 0u) + (k > 1 ? ms1 : 0u) + (k > 2 ? ms2 : 0u); };
  struct Out { bool ok; bool has_ba; uint32_t sa, sb, len; };
  auto duplex_of = [&](int ka, int kb, uint32_t plen) {          // ka: AB-side set or -1, kb: BA-side set or -1
    Out r; r.ok = false; r.has_ba = false; r.sa = 0; r.sb = 0; r.len = 0;
    const bool have_a = ka >= 0, have_b = kb >= 0;
    const uint32_t ua = (uint32_t)(ka < 0 ? 0 : ka), ub = (uint32_t)(kb < 0 ? 0 : kb);
    const uint32_t da = have_a ? (have_b ? dm_tr(ua) : dm_fu(ua)) : 0;
    const uint32_t db = have_b ? (have_a ? dm_tr(ub) : dm_fu(ub)) : 0;
    const bool cov_a = have_a && da > 0, cov_b = have_b && db > 0;
    if (!cov_a && !cov_b) return r;
    if (cov_a && cov_b) { r.ok = min_ok(da, db); r.has_ba = true; r.sa = ua; r.sb = ub; r.len = plen; return r; }
    const uint32_t ks = cov_a ? ua : ub;                            // one covered strand: copied whole, depth over its full length
    r.ok = min_ok(dm_fu(ks), 0); r.sa = ks; r.sb = ks; r.len = elen(ks);
    return r;
  };
  const bool h1 = ms0 != 0, h2 = ms1 != 0, h3 = ms2 != 0, h4 = ms3 != 0;
  Out o1, o2;
  o1.ok = o2.ok = false; o1.has_ba = o2.has_ba = false; o1.sa = o1.sb = o2.sa = o2.sb = 0; o1.len = o2.len = 0;
  if (h1 && h2 && h3 && h4) { o1 = duplex_of(0, 3, plen1); o2 = duplex_of(1, 2, plen2); }
  else if (h1 && h2 && !h3 && !h4) { if (P.dmin_yx == 0) { o1 = duplex_of(0, -1, 0); o2 = duplex_of(1, -1, 0); } }
  else if (!h1 && !h2 && h3 && h4) { if (P.dmin_yx == 0) { o1 = duplex_of(-1, 2, 0); o2 = duplex_of(-1, 3, 0); } }
  const bool emitted = o1.ok && o2.ok;
  // statistics (duplex_caller.rs:2587-2610 with the re-attribution of :1894-1926)
  if (emitted) { s_cons = 2; rj_zero = n_zero; s_filtered += n_zero; }
  else { rj_insuf = n_ab - n_zero; rj_zero = n_zero; s_filtered += n_ab; }

  // ---- 8D. consensus UMI and descriptor of each record ------------------------------------------------------------------------------------------------------
  if (emitted) {
    const DeviceTables* TU = P.TU;
    const uint32_t fp = uni(Mp->fp), fc = uni(Mp->fc), fp_mi_len = uni(Mp->mi_len);
    const bool fc_has_cb = uni(Mp->has_cb) != 0;
    const uint32_t fc_cb_len = uni(Mp->cb_len);
    const bool full = h1 && h2 && h3 && h4;
    bool rx_fail = false;
#pragma unroll 1
    for (uint32_t t = 0; t < 2; t++) {
      const Out& O = t == 0 ? o1 : o2;
      // source reads of this record's UMIs, A-side first (file order inside a side); a read is flipped when its FIRST flag differs from the record's
      // (duplex_read_into :1336-1368).  side 0: the AB-strand set, side 1: the BA-strand set; 4: none
      const uint32_t ksa = (full || h1) ? (t == 0 ? 0u : 1u) : 4u;
      const uint32_t ksb = full ? (t == 0 ? 3u : 2u) : h1 ? 4u : (t == 0 ? 2u : 3u);
      const bool rec_first = t == 0;
      // the reads that carry RX: how many, the first one's length, are all of that length (scalar: the rows' last dword)
      uint32_t cnt = 0, ulen = 0;
      bool len_bad = false;
      for (uint32_t side = 0; side < 2; side++) {
        const uint32_t ks = side == 0 ? ksa : ksb;
        if (ks > 3u) continue;
        const RowPtr er = (RowPtr)(rows + rbase(ks));
        const uint32_t m = pick(ks, ms0, ms1, ms2, ms3);
        for (uint32_t j = 0; j < m; j++) {
          const u32x8 R = er[uni(j)];
          if (!((R[7] >> 17) & 1u)) continue;
          if (cnt == 0) ulen = R[7] >> 24;
          else if ((R[7] >> 24) != ulen) len_bad = true;
          cnt++;
        }
      }
      char my_ch = 0;
      if (cnt) {
        if (len_bad || ulen > (uint32_t)FAST_RX_CAP) rx_fail = true;
        else {
          const bool mychar = lane < ulen;
          ColumnAcc acc;
          acc.reset();
          uint32_t non_dna = 0, seen = 0;
          uint8_t fch = 0;
          bool mixed = false, differs = false;
          const double uc = TU->t.correct[20], ue = TU->t.error_per_alt[20];
          for (uint32_t side = 0; side < 2; side++) {
            const uint32_t ks = side == 0 ? ksa : ksb;
            if (ks > 3u) continue;
            const RowPtr er = (RowPtr)(rows + rbase(ks));
            const uint32_t m = pick(ks, ms0, ms1, ms2, ms3);
            for (uint32_t j = 0; j < m; j++) {
              const u32x8 R = er[uni(j)];
              if (!((R[7] >> 17) & 1u)) continue;              // (uniform: the read carries no RX)
              const uint8_t* const rx = row_seq(R) + (R[7] & 0xFFFFu);
              // '-' structure of this read's RX (flipping a paired UMI swaps the halves around the single dash)
              const uint8_t raw = mychar ? rx[lane] : (uint8_t)0;
              const unsigned long long dm = __ballot(mychar && raw == '-');
              const uint32_t nd = (uint32_t)__popcll(dm), dp = dm ? (uint32_t)__builtin_ctzll(dm) : 0u;
              const bool flip = (((R[7] >> 18) & 1u) != 0) != rec_first;
              if (flip && nd > 1) rx_fail = true;
              uint32_t src = lane;
              if (flip && nd == 1) { const uint32_t ql = ulen - dp - 1; src = lane < ql ? dp + 1 + lane : lane == ql ? dp : lane - ql - 1; }
              const uint8_t ch = mychar ? rx[src] : (uint8_t)'A';
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
          if (cnt == 1 || !__any(mychar && differs)) {
            const int bl = bam::ascii_to_lane(fch);
            my_ch = cnt == 1 ? (char)fch : bl != 255 ? "ACGT"[bl] : (fch == 'N' || fch == 'n') ? 'N' : (char)fch;
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
          push_full(need_full, (1ull << 63) | ((uint64_t)(slot0 + 1 + t) << 8) | lane, acc.s, acc.obs);   // (a side holds at most 255 reads: the counts are bytes)
        }
      }
      const uint32_t slot = slot0 + 1 + t;
      DuplexDesc* const Dd = &P.dends[slot];
      if (lane < ulen && cnt && ulen <= (uint32_t)FAST_RX_CAP) Dd->rx[lane] = my_ch;
      if (lane == 0) {
        const uint32_t L = O.len;
        Dd->a_off = col_base + eoff(O.sa); Dd->b_off = col_base + eoff(O.sb);
        Dd->len = L; Dd->first_rec = r0 + fp; Dd->cb_rec = r0 + fc;
        Dd->mi_off = Mp->mi_off; Dd->mi_len = (uint8_t)fp_mi_len;
        Dd->has_cb = fc_has_cb ? 1 : 0; Dd->cb_off = Mp->cb_off; Dd->cb_len = (uint8_t)fc_cb_len;
        Dd->has_rx = cnt > 0; Dd->rx_len = (uint8_t)ulen; Dd->type = (uint8_t)(1 + t); Dd->has_ba = O.has_ba ? 1 : 0;
        Dd->meth = 0; Dd->capped = (CAP != 0 && cmask != 0) ? 1 : 0;
        const uint32_t nm = P.prefix_len + 1 + fp_mi_len;
        const uint32_t per_strand = P.per_base_tags ? 2 * (3 + L + 1) + 2 * (8 + 2 * L) : 0;     // ac/aq strings + ad/ae arrays
        // every int tag holds a depth <= DUPLEX_DEEP_SIDE_MAX (a byte: c or C): 4 bytes each
        const uint32_t size = 32 + nm + 1 + (L + 1) / 2 + L + (3 + fp_mi_len + 1) + (fc_has_cb ? 3 + fc_cb_len + 1 : 0) + (3 + P.rg_len + 1) +
                              3 * (4 + 7 + 4) + per_strand + (O.has_ba ? per_strand : 0) + (cnt ? 3 + ulen + 1 : 0);
        Dd->rec_size = size;
        Dd->valid = 1;
        P.rec_sizes[slot] = (uint64_t)size + 4;
      }
    }
    if (rx_fail || __any(list_overflow)) {            // undo: the general path owns this molecule
      if (lane < 2) { P.dends[slot0 + 1 + lane].valid = 0; P.rec_sizes[slot0 + 1 + lane] = 0; }
      to_defer();
      return;
    }
  } else if (__any(list_overflow)) { to_defer(); return; }
  flush_stats();
}
