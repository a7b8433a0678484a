// simplex_deep.inc — deep simplex families (more than 64 records): k_deep_parse (a workgroup per family, thread = record) +
// k_deep_cols (a wavefront per family, lane = column, the member reads STREAMED from global memory).
// Included by fastpath.hip inside `namespace fgx { namespace {` after simplex_split.inc.
//
// Why: every other family kernel keeps the family's reads in LDS — whole records (k_family, k_simplex_wave2: 330 B per read) or
// sequence + qualities (k_split_cols: 240 B per read).  A family of 100 reads then owns 24 - 80 KB of a CU's 160 KB, a CU holds a
// handful of wavefronts, and every dependent LDS / f64 step is waited for in full: k_family spent 11.5 of the 27.5 ms of a 1 M-family
// long-tail batch (BASELINE configs[3] shape) on the 5.8 % of families above 64 records (2.5 ns per read; profiles/r04h).  Nothing in
// the column loop needs the tile: lane = column reads ITS byte of member read j — 64 consecutive bytes per wavefront and row, a
// coalesced load — in file order, and the one thing the tile was written for, the overlapping-bases pre-correction
// (overlapping.rs:236-336), is a pure function of the read's base and its mate's base at the shared position: it is applied where the
// byte is loaded.  So the column kernel needs no LDS beside its tables, a CU holds as many wavefronts as registers allow, loads of
// four rows are in flight together, and the family size is bounded by nothing but the counters' widths (255 reads per end).
//
//   k_deep_parse   thread = record, the family's per-record state in LDS arrays: the record rules of record_core.h (shape checks, aux
//                  walk, closed-form mate clip, name hash; deep_parse_records, shared with k_wide_parse), mate pairing with names verified, shared span of each pair, the
//                  overlapping-bases COUNTERS (a wavefront per pair, lane = shared position), the final length of each read (its 3' end
//                  walked back over what the pre-correction leaves there), the family gates, the member rows of each end in file
//                  order (one 32-byte DeepRow per retained read) and everything of the EndDescs that does not depend on the columns.
//   k_deep_cols    wavefront = family: per end and 64-column pass the rows in file order, four at a time; Kahan chains by order of
//                  appearance (ChainAcc, consensus_math.h — the column of a deep family shows a second base more often than not);
//                  the unanimous gate or an item for k_call_full; consensus UMI; record sizes (the cD / cM widths depend on the
//                  depths), counters.
//
// Shape: k_simplex_wave2's record shape (simplex_wave2.inc), at most DEEP_MAX records (DEEP_CAP_MAX under --max-reads), at most 255
// retained reads per end; no family with a fragment consensus AND a pair.  Everything else goes to k_family (up to 128 records) and
// from there to the host path.  The CLIPS 1 builds of k_deep_parse (below) also take reads with soft / hard clips around one aligned block: the
// methylation-aware mode launches them always, the plain mode under FGX_DEEP_CLIPS=1 (default off) in place of the CLIPS 0 builds.
//
// --max-reads (downsample_filtered_source_reads, vanilla_caller.rs:902-932) is decided in k_deep_parse where the family gates are taken,
// with the counters and in the order of k_family_wave<0> and k_family (fastpath.hip): per end, after the zero-length reads are out and
// the --min-reads checks, an end above the cap keeps its max_reads lowest fgbio name ranks (name_rank of the name in the blob, a thread
// per record into `key`, whose pairing hash is done with; signed compare, ties in file order); the dropped reads get final length 0 —
// "not retained" to every later step, so lengths, the min_reads-th-longest rule, rows, RX, cell barcode, orphan count and the methylation
// anchor see the survivors only, in file order — and count as Downsampled (DeepFam::rej_down, flushed by k_deep_cols).  The overlap
// pre-correction and its counters keep the whole family: a survivor's row may name a dropped mate, whose bytes are still in the blob.  The
// limit of 255 reads per end applies after the cut.  The branch is workgroup-uniform: without a biting cap nothing of it runs.
//
// Reference semantics restated: the same as k_simplex_wave2 (vanilla_caller.rs:1080-1296, 1304-1422, 1454-1646, 1652-1755;
// overlapping.rs:236-336, 627-684; raw-bam/overlap.rs:181-357; simple_umi.rs:46-117).

constexpr uint32_t DEEP_MAX = 512;           // records per family (LDS arrays of k_deep_parse: 23 KB; an end holds at most 255 retained reads anyway)
constexpr uint32_t DEEP_CAP_MAX = 1024;      // ... under --max-reads, which leaves an end at most max_reads of them (46 KB; `partner` stays 16 bits)

struct DeepRow {            // 32 bytes: one retained read of an end — eight dwords, read through the scalar unit (one s_load_dwordx8; sub-dword
                            // fields of a struct would come through vector memory, one dependent round trip before the row's own loads)
  uint32_t w[8];            // [0,1] blob offset of its SEQ bytes (the qualities follow at + (l_seq + 1) / 2)   [2,3] the same of the mate it shares
                            // reference positions with   [4] l_seq | final_len << 16   [5] mate l_seq | wo << 16   [6] mo | wc << 16 (shared bases: the
                            // first one in this read `wo` / in the mate `mo`, how many `wc`; 0: none)   [7] RX value offset from SEQ | flags << 16
                            // (bit 0 reverse strand, bit 1 carries RX) | RX length << 24
};
struct DeepFam {            // 64 bytes
  uint32_t status;          // 1: k_deep_cols takes the family; 0: not this path's
  uint32_t n, row0;         // records; first DeepRow
  uint16_t m_a, m_b, lc_a, lc_b;   // retained reads and consensus length of end A (fragment or R1) / end B (R2)
  uint8_t ne, type_a, rx_len_a, rx_len_b;
  uint16_t rx_cnt_a, rx_cnt_b;     // retained reads with RX
  uint32_t rej_insuf, rej_zero, rej_orphan;
  uint32_t ov_agree, ov_dis, ov_corr;
  // methylation-aware mode (annotate_and_normalize, vanilla_caller.rs:781-860): per end the anchor = the LAST longest retained read;
  // column p of the end lies at reference position a_ref0 + step * p of contig a_info & 0x0FFFFFFF
  int32_t a_ref0[2];
  uint32_t a_info[2];       // contig | annotated << 28 | step is -1 << 29 | is_top_strand(anchor) << 30 | is_top_strand(first retained read) << 31
  uint32_t rej_down;        // retained reads that --max-reads dropped
  uint32_t clipped;         // methylation-aware mode: a record of the family has more than one CIGAR op (k_deep_cols<1> counts the family once it is decided)
  uint32_t a_rec[2];        // methylation-aware mode, the canonical second pass (FGX_METH_CANON=1): per end the anchor's record index in the batch + 1 — k_deep_cols<1> looks
                            // the reference base up through that record's reference runs (canon::RefRuns, meth_ref_runs) instead of the one a_ref0 run; 0: no runs given
  uint32_t _pad[3];
};
static_assert(sizeof(DeepRow) == 32 && sizeof(DeepFam) == 96, "deep descriptors");

struct DeepParams {
  const uint32_t* list; uint32_t n_list;     // the families (more than 64 records)
  const uint64_t* row0;                      // per list entry: first DeepRow (exclusive scan of the record counts)
  DeepRow* rows; DeepFam* fams;              // fams: per list entry
  uint32_t* out_list; uint32_t* n_out;       // families outside the shape → k_family
};

// n of each listed family (the scan of these is where its rows go)
__global__ void k_deep_sizes(const uint32_t* __restrict__ list, uint32_t n_list, const uint32_t* __restrict__ grp_first, uint64_t* __restrict__ sizes) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_list) return;
  const uint32_t g = list[i];
  sizes[i] = grp_first[g + 1] - grp_first[g];
}

// what the overlapping-bases pre-correction leaves at a shared position (overlapping.rs:236-336): codes and qualities of this read and
// its mate in, this read's corrected code and quality out
__device__ __forceinline__ void deep_correct(uint32_t& c, uint32_t& q, uint32_t c2, uint32_t q2) {
  if (c == 15u || c2 == 15u) return;
  if (c == c2) { const uint32_t sm = q + q2; q = sm < 93u ? sm : 93u; return; }
  const int32_t d = (int32_t)q - (int32_t)q2;
  const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
  c = d == 0 ? 15u : d > 0 ? c : c2;
  q = ad < (uint32_t)FGX_MIN_PHRED ? (uint32_t)FGX_MIN_PHRED : ad;
}

template <uint32_t MAXR>
struct DeepLds {
  unsigned long long off[MAXR];          // record body offset in the blob
  uint32_t key[MAXR];                    // name hash << 2 | 1 (R1 type) / 2 (R2 type) / 0
  int32_t pos[MAXR], ref_id[MAXR];
  uint16_t l_seq[MAXR], seq_rel[MAXR], name_len[MAXR], clip[MAXR], final_len[MAXR];
  uint16_t wo[MAXR], mo[MAXR], wc[MAXR];
  uint16_t rx_rel[MAXR], cb_rel[MAXR];
  int16_t partner[MAXR];                 // the mate this read shares positions with (R1 <-> R2), -1: none
  uint8_t bits[MAXR];                    // end type (0 fragment, 1 R1, 2 R2) | reverse << 2 | has RX << 3 | has cell tag << 4 | LAST flag << 5
  uint8_t rx_len[MAXR], cb_len[MAXR];
  uint32_t bad, cnt[3], rem[3], fmin[3], fmax[3], rxcnt[3], rxfirst[3], rxbad, ov_agree, ov_dis, ov_corr;
  uint32_t clen[3];
};

// What the clip-taking build of k_deep_parse keeps per record beside DeepLds: a read of the shape H* S* (M|=|X)+ S* H* is `lead` soft-clipped query
// bases, an aligned block of `aln` bases at pos, and the rest of l_seq soft-clipped behind it; `tot` = the lengths of ALL its ops, hard clips included —
// the one M op the reference's simplify_cigar_from_raw makes of it (S, H, =, X folded into M, neighbours merged)
template <uint32_t MAXR>
struct DeepClipLds : DeepLds<MAXR> {
  uint16_t lead[MAXR], aln[MAXR], tot[MAXR];
  uint32_t multi;                        // a record of the family has more than one CIGAR op
};
template <uint32_t MAXR, int CLIPS> struct DeepLdsOf { typedef DeepLds<MAXR> type; };
template <uint32_t MAXR> struct DeepLdsOf<MAXR, 1> { typedef DeepClipLds<MAXR> type; };

// The parse of k_deep_parse and k_wide_parse (their phase 1): thread = record, the bytes straight from global memory, the rules of record_core.h.  S: the
// per-record state (DeepLds, or WideRecs' arrays of the same names), C: the family's counters (`bad`: bit 0 some record is not this path's, bits 1 - 3 the
// end holds an unmapped record; `multi` under CLIPS).  `take_unmapped`: an unmapped record without a CIGAR is in the shape (streaming_header_odd).
template <int CLIPS, class Recs, class Cnt>
__device__ __forceinline__ void deep_parse_records(const FastParams& P, Recs& S, Cnt& C, const uint32_t r0, const uint32_t n, const uint32_t tid, const uint32_t nt,
                                                   const uint8_t* const sTagCls, const bool take_unmapped) {
  for (uint32_t r = tid; r < n; r += nt) {
    const unsigned long long off = P.rec_off[r0 + r];
    const uint32_t len = P.rec_len[r0 + r];
    bool odd = false;
    uint32_t l_seq = 0, seq_rel = 0, name_len = 0, clip = 0, hash = 0, flags = 0, ty = 0;
    int32_t pos = 0, ref_id = 0;
    record::TagFields tg = {};
    record::CigarBlock cb = record::cigar_block_start();   // (CLIPS) leading soft clip, aligned block, all ops
    if (len < 36u || len > 0xFFFFu || off > P.blob_len || (unsigned long long)len > P.blob_len - off) odd = true;
    else {
      const uint8_t* const rec = P.blob + off;
      const record::FixedHeader H = record::decode_header(gld32(rec), gld32(rec + 4), gld32(rec + 8), gld32(rec + 12), gld32(rec + 16));
      const record::Layout lay = record::layout(H, len);
      l_seq = H.l_seq; flags = H.flags;
      const bool unm = (flags & bam::F_UNMAPPED) != 0;      // an unmapped record: a read without a CIGAR — l_seq query bases, ref_id / pos unused
      if (lay.odd || record::streaming_header_odd(H, CLIPS != 0 ? WG_CIG_OPS : 1u, take_unmapped, 0u)) odd = true;
      else {
        name_len = H.l_name - 1;
        ref_id = unm ? unmapped_ref_key(r) : H.ref_id; pos = H.pos;   // (no shared span with an unmapped member, phase 2)
        seq_rel = lay.seq_off;
        if (record::streaming_flags_odd(H, false)) odd = true;
        if (!unm) {
          const uint32_t op = gld32(rec + 32 + H.l_name);
          if (CLIPS == 0 || H.n_cig == 1) {
            if (!record::single_block_op(op, l_seq)) odd = true;
            cb.aln = cb.tot = l_seq;
          } else if constexpr (CLIPS != 0) {
            // clips around one aligned block; I D N P are not this path's
            for (uint32_t i = 0; i < H.n_cig; i++) record::cigar_block_op(cb, i == 0 ? op : gld32(rec + 32 + H.l_name + 4 * i));   // (at most 16 lengths below 2^28)
            if (!record::cigar_block_fits(cb, l_seq) || cb.tot > 65535u) odd = true;
            atomicOr(&C.multi, 1u);
          }
        }
        AuxTags ax;
        aux_walk(rec, sTagCls, lay.aux_off, len - lay.aux_off, P, ax);       // (offsets inside the record: below 2^16)
        if (ax.oddw) odd = true;
        tg = record::unpack_tags(ax);
        if (r == 0 && record::first_record_odd(tg.has_mi, tg.mi_len, P.prefix_len)) odd = true;
        if (!odd && tg.has_mc && !(flags & (bam::F_UNMAPPED | bam::F_MATE_UNMAPPED))) {   // (either of them: no clip, whatever MC says)
          const uint32_t ML = record::mc_single_m(tg.mc_len, [&]() { return gld64(rec + tg.mc_lo); });
          const record::MateFields M = record::decode_mate(gld32(rec + 20), gld32(rec + 24));
          const bool closed = ML != 0 && record::mate_in_range(M);   // this read's mate is one M op in the closed form's range
          if (CLIPS != 0 && !(closed && H.n_cig == 1)) {
            // the general rule on the ops.  Every function of it (bamrec.h: reference length, leading / trailing soft clip, query length, query bases
            // up to a reference position, is_fr_pair) gives the same for H* S* (M|=|X)+ S* H* as for `lead S, block M, trail S`: hard clips count
            // nowhere, soft clips are summed from either end, neighbouring aligned ops are walked as one — so three ops stand for the sixteen
            uint32_t ops3[3] = {(cb.lead << 4) | 4u, cb.aln << 4, ((l_seq - cb.lead - cb.aln) << 4) | 4u};
            uint32_t mops[MAX_MC_OPS];
            bool overflow = false;
            if (!odd) {
              const bam::Rec v{rec, len};
              const unsigned long long cl = bam::mate_clip(v, ops3, 3, rec + tg.mc_lo, tg.mc_len, mops, MAX_MC_OPS, &overflow);
              if (overflow) odd = true;                        // (a mate of more ops than this kernel parses: the general path's)
              clip = (uint32_t)(cl > 65535ull ? 65535ull : cl);
            }
          } else if (!closed) odd = true;
          else clip = record::single_m_mate_clip(H, ref_id, M, (int32_t)ML);
        }
        if (!odd) {
          hash = record::name_hash30(name_len, [&](uint32_t o) { return gld32(rec + 32 + o); }, [&](uint32_t o) { return gld64(rec + 32 + o); });
          if (rec[lay.qual_off] == 0xFF) odd = true;                       // absent qualities (:1119-1124): the first one decides here
          if (tg.has_rx && tg.rx_len > 255u) odd = true;
        }
        ty = !(flags & bam::F_PAIRED) ? 0u : (flags & bam::F_FIRST) ? 1u : 2u;
      }
    }
    if (odd) C.bad = 1;
    else if (flags & bam::F_UNMAPPED) atomicOr(&C.bad, 2u << ty);    // bits 1 - 3: the end holds an unmapped record
    const uint32_t pt = odd ? 0u : (flags & bam::F_FIRST) ? 1u : (flags & bam::F_LAST) ? 2u : 0u;   // pair-map type (overlapping.rs:627-684)
    S.off[r] = off; S.key[r] = (hash << 2) | pt; S.pos[r] = pos; S.ref_id[r] = ref_id;
    S.l_seq[r] = (uint16_t)l_seq; S.seq_rel[r] = (uint16_t)seq_rel; S.name_len[r] = (uint16_t)name_len; S.clip[r] = (uint16_t)clip; S.final_len[r] = 0;
    S.wo[r] = 0; S.mo[r] = 0; S.wc[r] = 0; S.partner[r] = -1;   // (no mate yet; WideRecs' unsigned array holds it as 0xFFFFFFFF)
    if constexpr (CLIPS != 0) { S.lead[r] = (uint16_t)cb.lead; S.aln[r] = (uint16_t)cb.aln; S.tot[r] = (uint16_t)cb.tot; }
    S.rx_rel[r] = (uint16_t)tg.rx_lo; S.cb_rel[r] = (uint16_t)tg.cb_lo; S.rx_len[r] = (uint8_t)tg.rx_len; S.cb_len[r] = (uint8_t)tg.cb_len;
    S.bits[r] = (uint8_t)(ty | ((flags & bam::F_REVERSE) ? 4u : 0u) | (tg.has_rx ? 8u : 0u) | (tg.has_cb ? 16u : 0u) | ((flags & bam::F_LAST) ? 32u : 0u) |
                         ((flags & bam::F_UNMAPPED) ? 64u : 0u));
  }
}

// <NT, MAXR>: threads per workgroup and the records a family may have — <128, 128> and <256, 512> for the families above 64 records, <256, 1024>
// for those of more than 512 under --max-reads (an end fits its 255 reads after the cut only), <64, 64> for everything else when the streaming
// kernels are the whole pipeline (methylation-aware mode: a wavefront per family, 3 KB of LDS)
//
// CLIPS 1: the build of the methylation-aware mode — and, under FGX_DEEP_CLIPS=1, of the plain mode, where it keeps taking unmapped records and counts the
// families with a multi-op record it accepts (deep_clipped_counter) —, which takes soft- / hard-clipped reads (H* S* (M|=|X)+ S* H*, up to WG_CIG_OPS ops) beside the
// single-op ones.  The reference calls such a read in query space like any other (create_source_read :1094-1163 keeps the soft-clipped bases), so the
// column kernel sees no difference; what the clips change is restated here: the mate clip (bam::mate_clip on the ops), the shared span of a pair (the
// ALIGNED blocks overlap; the leading clip goes into the query offsets) and where the anchor's columns lie on the reference (step 6).  An indel read
// still sends the family to the deferred list: its columns are not one run of reference positions.  CLIPS 0 is the kernel without any of it.
template <uint32_t NT, uint32_t MAXR, int CLIPS = 0>
__global__ __launch_bounds__(NT) void k_deep_parse(FastParams P, DeepParams D) {
  constexpr uint32_t DEEP_NT = NT;
  __shared__ typename DeepLdsOf<MAXR, CLIPS>::type S;
  __shared__ __align__(16) uint8_t sTagCls[256];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t li = blockIdx.x;
  const uint32_t g = D.list[li];
  const uint32_t r0 = P.grp_first[g], n = P.grp_first[g + 1] - r0;
  DeepFam* const F = &D.fams[li];
  fill_tag_classes(sTagCls);
  if (tid == 0) {
    S.bad = 0; S.rxbad = 0; S.ov_agree = S.ov_dis = S.ov_corr = 0;
    if constexpr (CLIPS != 0) S.multi = 0;
    for (int e = 0; e < 3; e++) { S.cnt[e] = S.rem[e] = 0; S.fmin[e] = 0xFFFFFFFFu; S.fmax[e] = 0; S.rxcnt[e] = 0; S.rxfirst[e] = 0xFFFFFFFFu; S.clen[e] = 0; }
  }
  // not this path's: k_family decides (and defers what no device kernel takes)
  auto leave = [&]() {
    if (tid == 0) {
      F->status = 0;
      if (P.meth_mode) { const uint32_t k = atomicAdd(P.n_deferred, 1u); P.deferred[k] = g; }   // methylation-aware mode: k_family knows nothing of it — the general path's
      else { const uint32_t k = atomicAdd(D.n_out, 1u); D.out_list[k] = g; }
    }
  };
  // (first of all: a family that leaves for the deferred list — methylation-aware mode — is visited by no other kernel, and the slot tables are not cleared between batches)
  if (tid < 3) { P.ends[3 * g + tid].valid = 0; P.rec_sizes[3 * g + tid] = 0; }
  // the build for larger families takes it (the host launches it over this list next): above DEEP_MAX records only under --max-reads — without a cap
  // such a family has an end of more than 255 reads (almost always) — and the DEEP_CAP_MAX build, launched over what the DEEP_MAX build left, passes on what
  // that build had to decide
  if ((n > MAXR && (MAXR < DEEP_MAX || (MAXR < DEEP_CAP_MAX && n <= DEEP_CAP_MAX && P.max_reads >= 0))) || (MAXR > DEEP_MAX && n <= DEEP_MAX && !P.meth_mode)) {
    if (tid == 0) { F->status = 0; const uint32_t k = atomicAdd(D.n_out, 1u); D.out_list[k] = g; }
    return;
  }
  if (n > MAXR || n == 0 || n < P.min_reads) { leave(); return; }   // (uniform; fewer records than --min-reads: k_family counts them, simplex.rs:673-683)
  __syncthreads();
  const uint32_t min_bq = P.min_input_bq & 0xFFu;

  // ---- 1. parse: thread = record --------------------------------------------------------------------------------------------------------
  // (DeepLds holds the per-record arrays AND the family's counters: S is both arguments; k_wide_parse passes its global arrays and its LDS counters)
  deep_parse_records<CLIPS>(P, S, S, r0, n, tid, DEEP_NT, sTagCls, !P.meth_mode);   // (the clip builds outside the mode — FGX_DEEP_CLIPS=1 — keep taking unmapped records)
  __syncthreads();
  if (S.bad & 1u) { leave(); return; }
  if (S.bad >> 1) {
    // some record is unmapped (workgroup-uniform; a batch of mapped reads never comes here): bits 4 - 6, the end holds a mapped record.  An end with both
    // is not this path's — drop_unmapped_if_any_mapped (:1206-1232) works from the final lengths, k_family_wave<0> decides it up to 64 records
    for (uint32_t r = tid; r < n; r += DEEP_NT) if (!(S.bits[r] & 64u)) atomicOr(&S.bad, 16u << (S.bits[r] & 3u));
    __syncthreads();
    const uint32_t b = S.bad;
    if ((b >> 1) & (b >> 4) & 7u) { leave(); return; }
  }

  // ---- 2. pairs (pair map: per name the LAST R1-type and the LAST R2-type primary record; an R1 is paired unless a later R1 has its
  //         name) and the reference span each pair shares ----------------------------------------------------------------------------------
  if (P.overlap) {
    for (uint32_t a = tid; a < n; a += DEEP_NT) {
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
      if (!same) { atomicOr(&S.bad, 1u); continue; }        // equal hashes, different names: the exact rules live in k_family
      if (clater >= 0) continue;                            // a later R1 carries the name: this one is not paired
      const uint32_t b = (uint32_t)cmate;
      if (S.ref_id[a] != S.ref_id[b]) continue;
      // (CLIPS: the aligned blocks share reference positions; a leading clip shifts the block's query offset — k_family_wave<0>'s restatement.  The CLIPS 0
      // build has no aln / lead / tot arrays: it reads l_seq, here and at the anchor, in statements of its own)
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
    if (S.bad & 1u) { leave(); return; }
    // the overlapping-bases counters (overlapping.rs:51-60): a wavefront per pair, lane = shared position
    uint32_t ov_agree = 0, ov_dis = 0, ov_corr = 0;
    for (uint32_t a = wv; a < n; a += DEEP_NT / 64) {
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
    const uint32_t e = S.bits[r] & 3u;
    atomicAdd(&S.cnt[e], 1u);
    if (flr > 0) { atomicAdd(&S.rem[e], 1u); atomicMin(&S.fmin[e], flr); atomicMax(&S.fmax[e], flr); }
  }
  __syncthreads();

  // ---- 4. family gates (process_group :1329-1422, process_subgroup :1454-1646), as k_simplex_wave2 takes them ----------------------
  bool ok[3] = {false, false, false};
  uint32_t rej_insuf = 0, rej_zero = 0, rej_orphan = 0, rej_down = 0;
  bool bites = false, rank_rule = false;
  bool cand[3] = {false, false, false}, cut[3] = {false, false, false};   // the end reaches the cap / the cap bites on it
  uint32_t rem0[3] = {0, 0, 0};                              // retained reads of the end before the cut
  bool capped = false;
  for (uint32_t e = 0; e < 3; e++) {
    const uint32_t cnt = S.cnt[e], rem = S.rem[e];
    if (cnt == 0) continue;
    if (cnt < P.min_reads) { rej_insuf += cnt; continue; }
    rej_zero += cnt - rem;
    if (rem < P.min_reads) { rej_insuf += rem; continue; }
    if (rem == 0) continue;
    cand[e] = true; rem0[e] = rem;
    if (P.max_reads >= 0 && (long long)rem > P.max_reads) { cut[e] = true; capped = true; }
  }
  // --max-reads (downsample_filtered_source_reads :902-932, as k_family_wave<0> and k_family restate it): of an end above the cap the max_reads
  // lowest fgbio name ranks stay, ties in file order, and the survivors keep their file order.  A dropped read becomes a read of final length 0:
  // that is what "not retained" means to everything below (lengths, rows, UMIs, cell barcode, anchor), and its bytes stay where its mate's row
  // finds them.  (Workgroup-uniform: a caller without a cap, or one whose cap does not bite, runs nothing of this.)
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
      for (uint32_t e = 0; e < 3; e++) if (cut[e]) { S.rem[e] = 0; S.fmin[e] = 0xFFFFFFFFu; S.fmax[e] = 0; }
    __syncthreads();
    for (uint32_t r = tid, k = 0; r < n; r += DEEP_NT, k++) {
      const uint32_t e = S.bits[r] & 3u, fl = S.final_len[r];
      if (!cut[e] || fl == 0) continue;
      if ((drop >> k) & 1u) S.final_len[r] = 0;
      else { atomicAdd(&S.rem[e], 1u); atomicMin(&S.fmin[e], fl); atomicMax(&S.fmax[e], fl); }
    }
    __syncthreads();
  }
  for (uint32_t e = 0; e < 3; e++) {
    if (!cand[e]) continue;
    const uint32_t rem = S.rem[e];
    if (cut[e]) {
      rej_down += rem0[e] - rem;
      if (rem < P.min_reads) { rej_insuf += rem; continue; }   // (a cap below --min-reads)
      if (rem == 0) continue;
    }
    if (rem > 255u) { bites = true; continue; }             // (the per-chain observation counts of an item are bytes)
    ok[e] = true;
    if (S.fmin[e] != S.fmax[e] && P.min_reads > 1) rank_rule = true;
  }
  if (bites) { leave(); return; }
  // consensus length of an end: one final length → that; --min-reads 1 → the longest; else the min_reads-th longest (:1661-1669)
  if (rank_rule) {
    for (uint32_t r = tid; r < n; r += DEEP_NT) {
      const uint32_t e = S.bits[r] & 3u, fl = S.final_len[r];
      if (!ok[e] || fl == 0 || S.fmin[e] == S.fmax[e]) continue;
      uint32_t ge = 0;
      for (uint32_t j = 0; j < n; j++) ge += ((S.bits[j] & 3u) == e && S.final_len[j] >= fl) ? 1u : 0u;
      if (ge >= P.min_reads) atomicMax(&S.clen[e], fl);
    }
    __syncthreads();
  }
  uint32_t clen[3];
  for (uint32_t e = 0; e < 3; e++) clen[e] = !ok[e] ? 0u : (S.fmin[e] == S.fmax[e] || P.min_reads <= 1) ? S.fmax[e] : S.clen[e];
  const bool has_frag = ok[0], has_pair = ok[1] && ok[2];
  if (has_frag && has_pair) { leave(); return; }             // three consensus reads from one family: k_family
  if (!has_pair) { if (ok[1]) rej_orphan += S.rem[1]; else if (ok[2]) rej_orphan += S.rem[2]; }
  const uint32_t ne = has_frag ? 1u : has_pair ? 2u : 0u;
  const uint32_t type_a = has_frag ? 0u : 1u, end_a = has_frag ? 0u : 1u;
  const uint32_t m_a = ne ? S.rem[end_a] : 0u, m_b = ne == 2u ? S.rem[2] : 0u;
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
    if (S.wc[r]) { const uint32_t b = (uint32_t)S.partner[r]; mso = S.off[b] + S.seq_rel[b]; ml = S.l_seq[b]; }
    const bool hrx = (S.bits[r] & 8u) != 0;
    R.w[0] = (uint32_t)so; R.w[1] = (uint32_t)(so >> 32); R.w[2] = (uint32_t)mso; R.w[3] = (uint32_t)(mso >> 32);
    R.w[4] = (uint32_t)S.l_seq[r] | (fl << 16);
    R.w[5] = ml | ((uint32_t)S.wo[r] << 16);
    R.w[6] = (uint32_t)S.mo[r] | ((uint32_t)S.wc[r] << 16);
    R.w[7] = ((hrx ? (uint32_t)S.rx_rel[r] - (uint32_t)S.seq_rel[r] : 0u) & 0xFFFFu) | ((((S.bits[r] & 4u) ? 1u : 0u) | (hrx ? 2u : 0u)) << 16) | ((uint32_t)S.rx_len[r] << 24);
    D.rows[row0 + row] = R;
    if (hrx) { atomicAdd(&S.rxcnt[e], 1u); atomicMin(&S.rxfirst[e], r); }
  }
  __syncthreads();
  // UMIs of unequal length → consensus_umis panics → the general path reports it (vanilla_caller.rs:1842-1856)
  for (uint32_t r = tid; r < n; r += DEEP_NT) {
    const uint32_t e = S.bits[r] & 3u;
    if (!(S.bits[r] & 8u) || S.final_len[r] == 0 || S.rxfirst[e] == 0xFFFFFFFFu) continue;
    if (S.rx_len[r] != S.rx_len[S.rxfirst[e]]) S.rxbad = 1;
  }
  __syncthreads();
  if (ne) {
    const uint32_t eb = 2u;
    if (S.rxcnt[end_a] && S.rx_len[S.rxfirst[end_a]] > FAST_RX_CAP) S.rxbad = 1;
    if (ne == 2u && S.rxcnt[eb] && S.rx_len[S.rxfirst[eb]] > FAST_RX_CAP) S.rxbad = 1;
  }
  __syncthreads();
  if (S.rxbad) { leave(); return; }

  // ---- 6. the family's descriptor, and what the EndDescs hold that does not depend on the columns --------------------------------
  if (tid == 0) {
    DeepFam f;
    __builtin_memset(&f, 0, sizeof(f));
    f.status = 1; f.n = n; f.row0 = (uint32_t)row0;
    f.m_a = (uint16_t)m_a; f.m_b = (uint16_t)m_b; f.lc_a = (uint16_t)(ne ? clen[end_a] : 0u); f.lc_b = (uint16_t)(ne == 2u ? clen[2] : 0u);
    f.ne = (uint8_t)ne; f.type_a = (uint8_t)type_a;
    f.rx_cnt_a = (uint16_t)(ne ? S.rxcnt[end_a] : 0u); f.rx_cnt_b = (uint16_t)(ne == 2u ? S.rxcnt[2] : 0u);
    f.rx_len_a = (uint8_t)((ne && S.rxcnt[end_a]) ? S.rx_len[S.rxfirst[end_a]] : 0u);
    f.rx_len_b = (uint8_t)((ne == 2u && S.rxcnt[2]) ? S.rx_len[S.rxfirst[2]] : 0u);
    f.rej_insuf = rej_insuf; f.rej_zero = rej_zero; f.rej_orphan = rej_orphan; f.rej_down = rej_down;
    f.ov_agree = S.ov_agree; f.ov_dis = S.ov_dis; f.ov_corr = S.ov_corr;
    if constexpr (CLIPS != 0) {
      f.clipped = S.multi;
      if (S.multi && !P.meth_mode) atomicAdd(deep_clipped_counter(P), 1u);   // (FGX_DEEP_CLIPS=1; no leave() behind this point.  The mode counts in k_deep_cols<1>)
    }
    if (P.meth_mode && P.genome) {
      auto top_of = [&](uint32_t r) { return ((S.bits[r] & 4u) != 0) == ((S.bits[r] & 32u) != 0); };   // is_top_strand (methylation.rs:392-398): reverse == LAST
      for (uint32_t k = 0; k < ne; k++) {
        const uint32_t e = k == 0 ? end_a : 2u;
        int a = -1, first = -1;
        for (uint32_t r = 0; r < n; r++) {
          if ((S.bits[r] & 3u) != e || S.final_len[r] == 0) continue;
          if (first < 0) first = (int)r;
          if (a < 0 || S.final_len[r] >= S.final_len[(uint32_t)a]) a = (int)r;       // max_by_key: the last of the longest
        }
        if (a < 0) continue;
        const uint32_t ua = (uint32_t)a;
        const bool rv = (S.bits[ua] & 4u) != 0;
        bool placed = S.ref_id[ua] >= 0 && S.pos[ua] >= 0 && (uint32_t)S.ref_id[ua] < P.n_ref;
        uint32_t contig = (uint32_t)S.ref_id[ua];
        if constexpr (CLIPS != 0) {                          // (the builds of the mode) a canonical batch: the record no longer lies where it says — its runs name the contig
          const unsigned long long tab = P.contig_len[P.n_ref];
          if (tab) {
            const int32_t rid = ((const canon::RefRuns*)(uintptr_t)tab)[r0 + ua].ref_id;      // the ORIGINAL reference id; -1: the record had no position
            placed = rid >= 0 && (uint32_t)rid < P.n_ref;
            contig = (uint32_t)rid;
            f.a_rec[k] = r0 + ua + 1u;
          }
        }
        // query_to_ref_positions (methylation.rs:116-184) on the ONE M op the reference makes of the read: a forward anchor's column p lies at pos + p —
        // a leading clip shifts the lookup, as it does there —, a reverse anchor's at pos + T - 1 - p, T = the lengths of all its ops (l_seq when it
        // is one op; with hard clips more than l_seq)
        if constexpr (CLIPS != 0) f.a_ref0[k] = rv ? S.pos[ua] + (int32_t)S.tot[ua] - 1 : S.pos[ua];
        else f.a_ref0[k] = rv ? S.pos[ua] + (int32_t)S.l_seq[ua] - 1 : S.pos[ua];
        f.a_info[k] = (placed ? (contig & 0x0FFFFFFFu) | (1u << 28) : 0u) | (rv ? 1u << 29 : 0u) | (top_of(ua) ? 1u << 30 : 0u) | (top_of((uint32_t)first) ? 1u << 31 : 0u);
      }
    }
    *F = f;
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
      const uint32_t aux_off = (uint32_t)S.seq_rel[0] + ((l_seq0 + 1u) >> 1) + l_seq0;      // (seq_rel: behind the name and the CIGAR — one op, or none of an unmapped record)
      aux_walk(rec0, sTagCls, aux_off, P.rec_len[r0] - aux_off, P, ax);
    }
    E->col_off = P.col_base[g] + (k == 0 ? 0u : clen[end_a]);
    E->cons_len = clen[e];
    E->first_off = S.off[0]; E->kept_off = S.off[fk];
    E->type = (uint8_t)e;
    E->mi_off = (uint16_t)(ax.pk_mi & 0xFFFF); E->mi_len = (uint8_t)(ax.pk_mi >> 16);
    const bool hcb = P.cell0 && (S.bits[fk] & 16u);
    E->has_cb = hcb ? 1 : 0; E->cb_off = S.cb_rel[fk]; E->cb_len = S.cb_len[fk];
    E->has_rx = S.rxcnt[e] > 0; E->rx_len = (uint8_t)(S.rxcnt[e] ? S.rx_len[S.rxfirst[e]] : 0u);
    E->rec_size = 0; E->valid = 0;                           // k_deep_cols: the sizes of the cD / cM values depend on the depths
    E->meth = 0;                                             // (k_deep_cols<1> sets it)
  }
}

// -----------------------------------------------------------------------------------------------------------------------------
// k_deep_cols — wavefront = family, lane = column, rows streamed from global memory
// -----------------------------------------------------------------------------------------------------------------------------
#ifndef FGX_DEEP_OCC
#define FGX_DEEP_OCC 8
#endif
#ifndef FGX_DEEP_BATCH
#define FGX_DEEP_BATCH 4   /* rows whose loads are in flight together */
#endif
template <int METH>   // 1: the methylation-aware mode — reference lookup per column, unconverted / converted counts, converted bases read as unconverted
__global__ __launch_bounds__(256, FGX_DEEP_OCC) void k_deep_cols(FastParams P, DeepParams D) {
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
  const uint64_t col_base = uniform_u64(P.col_base[g]);
  uint8_t* const fam_code = P.col_code + col_base;
  uint8_t* const fam_qual = P.col_qual + col_base;
  uint16_t* const fam_depth = P.col_depth + col_base;
  uint16_t* const fam_err = P.col_err + col_base;
  const uint8_t* const pairs = (const uint8_t*)&sL.pair[0][0];
  const uint8_t* const blob = P.blob;
  const uint32_t min_bq = uni((uint32_t)P.min_input_bq & 0xFFu);
  const DeviceTables* T = P.T;
  const uint32_t my_list = blockIdx.x & (N_LISTS - 1);
  bool list_overflow = false;
  auto push_item = [&](bool need, uint64_t dest, const double* ll, uint32_t obs_packed, uint32_t chains) {   // an item straight into one of the global lists
    list_overflow |= push_full_global(P, lane, my_list, need, dest, ll, obs_packed, chains);
  };
  // The rows of an end are read through the scalar unit (constant address space: one s_load_dwordx8 per row, its fields in scalar registers —
  // every address below is `scalar base + this lane's index`); k_deep_parse wrote them, a kernel boundary ago.
  typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
  typedef const FGX_CONST_AS u32x8* RowPtr;
  auto row_seq = [&](const u32x8& r) { return blob + (((unsigned long long)r[1] << 32) | r[0]); };
  auto row_mate = [&](const u32x8& r) { return blob + (((unsigned long long)r[3] << 32) | r[2]); };

  uint32_t maxd[2] = {0, 0}, mind[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
  uint32_t row_base = 0, coff = 0;
#pragma unroll 1
  for (uint32_t k = 0; k < ne; k++) {
    const uint32_t m = m_k[k], Lc = lc_k[k];
    const RowPtr er = (RowPtr)(rows + row_base);
    uint32_t lmax = 0, lmin = 0xFFFFFFFFu;
    // methylation-aware mode: where the end's columns lie on the reference (the anchor read's), which read base is the unconverted cytosine
    // of the call's strand (C, top strand; G otherwise) and which the converted one (T / A) — as 4-bit codes in consensus orientation
    const uint32_t ainfo = METH ? uni(Fp->a_info[k]) : 0u;
    const bool annotated = METH && ((ainfo >> 28) & 1u);
    const int32_t aref0 = METH ? (int32_t)uni((uint32_t)Fp->a_ref0[k]) : 0;
    const bool atop = (ainfo >> 30) & 1u;
    const uint32_t tcode = atop ? 2u : 4u, vcode = atop ? 8u : 1u, target = atop ? (uint32_t)'C' : (uint32_t)'G';
    unsigned long long g_off = 0, g_len = 0;
    if (annotated) { g_off = uniform_u64(P.contig_off[ainfo & 0x0FFFFFFFu]); g_len = uniform_u64(P.contig_len[ainfo & 0x0FFFFFFFu]); }
    // a canonical batch (FGX_METH_CANON=1): the anchor's reference runs instead of the one run from a_ref0 — the anchor is wave-uniform, so are its runs:
    // scalar loads, a loop of uniform trip count; a column outside every run (an insertion) is no reference cytosine
    const uint32_t arec = METH ? uni(Fp->a_rec[k]) : 0u;
    RefRunsPtr a_runs = nullptr;
    uint32_t a_nruns = 0;
    if (arec) { a_runs = meth_ref_runs(P, arec - 1u); if (a_runs) a_nruns = uni(a_runs[1]) & 0xFFu; }
    auto ref_is_c = [&](uint32_t p) -> bool {
      if (!annotated) return false;
      long long rp = (long long)aref0 + (((ainfo >> 29) & 1u) ? -(long long)p : (long long)p);
      if (a_runs) {
        rp = -1;
        for (uint32_t r = 0; r < a_nruns; r++) {
          const uint32_t q0 = a_runs[2 + 4 * r], rl = a_runs[3 + 4 * r];
          const long long f0 = (long long)(((unsigned long long)a_runs[5 + 4 * r] << 32) | a_runs[4 + 4 * r]);
          const uint32_t d = p - q0;
          if (p >= q0 && d < rl) rp = ((ainfo >> 29) & 1u) ? f0 - (long long)d : f0 + (long long)d;
        }
      }
      if (rp < 0 || (unsigned long long)rp >= g_len) return false;
      uint32_t rb = P.genome[g_off + (unsigned long long)rp];
      if (rb >= 'a' && rb <= 'z') rb -= 32;
      return rb == target;
    };
    if (m == 1) {   // single-read consensus: LUT keyed by the unclamped quality (:1677-1708)
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
        if constexpr (METH != 0) {
          const bool is_c = ref_is_c(p);
          uint32_t mu = 0, mt = 0;
          if (is_c) { if (code == tcode) mu = 1; else if (code == vcode) { mt = 1; code = tcode; } }
          const uint64_t oo = col_base + coff + p;
          P.meth_flag[oo] = is_c ? 1 : 0; P.meth_u[oo] = (uint16_t)mu; P.meth_t[oo] = (uint16_t)mt;
        }
        const uint8_t adj = qq < 94 ? T->single_input_quals[qq] : 0;
        uint8_t ob, oq;
        if (adj < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; } else { ob = (uint8_t)code; oq = adj; }
        const uint32_t oc = coff + p, dd = code != 15 ? 1u : 0u;
        fam_code[oc] = ob; fam_qual[oc] = oq; fam_depth[oc] = (uint16_t)dd; fam_err[oc] = 0;
        lmax = dd > lmax ? dd : lmax; lmin = dd < lmin ? dd : lmin;
      }
    } else {
      for (uint32_t p0 = 0; p0 < Lc; p0 += 64) {
        const uint32_t p0s = uni(p0);
        const uint32_t p = p0s + lane;
        const bool incol = p < Lc;
        const uint32_t shp = (~p & 1u) << 2;                   // nibble shift of an even / odd index (a reverse read of even length flips it)
        const bool is_c = METH && incol && ref_is_c(p);
        uint32_t mu = 0, mt = 0;
        // Kahan chains by order of appearance (ChainAcc, consensus_math.h), all four updated by every observation: the column of a deep
        // family shows a second base more often than not, and a wavefront that keeps a two-chain path beside the four-chain one executes both
        // (chains 2 / 3 hold nothing of value until opened: a new base opens its chain as a copy of chain R, base_builder.rs:836-868)
        double s1 = 0.0, c1 = 0.0, s2 = 0.0, c2k = 0.0, s3 = 0.0, c3 = 0.0, sR = 0.0, cR = 0.0;
        uint32_t b1 = 0, b2 = 0, b3 = 0, cnt4 = 0;          // cnt4: observations of chains 1, 2, 3, R — a byte each (an end holds at most 255 reads)
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
            const uint32_t lim = fin < Lc ? fin : Lc;          // inside the read's final length AND a column of the consensus
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
            if constexpr (METH != 0) {                       // annotate_simplex_methylation + the normalisation (methylation.rs:193-242, vanilla_caller.rs:781-860)
              if (is_c && in_[t] && q >= min_bq) { if (c == tcode) mu++; else if (c == vcode) { mt++; c = tcode; } }
            }
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
              cnt4 += h1 ? 1u : h2 ? 0x100u : h3 ? 0x10000u : 0x1000000u;
            }
          }
        }
        // ---- call (k_simplex_wave2's) ----
        const uint32_t oc = coff + p;
        if constexpr (METH != 0) { if (incol) { const uint64_t oo = col_base + oc; P.meth_flag[oo] = is_c ? 1 : 0; P.meth_u[oo] = (uint16_t)mu; P.meth_t[oo] = (uint16_t)mt; } }
        const uint32_t n1 = cnt4 & 0xFF, depth = n1 + ((cnt4 >> 8) & 0xFF) + ((cnt4 >> 16) & 0xFF) + (cnt4 >> 24);
        bool need_full = false, resolved = true;
        uint32_t q_call = FGX_MIN_PHRED, code_call = 15;
        if (incol) {
          if (b2 != 0) resolved = false;                     // two or more distinct bases: never the unanimous fast path
          else if (n1 != 0) {
            uint32_t qq = 0;
            CallConst KC;
            KC.cap = sT.cap; KC.cap_threshold = sT.cap_threshold; KC.half_cerr_at_cap = sT.half_cerr_at_cap;
            resolved = unanimous_call_lds(sT, P.T->t.cerr_min, KC, s1, sR, &qq);
            if (resolved) { q_call = qq; code_call = b1; }
          }
          need_full = !resolved;
          fam_depth[oc] = (uint16_t)depth;                   // (at most 255 member reads: no saturation to apply)
          lmax = depth > lmax ? depth : lmax; lmin = depth < lmin ? depth : lmin;
        }
        {
          const double chain[4] = {s1, s2, s3, sR};
          push_item(need_full, col_base + oc, chain, cnt4, b1 | (b2 << 4) | (b3 << 8));
        }
        if (incol && resolved) {
          uint8_t ob, oq;
          if (depth < P.min_reads) { ob = 15; oq = 0; }
          else if (q_call < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; }
          else { ob = (uint8_t)code_call; oq = (uint8_t)q_call; }
          fam_code[oc] = ob; fam_qual[oc] = oq; fam_err[oc] = 0;
        }
      }
    }
    maxd[k] = uni(wave_max(lmax)); mind[k] = uni(wave_min(lmin));
    row_base += m; coff += Lc;
  }

  // ---- consensus UMI per end (simple_umi.rs:46-117): lane = character --------------------------------------------------------------
  const DeviceTables* TU = P.TU;
  char my_rx[2] = {0, 0};
  bool rx_bad = false;
  row_base = 0;
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
    bool need_full = false;
    if (rx_cnt == 1) { if (mychar) my_rx[k] = (char)fc; }    // one read = its bytes
    else if (!__any(mychar && !all_same)) {                  // every retained read carries the same value: normalised (A C G T N upper case)
      if (mychar) { const uint32_t ch = fc, up = ch & 0xDFu, idx = up - 'A'; const bool dna = idx < 26 && ((0x00082045u >> idx) & 1u); my_rx[k] = (char)(dna ? up : ch); }
    } else if (mychar) {
      if (non_dna == 0) {
        int bi; uint8_t q;
        CallConst KU;
        KU.cap = TU->t.cap; KU.cap_threshold = TU->t.cap_threshold; KU.half_cerr_at_cap = TU->t.half_cerr_at_cap;
        const bool resolved = column_call_fast_lds(TU->t, KU, acc.s, acc.obs, &bi, &q);
        my_rx[k] = bi >= 0 ? "ACGT"[bi] : 'N';
        need_full = !resolved;
      } else if (non_dna == seenu && !mixed) my_rx[k] = (char)fc;
      else rx_bad = true;
    }
    if (!mychar) { need_full = false; }
    const uint32_t e = k == 0 ? type_a : 2u;
    if (acc.obs[0] > 255u || acc.obs[1] > 255u || acc.obs[2] > 255u || acc.obs[3] > 255u) rx_bad = rx_bad || need_full;
    push_item(need_full, (1ull << 63) | ((uint64_t)(slot0 + e) << 8) | lane, acc.s, acc.obs[0] | (acc.obs[1] << 8) | (acc.obs[2] << 16) | (acc.obs[3] << 24), 0u);
  }
  if (__any(rx_bad) || __any(list_overflow)) {               // the general path redoes the family (nothing was counted, no record size is set)
    if (lane == 0) { const uint32_t kk = atomicAdd(P.n_deferred, 1u); P.deferred[kk] = g; }
    return;
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
      if constexpr (METH != 0) { const uint32_t ai = Fp->a_info[k]; E->meth = (uint8_t)(((ai >> 28) & 1u) | ((ai >> 31) << 1)); }
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
    if constexpr (METH != 0) { if (Fp->clipped) atomicAdd(meth_clipped_counter(P), 1u); }
  }
}


// -----------------------------------------------------------------------------------------------------------------------------
// methylation-aware mode: the tags that follow RX — MM / ML (build_mm_ml_tags, methylation.rs:264-343) and cu / ct
// (vanilla_caller.rs:1853-1876).  Their size depends on the FINAL consensus bases (k_call_full's included): k_meth_sizes runs after it and
// adds them to the record sizes before the scan; k_meth_tail writes them behind what k_emit wrote.  A thread per record: the MM string is
// a sequential scan of the record's cytosines (a consensus BAM has an eighth of the raw reads).
// -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t meth_digits(uint32_t v) { return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : 6u; }
// One 64-column chunk of a record's MM / ML scan (lane = column): `tracked` = the consensus base is the strand's cytosine, `hit` = such a
// base with methylation evidence (an MM entry: "," + the number of tracked bases skipped since the previous entry).  Returns this lane's
// skip count (meaningful on hit lanes) and keeps `carry` = tracked bases without evidence since the last entry, across chunks.
__device__ __forceinline__ uint32_t meth_chunk_skip(uint32_t lane, bool tracked, bool hit, uint32_t& carry, unsigned long long& hit_mask) {
  const unsigned long long mt = __ballot(tracked && !hit), mh = __ballot(hit);
  const unsigned long long below = (1ull << lane) - 1ull;
  const unsigned long long prev = mh & below;                                 // entries before this lane in the chunk
  uint32_t skip;
  if (prev) { const uint32_t p = 63u - (uint32_t)__clzll((long long)prev); skip = (uint32_t)__popcll(mt & below & ~((2ull << p) - 1ull)); }
  else skip = carry + (uint32_t)__popcll(mt & below);
  if (mh) { const uint32_t last = 63u - (uint32_t)__clzll((long long)mh); carry = (uint32_t)__popcll(last == 63u ? 0ull : (mt >> (last + 1))); }
  else carry += (uint32_t)__popcll(mt);
  hit_mask = mh;
  return skip;
}
// A wavefront per record (slot); 64 columns per step.
__global__ __launch_bounds__(256) void k_meth_sizes(FastParams P, uint32_t n_slots, MethSlot* __restrict__ ms) {
  const uint32_t slot = uni((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (slot >= n_slots) return;
  MethSlot r; r.std_size = 0; r.n_ml = 0; r.mm_len = 0; r._pad = 0;
  if (P.rec_sizes[slot] != 0) {
    EndDesc* const E = &P.ends[slot];
    r.std_size = uni(E->rec_size);
    const uint32_t meth = uni(E->meth);
    if (uni(E->valid) && (meth & 1u)) {
      const uint32_t track = (meth & 2u) ? 2u : 4u, n = uni(E->cons_len);
      const uint64_t co = uniform_u64(E->col_off);
      uint32_t carry = 0, mm = 0;
      for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + lane;
        const bool in = i < n;
        const bool tracked = in && (uint32_t)P.col_code[co + (in ? i : 0u)] == track;
        const bool hit = tracked && P.meth_flag[co + i] && ((uint32_t)P.meth_u[co + i] + P.meth_t[co + i]) > 0;
        unsigned long long mh;
        const uint32_t skip = meth_chunk_skip(lane, tracked, hit, carry, mh);
        r.n_ml += (uint32_t)__popcll(mh);
        mm += hit ? 1u + meth_digits(skip) : 0u;
      }
      r.mm_len = uni(wave_sum(mm));
      uint32_t extra = 2u * (8u + 2u * n);                                     // cu, ct: B:s arrays
      if (r.n_ml) extra += (3u + 3u + r.mm_len + 1u + 1u) + (8u + r.n_ml);      // MM:Z:<C+m|G-m>,..; NUL and ML:B:C
      if (lane == 0) { E->rec_size = r.std_size + extra; P.rec_sizes[slot] = (uint64_t)(r.std_size + extra) + 4; }
    }
  }
  if (lane == 0) ms[slot] = r;
}
__global__ __launch_bounds__(256) void k_meth_tail(FastParams P, uint32_t n_slots, const MethSlot* __restrict__ ms, const uint64_t* __restrict__ out_off, uint8_t* __restrict__ out) {
  const uint32_t slot = uni((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (slot >= n_slots || P.rec_sizes[slot] == 0) return;
  const EndDesc& E = P.ends[slot];
  const uint32_t meth = uni(E.meth);
  if (!uni(E.valid) || !(meth & 1u)) return;
  const uint32_t std_size = uni(ms[slot].std_size), n_ml = uni(ms[slot].n_ml), mm_len = uni(ms[slot].mm_len);
  uint8_t* q = out + uniform_u64(out_off[slot]) + 4 + std_size;
  const bool top = (meth & 2u) != 0;
  const uint32_t track = top ? 2u : 4u, n = uni(E.cons_len);
  const uint64_t co = uniform_u64(E.col_off);
  if (n_ml) {
    uint8_t* const mmq = q + 6;                                                // the MM entries
    uint8_t* const ml = q + 3 + 3 + mm_len + 2;                                // the ML tag, behind MM's ";" and NUL
    if (lane < 6) q[lane] = lane == 0 ? 'M' : lane == 1 ? 'M' : lane == 2 ? 'Z' : lane == 3 ? (top ? 'C' : 'G') : lane == 4 ? (top ? '+' : '-') : 'm';
    if (lane < 8) ml[lane] = lane == 0 ? 'M' : lane == 1 ? 'L' : lane == 2 ? 'B' : lane == 3 ? 'C' : (uint8_t)(n_ml >> (8 * (lane - 4)));
    uint32_t carry = 0, ml_base = 0, mm_base = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
      const uint32_t i = i0 + lane;
      const bool in = i < n;
      const bool tracked = in && (uint32_t)P.col_code[co + (in ? i : 0u)] == track;
      const uint32_t u = in ? P.meth_u[co + i] : 0u, t = in ? P.meth_t[co + i] : 0u;
      const bool hit = tracked && P.meth_flag[co + i] && (u + t) > 0;
      unsigned long long mh;
      const uint32_t skip = meth_chunk_skip(lane, tracked, hit, carry, mh);
      const uint32_t nd = meth_digits(skip), mine = hit ? 1u + nd : 0u;
      uint32_t incl = mine;                                                     // inclusive prefix sum of the entries' lengths over the wavefront
      for (int o = 1; o < 64; o <<= 1) { const uint32_t v = (uint32_t)__shfl_up((int)incl, o); if ((int)lane >= o) incl += v; }
      if (hit) {
        const uint32_t total = u + t, num = P.meth_mode == FGX_METHYLATION_EM_SEQ ? u : t;     // EM-Seq: unconverted / total; TAPs: converted / total
        const uint32_t pr = num * 255u / total;
        ml[8 + ml_base + (uint32_t)__popcll(mh & ((1ull << lane) - 1ull))] = (uint8_t)(pr > 255u ? 255u : pr);
        uint8_t* e = mmq + mm_base + (incl - mine);
        *e++ = ',';
        uint32_t v = skip;
        for (uint32_t d = nd; d-- > 0;) { e[d] = (uint8_t)('0' + v % 10u); v /= 10u; }
      }
      ml_base += (uint32_t)__popcll(mh);
      mm_base += uni((uint32_t)__shfl((int)incl, 63));
    }
    if (lane == 0) { mmq[mm_len] = ';'; mmq[mm_len + 1] = 0; }
    q = ml + 8 + n_ml;
  }
  for (int a = 0; a < 2; a++) {
    if (lane < 8) q[lane] = lane == 0 ? 'c' : lane == 1 ? (a == 0 ? 'u' : 't') : lane == 2 ? 'B' : lane == 3 ? 's' : (uint8_t)(n >> (8 * (lane - 4)));
    const uint16_t* src = (a == 0 ? P.meth_u : P.meth_t) + co;
    for (uint32_t i = lane; i < n; i += 64) { const uint32_t v = src[i]; q[8 + 2 * i] = (uint8_t)v; q[9 + 2 * i] = (uint8_t)(v >> 8); }
    q += 8 + 2 * n;
  }
}
// every family of the batch on the list (methylation-aware mode: the streaming kernels are the whole pipeline)
__global__ void k_iota(uint32_t* __restrict__ list, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) list[i] = i;
}
