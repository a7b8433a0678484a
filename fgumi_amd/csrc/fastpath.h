// fastpath.h — declarations for the device-resident simplex pipeline (fastpath.hip).
#pragma once
#include <algorithm>
#include "engine.h"
#include "canon_core.h"

// (small rules shared by kernels and host code)
#if defined(__HIPCC__)
#define FP_HD __host__ __device__ __forceinline__
#else
#define FP_HD inline
#endif

namespace fgx {

// the canonical pass's parameters out of a caller's options (api.cpp; the debug entry of canon_deep.inc)
inline canon::Params canon_params_of(const fgx_options* o) {
  canon::Params P;
  P.min_bq = o->min_input_base_quality; P.overlapping = o->overlapping_consensus; P.trim = o->trim; P._pad = 0;
  P.min_total = o->duplex_min_reads[0]; P.min_xy = o->duplex_min_reads[1]; P.min_yx = o->duplex_min_reads[2];
  P.max_reads_per_strand = o->duplex_max_reads_per_strand;
  P.cell_tag[0] = o->cell_tag[0]; P.cell_tag[1] = o->cell_tag[1]; P._pad2[0] = P._pad2[1] = 0;
  return P;
}
// FGX_DEEP_INDELS=1 (canon_deep.inc; the kernel lives in the fastpath.hip translation unit): the canonical form of the deferred duplex molecules of 65 .. 512 records, a
// workgroup per molecule.  Same arrays as launch_canon_molecules (canon_device.hip), which calls it behind its lane kernel; molecules of up to 64 records are skipped.
void launch_canon_duplex_deep(hipStream_t s, const canon::Params& P, const uint8_t* d_blob, const uint64_t* d_rec_off, const uint32_t* d_rec_len, const uint32_t* d_grp_first,
                              const uint32_t* d_def, uint32_t nd, const uint64_t* d_first, uint8_t* d_out, const uint64_t* d_out_off, uint32_t* d_out_len, int* d_status,
                              canon::Delta* d_delta);

constexpr int FAST_RX_CAP = 48;   // longest RX value handled on the device (longer → general path)

struct EndDesc {            // one consensus read (a family end), written by the family kernels, consumed by k_emit
  uint64_t col_off;         // first column in the per-position arrays
  uint64_t first_off;       // blob offset (record body) of the first record of the MI group: MI value → read name + MI tag
  uint64_t kept_off;        // blob offset of the first retained source read: cell-barcode tag
                            // (offsets, not record indices: k_emit goes from the descriptor straight to the bytes, one dependent
                            // memory round trip less per record)
  uint32_t cons_len;
  uint32_t rec_size;        // BAM block_size of the record to emit
  uint16_t mi_off, cb_off;
  uint8_t mi_len, cb_len, rx_len, type;   // type: 0 fragment, 1 R1, 2 R2
  uint8_t has_cb, has_rx, valid, meth;   // meth (methylation-aware mode): bit 0 the call was annotated (cu / ct, MM / ML follow RX), bit 1 the MM / ML strand is the top strand
  char rx[FAST_RX_CAP];
};
// methylation-aware mode: what k_meth_sizes found for a record — the bytes of the standard record (the methylation tags follow them), ML entries, characters of the MM entries
struct MethSlot { uint32_t std_size, n_ml, mm_len, _pad; };

struct DuplexDesc {         // one duplex consensus record (slot 3g+1 = R1, 3g+2 = R2), written by k_family_wave<1>, consumed by k_emit_duplex
  uint64_t a_off, b_off;    // first column of the AB-side strand and of the BA-side strand (b = a when a single strand is passed through)
  uint32_t len;             // record length: the paired span of both strands, or the whole lone strand
  uint32_t first_rec;       // first paired record of the molecule (MI value → read name + MI tag, minus the /A|/B suffix)
  uint32_t cb_rec;          // first /A (else /B) record: cell-barcode source
  uint32_t rec_size;
  uint16_t mi_off, cb_off;
  uint8_t mi_len, cb_len, rx_len, type;
  uint8_t has_cb, has_rx, valid, has_ba;
  char rx[FAST_RX_CAP];
  uint8_t meth;             // methylation-aware mode (k_family_wave<1, 1> and <1, 1, 1>; in what was padding): bit 0 the AB-side strand's call was annotated, bit 1 the BA-side
                            // strand's, bit 2 a lone strand passed through is the BA one (is_ba_only: its tags are bm / bu / bt and its MM strand is G-m)
  uint8_t capped;           // --max-reads-per-strand bit a read set of the molecule (k_family_wave<1, 0, 1> and <1, 1, 1>; padding too): the duplex error recount (cE / ce) reads the
                            // counts over ALL source reads from col_obs_all, col_obs holds the counts of the scoring reads (depths)
};
static_assert(sizeof(DuplexDesc) == 96, "DuplexDesc: the methylation byte and the cap flag lie in the padding");
// methylation-aware mode, duplex: what k_duplex_meth_sizes found for a record — the bytes of the standard record (the methylation tags follow them) and per
// MM string (0 the AB-side strand's am / bm, 1 the BA-side strand's bm, 2 the duplex MM) its entries and the characters of its entries
struct DuplexMethSlot { uint32_t std_size, n_hit[3], mm_len[3], _pad; };

struct CodecDesc {          // one CODEC consensus record (slot 3g+1), written by k_family_wave<2>, consumed by k_emit_codec
  uint64_t s1_off, s2_off;  // R1-strand and R2-strand single-strand column segments (read orientation)
  uint32_t l1, l2, cons_len;
  uint32_t first_rec, cb_rec, rec_size;
  uint16_t mi_off, cb_off;
  uint8_t mi_len, cb_len, rx_len, flags;   // flags: bit 0 = longest R1 on the reverse strand, bit 1 = longest R2 on the reverse strand
  uint8_t has_cb, has_rx, valid, _pad;
  char rx[FAST_RX_CAP];
};

struct FullItem {           // a column (or UMI character) whose call needs the full log-sum-exp chain
  uint64_t dest;            // bit 63 clear: scratch column index; set: (slot << 8 | char index) of an RX character
  double ll[4];             // chains == 0: log-likelihoods of A, C, G, T; else: Kahan chains 1, 2, 3 and R as the kernel holds them
  uint32_t obs;             // observation counts, one byte each, in the order of ll
  uint32_t chains;          // 0, or the one-hot BAM codes of chains 1 | 2 << 4 | 3 << 8 (0 = chain not opened); every other base reads chain R
};
constexpr int N_LISTS = 1024;
// LDS slice of a wavefront in the FIRST k_split_cols launch of a batch (choose_split_build, fastpath.hip): the MEAN family's tile — rows of
// 160 + 80 bytes, 16 bytes of slack — and room behind it: in the packed build for the 8-byte descriptors of the columns the pass does not answer
// itself and the FullItems of those that need k_call_full (56 bytes per such column, ~14 flagged columns and 3.3 items per depth-8 family of
// `simulate` data); at least the slice of a 16-record family.  A family whose flagged columns and items do not fit takes the next launch.
// The packed build's 5632 bytes — 1776 of room at depth 8 — are seven workgroups of four wavefronts in a CU's 160 KB.  5024 bytes (1168 of
// room: an eighth workgroup, which the packed kernel's registers allow) were measured and NOT taken — profiles/cols_scalar_state.md: 0.29 ms
// of 26.4 less per depth-8 step, but 18 families of 5 M sent to the second launch where there were none, and a long-tail batch, whose families of
// 20 and 21 records then miss the first slice, 8 ms of 68 slower.
constexpr uint32_t S2_ROW_BYTES = 240, S2_TILE_SLACK = 16, S2_ROOM_PACKED = 1680, S2_ROOM_CLASSIC = 400, S2_SLICE16_PACKED = 5632, S2_SLICE16_CLASSIC = 4352,
                   S2_FLAG_DESC_BYTES = 8;
inline uint32_t s2_tile_bytes(double mean_recs) { return (uint32_t)(mean_recs + 0.999) * S2_ROW_BYTES + S2_TILE_SLACK; }
inline uint32_t s2_first_slice_bytes(double mean_recs, bool packed) {
  const uint32_t floor16 = packed ? S2_SLICE16_PACKED : S2_SLICE16_CLASSIC;
  const uint32_t mean_need = s2_tile_bytes(mean_recs) + (packed ? S2_ROOM_PACKED : S2_ROOM_CLASSIC);
  return mean_need > floor16 ? std::min<uint32_t>((mean_need + 15u) & ~15u, 17408u) : floor16;
}
// FullItem.chains with this bit set: the column did not stay with one base — `ll` holds its observations instead of chains,
// 16-bit each (4-bit code in consensus orientation << 8 | quality), chains & 0xFF of them in file order (at most 16);
// k_call_full accumulates them with the four-lane Kahan loop (base_builder.rs:836-868) and calls the column
constexpr uint32_t FULL_ITEM_OBS = 0x80000000u;
// A column of more than 16 observations (an end of up to 64 reads) takes ceil(m / 16) CONSECUTIVE items of one list: the head item as above
// with m = chains & 0xFF, then continuation items — chains == FULL_ITEM_CONT, observations 16 .. in `ll` again — which k_call_full's own
// threads skip.  (A family's items stay in one list when it holds such a column: k_split_cols pads a list's tail with continuation items.)
constexpr uint32_t FULL_ITEM_CONT = 0x40000000u;

// ---- k_call_full's answers for the pair writer (FGX_FULL_RESULTS, on by default) ---------------------------------------------------------
// The answer to an item is six bytes that ONE kernel reads: k_emit, which holds the family's columns in registers a moment later.  For a
// family the packed build of k_split_cols finished and emit_pair will write (full_results_family below), k_call_full leaves the answer in
// slot `list * full_cap + i` of an array beside the item pool — one coalesced 8-byte store — instead of four sub-dword stores into scratch
// planes whose lines left the cache milliseconds ago, and emit_pair patches the family's few answers into its registers.
//   k_split_cols (packed build, scratch path) writes the family's index + 1 into the `obs` word of its observation and continuation items
//                and {first slot, items, in one piece} into the 64-bit word `col_off` of the family's FRAGMENT EndDesc (slot 3g: no record
//                of a pair family, copied to LDS by k_emit with the other two);
//   k_split_finish decides with full_results_family and writes the family's byte of `full_flag` (cleared per batch);
//   k_call_full reads that byte through the item's family index; every other item is scattered into the planes as before;
//   k_emit     reads the same byte and, when set, lets emit_pair load and apply the family's results.
struct FullResult {
  uint32_t w0;              // low 16 bits of the scratch column index | code << 16 | quality << 24 (code FULL_RESULT_NONE: a continuation item's slot)
  uint32_t w1;              // errors (<= 32767) | depth << 16
};
static_assert(sizeof(FullResult) == 8, "a result is one 8-byte store");
constexpr uint32_t FULL_RESULT_NONE = 0xFFu;
constexpr uint32_t FULL_RESULT_MAX_ITEMS = 64;   // a lane of the writer's wavefront per result
// the default of the switch FGX_FULL_RESULTS (1: on unless FGX_FULL_RESULTS=0; 0: on only with FGX_FULL_RESULTS=1)
#ifndef FGX_FULL_RESULTS_DEFAULT
#define FGX_FULL_RESULTS_DEFAULT 1
#endif
// counters of the path (fgx_debug_last_full_results), spread over STAT_SLOTS slots of FULL_STATS_STRIDE words: [0] column answers through the array, [1] column answers
// scattered, [2] families the writer applies, [3] families refused because their items are not in one piece, [4] families refused because they hold more than 64 items
// ([5 .. 8) of a slot: k_split_finish's counters of the packed overlap step — packed, byte-wise, of those voted out by the guard)
constexpr int FULL_STATS_N = 5, FULL_STATS_STRIDE = 8, OV_STATS_N = 3;
static_assert(FULL_STATS_N + OV_STATS_N <= FULL_STATS_STRIDE, "the overlap counters share the slots of the result counters");
// the family's word in its fragment EndDesc: first slot | items << 32 | (in one piece) << 48
FP_HD uint64_t full_range_word(uint32_t first, uint32_t items, bool whole) {
  return (uint64_t)first | ((uint64_t)(items < 0xFFFFu ? items : 0xFFFFu) << 32) | ((uint64_t)(whole ? 1u : 0u) << 48);
}
// Where a family's items went when `items` of them were reserved at `base` of a list of `cap` slots (s2_cols_family phase 7): in one piece
// iff the reservation lies inside the list.  (A family with a column of several items never cuts its range: it moves to a list that holds it all.)
FP_HD bool full_range_whole(uint32_t base, uint32_t items, uint32_t cap) { return base < cap && items <= cap - base; }
// emit_pair's condition, as a function of the descriptors' fields: k_split_finish and emit_pair call this one function.  dcol: first scratch
// column of R2 minus that of R1; dout: output offset of R2 minus that of R1 (both as unsigned differences: a negative one is huge).
FP_HD bool emit_pair_takes(uint32_t Lc1, uint32_t Lc2, uint32_t name_len, uint32_t rg_len, uint32_t mi_len, uint32_t cbl1, uint32_t cbl2,
                                                uint32_t rxl1, uint32_t rxl2, bool same_first, uint64_t dcol, uint64_t dout) {
  return Lc1 >= 8u && Lc1 <= 256u && Lc2 >= 8u && Lc2 <= 256u && name_len + 1u <= 32u && rg_len + 4u <= 32u && mi_len + 4u <= 32u &&
         cbl1 + 4u <= 32u && cbl2 + 4u <= 32u && rxl1 + 4u <= 32u && rxl2 + 4u <= 32u && rxl1 <= (uint32_t)FAST_RX_CAP && rxl2 <= (uint32_t)FAST_RX_CAP &&
         same_first && dcol < (1ull << 30) && dout - 1ull < (1ull << 30) - 1ull;
}
// "the writer applies": a pair family of the packed build whose items lie in one piece of at most 64 slots and whose pair emit_pair takes
FP_HD bool full_results_family(bool packed, bool pair, bool whole, uint32_t items, bool pair_taken) {
  return packed && pair && whole && items <= FULL_RESULT_MAX_ITEMS && pair_taken;
}

// ---- split simplex pipeline (simplex_split.inc): k_split_parse leaves one SplitRec per record and one SplitFam per family;
// k_split_cols (one wavefront per family) reads them instead of parsing, pairing and walking tags itself --------------------------
struct SplitRec {           // 32 bytes
  uint32_t body_off;        // record body offset minus the body offset of the family's first record
  uint16_t seq_rel;         // SEQ offset inside the body (qualities follow at + (l_seq + 1) / 2)
  uint16_t l_seq;
  uint16_t clip;            // bases past the mate's start (raw-bam/overlap.rs:181-357), <= l_seq
  uint16_t ov_off1, ov_off2, ov_cnt;   // an R1 with a mate: first shared base in this read / in the mate, number of shared bases (0: none)
  uint8_t slot, mate_slot;  // row of this read / of its mate in the family's LDS tile (rows of end A first, then end B, file order inside an end)
  uint8_t bits;             // end type (0 fragment, 1 R1, 2 R2) | reverse strand << 2 | has the cell tag << 3
  uint8_t cb_len;
  uint16_t cb_rel, mi_rel;  // tag values: offsets inside the body
  uint8_t mi_len, rx_len;
  uint16_t rx_rel;
  uint32_t _pad;
};
struct SplitFam {           // 32 bytes
  uint32_t flags;           // bit 0: k_split_cols takes the family (else it goes to k_simplex_wave2 untouched)
  uint32_t need_bytes;      // LDS bytes of the family's tile: rows x (qs + ss)
  uint16_t qs, ss;          // row strides of the quality / sequence tiles (multiples of 16)
  uint8_t n, m_a, m_b, type_a;   // records; rows of end A / end B; type of end A (0 fragment, 1 R1) — end B is R2
  uint8_t rev_a, rev_b;     // strand of the rows of end A / end B (a regular end has one)
  uint8_t rx_len, rx_all;   // rx_all 1: every record carries the same RX value of rx_len bytes; 0: no record has one
  uint16_t len_a, len_b;    // longest read of end A / end B (reverse ends: THE read length)
  uint32_t inv_cpr;         // ceil(2^24 / chunks per row): row of flat chunk t = (t * inv_cpr) >> 24
  uint16_t qc, sc;          // 16-byte chunks per row: qualities, sequence
};
struct SplitOut {           // 32 bytes: what k_split_cols decided for a family; k_split_finish (a thread per family) turns it into the
                            // EndDescs, record sizes and counters
  uint8_t status;           // 0: not finished by k_split_cols (another kernel's family); 1: finished; 2: fewer records than --min-reads
  uint8_t ne;               // consensus reads: 0, 1 (fragment) or 2 (R1 + R2)
  uint8_t type_a;           // end A: 0 fragment, 1 R1
  uint8_t fk_a, fk_b;       // first retained record of end A / end B (index inside the family): cell-barcode source
  uint8_t kept_a, kept_b;   // retained reads per end (the UMI rule: one read = its bytes, several = normalised)
  uint8_t n;                // records of the family
  uint16_t lc_a, lc_b;      // consensus lengths
  uint32_t rej;             // rejected reads: insufficient | zero length << 8 | orphan << 16
  uint32_t ov_agree, ov_dis, ov_corr;   // overlapping-bases counters (ov_corr: the count in S2_OV_COUNT, above it which step corrected a packed-build family)
  uint32_t depth_stats;    // direct records: max | min << 8 of the per-base depths of end A, the same of end B << 16 (the cD / cM tags; at most 16 reads per end)
};
static_assert(sizeof(SplitRec) == 32 && sizeof(SplitFam) == 32 && sizeof(SplitOut) == 32, "split descriptors are moved as two 16-byte pieces");
// SplitOut.ov_corr of a family the packed build finished (fgx_debug_last_packed_overlap): the overlap of its mates was corrected by the packed
// step (eight bases per lane) / by the byte-wise steps / by those because a shared quality of 128 or more voted it out of the packed step
constexpr uint32_t S2_OV_COUNT = 0x0FFFFFFFu, S2_OV_PACKED = 1u << 28, S2_OV_BYTEWISE = 1u << 29, S2_OV_GUARD = 1u << 30;

// ---- direct records (round 4): k_split_cols writes the consensus records of its families itself ------------------------------------
// k_split_parse predicts the exact bytes of every family's records (final lengths at the reads' 3' ends, consensus lengths, tag
// lengths); a per-chunk exclusive scan turns them into output offsets before the chunk's column kernel starts; the column lanes store
// nibbles / qualities / cd / ce straight into the records and the family's wavefront writes header, name and tags.  The columns that
// wait for k_call_full are patched in the records by that kernel (nibble OR, quality byte, cd / ce entries, the record's error count),
// and k_fix_ce rewrites the cE value of the records that had errors.  No column scratch, no EndDesc, no k_emit for these families.
struct SlotDesc {           // one directly written record (slot 3g + type): what k_call_full / k_fix_ce need to patch it
  uint64_t out_off;         // offset of the record (its block_size prefix) in the output buffer
  uint32_t lc_seq;          // consensus length | offset of SEQ inside the record (from the prefix) << 16
  uint32_t sum_depth;       // sum of the per-base depths: the denominator of cE
};
constexpr uint64_t FULL_DEST_DIRECT = 1ull << 62;   // FullItem.dest: DIRECT | slot << 16 | column

struct FastParams {
  const uint8_t* blob; const uint64_t* rec_off; const uint32_t* rec_len; const uint32_t* grp_first;
  uint32_t g0;
  const DeviceTables* T; const DeviceTables* TU;
  uint32_t min_reads; int64_t max_reads;
  char tag0, tag1, cell0, cell1;   // (dword-aligned: the kernels read them with scalar loads; at odd offsets they came through vector memory)
  uint32_t min_input_bq, min_cons_bq, trim, overlap, per_base_tags, track_rejects;   // (one dword each: adjacent bytes were fetched as one unaligned vector load)
  uint32_t prefix_len, rg_len;
  EndDesc* ends; uint64_t* rec_sizes;
  uint8_t* col_code; uint8_t* col_qual; uint16_t* col_depth; uint16_t* col_err;
  const uint64_t* col_base;        // per-group first scratch column (exclusive scan of the column bound)
  unsigned long long* stats;
  uint32_t* deferred; uint32_t* n_deferred;
  const uint32_t* group_list;      // nullptr: group = g0 + blockIdx.x
  uint32_t* retry; uint32_t* n_retry;   // families needing more LDS than this launch provides (nullptr: defer them)
  uint32_t* retry_old; uint32_t* n_retry_old;   // k_simplex_wave2: families outside its record shape → k_family_wave<0>
  const void* w2_image;            // k_simplex_wave2: image of its LDS tables (W2Lds, simplex_wave2.inc)
  const void* fw_image;            // k_family_wave: image of its LDS tables (FwLds, fastpath.hip)
  SplitRec* split_rec; SplitFam* split_fam; SplitOut* split_out;   // split simplex pipeline: k_split_parse → k_split_cols → k_split_finish
  uint32_t* route; uint32_t* n_route;         // k_split_cols: families it does not take → k_simplex_wave2
  uint32_t* big; uint32_t* n_big;             // families of more than 64 records (no wavefront-per-family kernel takes them): straight to k_family's list (may be null)
  const void* s2_image;            // k_split_cols: image of its LDS tables (S2Lds, simplex_split.inc)
  const uint4* fam_desc;           // per family {first record offset lo, hi, bytes to the end of the last record (~0: none), records} (k_col_bound)
  uint64_t blob_len;               // records must end inside the blob (checked before the family's bytes are staged)
  // direct records (k_split_parse predicts, k_split_cols<.., .., 1> writes)
  uint32_t* dir_size;              // per family: bytes of its consensus records (block_size prefixes included); 0: none / not this pipeline's
  const uint64_t* dir_off;         // per family: offset of its first record in `out` (exclusive scan of dir_size)
  uint8_t* out; uint64_t out_cap;  // the output buffer
  uint64_t* out_off;               // per slot (3g + type): offset of the record in `out` (what the scan of rec_sizes gives the scratch path)
  SlotDesc* slot_desc; uint32_t* slot_err;   // per slot: patch descriptor; errors counted by k_call_full
  const char* strings;             // read-name prefix | read group id
  uint32_t* dir_flags;             // [0] families whose records differ in size from the prediction, [1] records past out_cap
  uint32_t lds_tile_bytes;
  uint32_t lds_wave_bytes;
  uint32_t s2_partner;             // k_split_cols<.., 1>: a <.., 2> launch over the same families follows (else it hands the families that are not its shape to the next launch)
  uint32_t s2_packed;              // k_split_cols: 1 = ends of at least s2_nsafe rows try the packed pass first (round 5; FGX_S2_PACKED=0: measurements); | 2: debug counters; | 4: the clean test (FGX_S2_CLEAN_ROWS=0: off); | 8: the packed overlap step (FGX_S2_PACKED_OVERLAP=0: off)
  uint32_t s2_nsafe;               // k_split_cols: unanimous_cap_depth(tables, min_input_bq) — agreeing observations from which a column is the cap for certain (gate_core.h)
  FullItem* full_items; uint32_t* full_count; uint32_t full_cap;   // N_LISTS append lists of `full_cap` items each
  uint32_t full_results;           // 1: k_call_full's answers go to the pair writer through a result array (FullResult above; FGX_FULL_RESULTS=0: off)
  uint8_t* full_flag;              // per family: the writer applies its results (k_split_finish; cleared per batch)
  unsigned long long* full_stats;  // STAT_SLOTS x FULL_STATS_STRIDE words: the counters of the path (FULL_STATS_N above)
  // methylation-aware mode on the streaming kernels (simplex_deep.inc; meth_mode = FGX_METHYLATION_*, 0: off): the genome of fgx_set_reference
  // (contig i = [contig_off[i], + contig_len[i])), and per scratch column: the reference shows a cytosine of the call's strand | unconverted |
  // converted source bases (methylation.rs:193-242)
  uint32_t meth_mode, n_ref;
  const uint8_t* genome; const uint64_t* contig_off; const uint64_t* contig_len;
  uint8_t* meth_flag; uint16_t* meth_u; uint16_t* meth_t;
  // duplex (k_family_wave<1>; with the methylation-aware mode k_family_wave<1, 1>, which fills meth_flag / meth_u / meth_t per column of the four read sets)
  uint32_t dmin_total, dmin_xy, dmin_yx; int64_t dmax_reads;
  uint32_t* col_obs;               // per column: observation counts of A,C,G,T, one byte each
  uint32_t* col_obs_all;           // the same over every source read of the set, for the molecules a --max-reads-per-strand cap bites (allocated when the caller has a cap)
  DuplexDesc* dends;
  // CODEC (k_family_wave<2>)
  CodecDesc* cends; uint32_t cmin_reads, cmin_duplex_len; int64_t cmax_reads;
};

struct EmitParams {
  const uint8_t* blob; const uint64_t* rec_off; const EndDesc* ends; const uint64_t* out_off; uint8_t* out;
  uint64_t out_base; uint32_t slot0, slot_end;
  const uint8_t* col_code; const uint8_t* col_qual; const uint16_t* col_depth; const uint16_t* col_err;
  const char* prefix; uint32_t prefix_len; const char* rg; uint32_t rg_len;
  uint8_t per_base_tags; char tag0, tag1, cell0, cell1;
  const uint32_t* fam_list; uint32_t n_fam;   // non-null: a wavefront per LISTED family (direct records: the families that left the split pipeline)
  const FullResult* full_res; const uint8_t* full_flag;   // k_call_full's answers for emit_pair (null: none; fastpath.h, FullResult)
};

struct DuplexEmitParams {
  const uint8_t* blob; const uint64_t* rec_off; const DuplexDesc* ends; const uint64_t* out_off; uint8_t* out;
  uint32_t slot0, slot_end;
  const uint8_t* col_code; const uint8_t* col_qual; const uint16_t* col_err; const uint32_t* col_obs;
  const char* prefix; uint32_t prefix_len; const char* rg; uint32_t rg_len;
  uint8_t per_base_tags; char cell0, cell1;
  uint32_t* n_slow;                // k_count_slow counts the valid records the fast writer leaves to the per-field kernel here (0: that kernel is not launched at all)
  const uint8_t* meth_flag;        // methylation-aware mode (the <1> builds of the writers): per column, the reference shows a cytosine of the strand's call
  const uint32_t* col_obs_all;     // a caller with --max-reads-per-strand (the CAP builds of the writers): the recount source of the records with DuplexDesc::capped
};

struct CodecEmitParams {
  const uint8_t* blob; const uint64_t* rec_off; const CodecDesc* ends; const uint64_t* out_off; uint8_t* out;
  uint32_t slot0, slot_end;
  const uint8_t* col_code; const uint8_t* col_qual; const uint16_t* col_depth; const uint16_t* col_err;
  const char* prefix; uint32_t prefix_len; const char* rg; uint32_t rg_len;
  uint8_t per_base_tags; char cell0, cell1;
  uint8_t has_outer, outer_qual, has_ss, ss_qual; uint32_t outer_len;
  unsigned long long* stats;       // slot-spread counters: [24] consensus bases, [25] duplex bases, [26] disagreeing duplex bases
  uint32_t* n_slow;                // k_count_slow counts the valid records the fast writer leaves to the per-field kernel here
};

struct FastResult {
  const uint8_t* d_out; uint64_t out_len; uint64_t count;
  uint64_t stats[FGX_STATS_LEN];
  uint32_t n_deferred; const uint32_t* d_deferred;
  const uint64_t* d_out_off;     // byte offset of each of the 3*n_grp slots in d_out
  const uint64_t* d_slot_size;   // bytes of each slot (block_size prefix included; 0 = no record)
  uint32_t n_slots;
  double ms_kernels, ms_k_family, ms_k_emit; uint64_t cols_used; uint64_t full_items;
};

struct FastPath {
  DevBuf d_ends, d_sizes, d_offsets, d_code, d_qual, d_depth, d_err, d_misc, d_deferred, d_out, d_scan_tmp, d_strings;
  uint32_t lds_tile_bytes = 12288;        // first launch: tiles of the common small families
  uint32_t lds_tile_bytes_large = 65536;  // workgroup-per-family kernel: raw records + unpacked base / quality tiles of one big family (2 workgroups per CU)
  DevBuf d_retry, d_bound, d_colbase, d_statslots, d_full_items, d_full_count, d_obs, d_obs_all, d_retry2, d_retry_old;
  DevBuf d_full_res, d_full_flag;         // k_call_full's result array (a slot per slot of d_full_items) and the per-family flags
  uint64_t last_full_results[FULL_STATS_N] = {0, 0, 0, 0, 0};   // the last batch: items answered through the array, items scattered, families the writer applied, families refused as not in one piece
  DevBuf d_w2img;                         // W2Lds image, built from the caller's tables at the first batch
  DevBuf d_famdesc;                       // k_col_bound's family descriptors
  DevBuf d_fwimg;                         // FwLds image (k_family_wave)
  DevBuf d_split_rec, d_split_fam, d_split_out, d_route, d_s2img;   // split simplex pipeline
  DevBuf d_big;                            // simplex families of more than 64 records: k_family's list, filled by the first kernel that sees them
  uint32_t last_big_families = 0;          // ... in the last batch
  uint32_t last_deep_families = 0;         // ... of which k_deep_parse + k_deep_cols (simplex_deep.inc) took
  DevBuf d_deep_sizes, d_deep_row0, d_deep_rows, d_deep_fams, d_deep_out, d_deep_out2;
  DevBuf d_deep_walk;                      // duplex_deep.inc under --max-reads-per-strand: the scoring rows of capped sets in walk order (allocated for a caller with a cap);
                                           // codec_deep.inc: the RX values of a molecule's records in file order
  uint32_t last_duplex_deep = 0;           // duplex molecules of more than 64 records that k_duplex_deep_parse + k_duplex_deep_cols (duplex_deep.inc) decided in the last batch;
                                           // not counted into last_big_families / last_deep_families (the simplex path's).  They use d_big and the d_deep_* buffers.
  uint32_t last_duplex_deep_capped = 0;    // ... of which a --max-reads-per-strand bit a set (the CAP builds; FGX_DUPLEX_DEEP_CAP=1)
  uint32_t last_codec_deep = 0;            // CODEC molecules of more than 64 records that k_codec_deep_parse + k_codec_deep_cols (codec_deep.inc; FGX_CODEC_DEEP=1) decided in the
                                           // last batch; likewise not counted into the simplex path's counters.  They use d_big, the d_deep_* buffers and d_deep_walk (the RX list).
  uint32_t last_codec_deep_capped = 0;     // ... of which a --max-reads-per-strand dropped a read (the CAP builds of the record kernel)
  bool canon_second_pass = false;          // set by the caller around the `run` of a canonical second pass: codec_deep.inc stays off there, and duplex_deep.inc unless FGX_DEEP_INDELS=1
  uint32_t last_deep_indels = 0;           // FGX_DEEP_INDELS=1: molecules of more than 64 records that the deep duplex kernels decided in the canonical SECOND pass of the last batch
  bool rejects_pass = false;               // set by the host entry around the device pass of a --rejects batch (which runs with the option cleared): off there too
  uint32_t last_wide_families = 0;         // ... and of what those left, the wide kernels (simplex_wide.inc; FGX_DEEP_WIDE=1) took — not counted into last_deep_families
  DevBuf d_wide_scratch, d_wide_pass, d_wide_pass0, d_wide_depth;   // k_wide_parse's per-record state, the families' column passes and their scan, the passes' depth extremes
  DevBuf d_mflag, d_mu, d_mt, d_mslot, d_mcontigs;   // methylation-aware mode: per-column annotation, per-slot tag sizes, the contig table
  const void* ref_runs = nullptr;          // methylation-aware mode, the canonical second pass (FGX_METH_CANON=1): canon::RefRuns of every record of the batch `run` is
                                           // about to take, device memory; set by the caller around that one `run`, null otherwise (the records lie where they say)
  uint32_t last_meth_device = 0;           // families of the last batch that the device pipeline decided in the methylation-aware mode
  uint32_t last_deep_clipped = 0;          // FGX_DEEP_CLIPS=1, outside the mode: families / molecules of more than 64 records with a multi-op record that the clip builds of the streaming record kernels accepted
  uint32_t last_meth_clipped = 0;          // ... of which held a record of more than one CIGAR op (clips around one aligned block) and were not deferred
  uint32_t last_routed = 0;                // families the split pipeline handed to the k_simplex_wave2 chain in the last batch
  uint64_t last_packed_clean = 0, last_packed_general = 0;        // ... of the packed build's: by its clean row loop (no quality read) / by its general one
  uint64_t last_packed_overlap[OV_STATS_N] = {0, 0, 0};           // ... whose overlapping mates the packed step corrected / the byte-wise steps / of those: voted out of the packed step by its guard
  uint64_t last_packed_families = 0, last_classic_families = 0;  // families of the last batch finished by k_split_cols's packed build / by its classic builds (k_split_finish counts them)
  uint32_t last_split_build = 0;           // first-stage build of the last batch: 0 classic alone (or no split pipeline), 1 packed alone, 2 packed + partner launch
  uint32_t last_first_stage_retries = 0;   // families the first stage handed to the next launch
  uint32_t last_launches = 0, last_host_syncs = 0;   // kernel launches (library scans not counted) / host synchronisations of the last batch
  DevBuf d_dir_size, d_dir_off, d_dir_base, d_slot_desc, d_slot_err, d_out2, d_scan_tmp2;   // direct records (simplex_split.inc, fastpath.h)
  bool direct_off = false;                // a batch whose predicted record sizes did not hold: this caller stays on the scratch path (diagnostics: last_direct)
  uint64_t dir_cap_min = 0;               // output room a batch asked for beyond the first estimate
  uint32_t dir_chunks_run = 0;            // chunks of the last direct batch that held families: d_dir_base[dir_chunks_run] = bytes of all directly written records
  int last_direct = 0;                    // 0: the last batch went through the column scratch + k_emit; 1: records written directly; 2: directly + merge
  uint32_t lds_wave_bytes = 6144;         // wave-per-family kernel: LDS copy of one family's raw records
  uint32_t lds_wave_bytes_duplex = 8704;  // duplex molecules carry both strands (config 3: 24 records x ~330 B)
  uint32_t lds_wave_bytes_codec = 5120;   // CODEC (config 5: 8 records x ~570 B): its kernel needs 71 VGPRs, so the smaller slice buys a sixth wave per SIMD (+3 %)
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  // split simplex pipeline: the record kernel runs chunk by chunk on a second stream, under the column kernel of the chunk before
  uint32_t pool_slack = 256; bool pool_init = false;
  uint32_t pool_div = 8;                  // k_call_full's append lists hold 1 / pool_div of the column bound (halved when a batch exhausts them)
  static constexpr int RUN_AGAIN_LARGER_POOL = -77;   // (also: the batch again without / with more room for the direct records)
  // hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: one flag per FastPath (= per caller = per device), not per process
  bool lds_attr_set = false, s2_attr_set = false, v2_attr_set = false;
  static constexpr int MAX_CHUNKS = 65;
  uint32_t last_split_chunks = 0;         // chunks the record / column pipeline ran the last batch in (0: another head of the chain); diagnostics
  hipStream_t s2 = nullptr;
  hipEvent_t ev_chunk[MAX_CHUNKS] = {}, ev_cols[MAX_CHUNKS] = {}, ev_fin = nullptr, ev_sample = nullptr;
  int run(fgx_caller* c, const uint8_t* d_blob, uint64_t blob_len, const uint64_t* d_rec_off, const uint32_t* d_rec_len, uint32_t n_rec,
          const uint32_t* d_grp_first, uint32_t n_grp, FastResult* res);
  void release();
};

}  // namespace fgx
