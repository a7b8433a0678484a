// fastpath.hip — the device-resident pipelines of the three callers: raw BAM records in HBM → consensus BAM records in HBM,
// no host work per family.  Sections, in file order:
//
//   shared device helpers     ReadInfo / Shared (LDS state of the workgroup kernel), name_rank (fgbio Murmur3 name rank), general-CIGAR
//                             helpers (map_ref_to_query, simplified CIGARs, alignment_filter = select_most_common_alignment_group)
//   k_family                  ONE WORKGROUP (512 threads) PER FAMILY: families with more than 64 records, a byte span beyond the largest
//                             wave slice, or any read with an indel / skip.  Records copied HBM→LDS once; a thread per record parses
//                             (general CIGARs up to 6 ops), unpacks, pairs mates, corrects overlaps through both CIGARs, computes the
//                             source-read geometry, runs the gates (alignment filter, --max-reads downsampling, min-reads at every
//                             shrink point, orphan rule); a thread per column calls the consensus; per-character UMI consensus.
//   k_family_wave<MODE>       ONE WAVEFRONT PER FAMILY / MOLECULE, the common case.  MODE 0 simplex, 1 duplex (strand partition, four
//                             single-strand column sets, descriptors of the two duplex records), 2 CODEC (FR pairs, virtual hard clip
//                             against the mate, overlap geometry, two strand column sets).  Phases: stage raw records into LDS → parse
//                             (lane = record) → overlap pre-correction → geometry → gates → columns (lane = column, reads walked in file
//                             order: summation order is observable) → UMI consensus → descriptors + stats.  Columns the unanimous fast
//                             path cannot decide go to 1024 chained lists for k_call_full.
//   k_call_full               one lane per deferred column (or UMI character): ln_sum_exp chain on the device libm, tie rule, Phred.
//   k_emit / k_emit_duplex[_fast] / k_emit_codec[_fast]      (record_writers.inc)
//                             one wavefront per consensus record: header, name `<prefix>:<MI>`, 4-bit sequence, qualities and the
//                             caller's tag set at the record's scanned offset (the _fast writers take the records of common shape,
//                             the generic per-field writers the rest); duplex / CODEC combine the strands here.
//   k_col_bound, k_reduce_stats, FastPath::run
//                             column-slot bounds, counter reduction, and the host orchestration: staged wave launches over growing
//                             LDS slices with retry lists (4 / 2 / 1 wavefronts per workgroup), workgroup kernel for what is left,
//                             scans, emit.
//
// Reference semantics restated (bit-exact contract), paths under crates/fgumi-consensus/src/ unless noted:
//   src/lib/commands/simplex.rs:669-701 (group skip, overlap pre-step, consensus_reads)
//   overlapping.rs:236-336, 565-684 ; vanilla_caller.rs:48-120, 862-932, 1080-1296, 1304-1422, 1454-1646, 1652-1755, 1767-1881 ;
//   simple_umi.rs:46-117 ; duplex_caller.rs:560-1405, 1837-2624 ; codec_caller.rs:504-1911 ;
//   crates/fgumi-raw-bam/src/{overlap.rs:21-357, hash.rs:14-89, builder.rs:122-301, cigar.rs:404-500}
//
// Families the device does not decide are DEFERRED untouched to the general host path (simplex_host.cpp, duplex_host.cpp,
// codec_host.cpp): reads with more than 16 CIGAR ops or SEQ / CIGAR length mismatch, malformed records (so that
// the general path raises the reference's fatal error), unmapped reads of the duplex / CODEC callers and of the methylation-aware mode, an unmapped
// record that carries CIGAR ops, more than FAST_MAX_READS reads or more LDS than the launch provides,
// duplex / CODEC molecules with indels.  A per-strand read cap that bites is decided here (the CAP builds of k_family_wave<1> / <2> and of the
// duplex record writers, k_family_wave<1, 1, 1> in the methylation-aware mode); deferred under one: a duplex cap of 0.  The simplex kernels take unmapped records
// (`fgumi group --allow-unmapped`): a read without a CIGAR, no mate clip, no overlap step; ends that are uniform by flag stay where a mapped family of their
// shape runs, an end with mapped AND unmapped reads is k_family_wave<0>'s (drop_unmapped_if_any_mapped) — up to 64 records and without indel reads, else
// deferred.  See DESIGN.md 3.
#if !defined(FGX_WAVEMU)      // (tests/wavemu compiles this file for the HOST under a 64-lane lock-step shim, with stand-ins for the runtime and the scans)
#include <hipcub/hipcub.hpp>
#endif
#include "bamrec.h"
#include "canon_core.h"
#include "engine.h"
#include <cstdlib>
#include <memory>
#include <string>
#include <type_traits>
#include "fastpath.h"
#include "gate_core.h"
#include "packed_core.h"
#include "record_core.h"

// The device-only spellings behind macros, so that tests/wavemu (a wave-level host emulator of the wavefront kernels) can compile this
// file for the host: dynamic LDS, and the inline assembly — scheduling pins for the device compiler ("+v" / "s" constraints mean nothing on a CPU) and
// four scalar-unit idioms with plain C++ twins.
#if defined(FGX_WAVEMU)
#define FGX_DYN_LDS(name) uint8_t* const name = wavemu::dyn_lds()
#define FGX_PIN(...) ((void)0)
#define FGX_UNDEF4(a, b, c, d) do { a = 0; b = 0; c = 0; d = 0; } while (0)
#define FGX_MEM_PIN() ((void)0)
#define FGX_CONST_AS
#else
#define FGX_DYN_LDS(name) extern __shared__ __align__(16) uint8_t name[]
#define FGX_PIN(...) asm volatile("" : __VA_ARGS__)
#define FGX_UNDEF4(a, b, c, d) asm volatile("" : "=v"(a), "=v"(b), "=v"(c), "=v"(d))     /* "whatever the registers hold" costs no instruction */
#define FGX_MEM_PIN() asm volatile("" ::: "memory")
#define FGX_CONST_AS __attribute__((address_space(4)))
#endif

namespace fgx {

using bam::rd16;
using bam::rd32;

namespace {

#ifndef FGX_BLOCK_NT
#define FGX_BLOCK_NT 512
#endif
constexpr int NT = FGX_BLOCK_NT;        // threads per family workgroup
constexpr int FAST_MAX_READS = 128;     // per-read LDS tables
constexpr int MAX_MC_OPS = 8;
constexpr uint32_t MAX_CIG_OPS = 6;     // clips + aligned ops of a read the WAVEFRONT kernels take
// Round 5: the workgroup-per-family kernel (k_family: indel / clipped simplex families of up to 128 records) takes reads of up to 16 CIGAR ops
// and mates whose MC tag holds up to 17 — real aligner output carries such CIGARs in a fraction of a percent of its reads, and round 4 sent
// every family that holds one through the general path (host orchestration, ~5 M reads/s); the wavefront kernels hand them on
constexpr uint32_t WG_CIG_OPS = 16;
constexpr int WG_MC_OPS = 17;
constexpr uint32_t COL_BOUND_PAD = 48;   // columns on top of a family's column bound: the padding of the packed build's scratch layout (simplex_split.inc, round 6)
constexpr int STAT_SLOTS = 1024;        // spread the per-batch counters over many addresses (atomic contention)
// Methylation-aware mode: families / molecules with a record of more than one CIGAR op that the device kernels decided (fgx_debug_last_meth_clipped).
// The counter is the word of d_misc behind the deferred count (MISC_N_METH_CLIPPED == MISC_N_DEFERRED + 1, asserted at the enum) and is reached from
// that pointer: a further member of FastParams would move the arguments of every kernel that takes one, the builds that count nothing included.
// This holds only while P.n_deferred points at the low half of that 8-byte word of d_misc (fill_params sets it so; a u32 counter uses its word's low
// half, so the next word's counter is two uint32_t further): whoever points n_deferred elsewhere gives this counter a FastParams member of its own.
__device__ __forceinline__ uint32_t* meth_clipped_counter(const FastParams& P) { return P.n_deferred + 2; }
// FGX_DEEP_CLIPS=1, outside the mode: simplex families / duplex molecules of more than 64 records with a record of more than one CIGAR op that the clip builds
// of the streaming record kernels accepted (fgx_debug_last_deep_clipped).  The HIGH half of the same word, for the same reason; the mode's counter never
// passes 2^32, and the read-back takes the halves apart.
__device__ __forceinline__ uint32_t* deep_clipped_counter(const FastParams& P) { return P.n_deferred + 3; }

struct ReadInfo {          // LDS, one per record of the family
  uint64_t goff;           // record body offset in the blob
  int32_t pos, ref_id;
  uint32_t name_hash;
  uint32_t row;            // row offset (bytes) of this read's bases / quals in the LDS tiles
  uint16_t l_seq, flags, seq_off, name_len;
  uint16_t final_len, trim_to, clip, mi_off;
  uint16_t rx_off, cb_off;
  int16_t mate;            // index of the R2 paired with this R1 (only set on the R1), else -1
  uint8_t mi_len, rx_len, cb_len, end;   // end: 0 fragment, 1 R1, 2 R2, 255 = not a candidate
  uint8_t has_mi, has_rx, has_cb, all_ff;
  uint8_t excluded, zero_len, minority, _p1;   // minority: dropped by the alignment filter (select_most_common_alignment_group)
};

struct Shared {
  ReadInfo ri[FAST_MAX_READS];
  uint16_t members[FAST_MAX_READS];     // kept reads, grouped by end, file order inside an end
  uint32_t stats[FGX_STATS_LEN];
  uint32_t defer;
  uint32_t n_ends;
  uint32_t end_type[3], end_first[3], end_cnt[3], end_len[3], end_coloff[3];
  uint32_t end_maxd[3], end_mind[3], end_sumd[3], end_sume[3];
  uint32_t end_rx_cnt[3], end_rx_len[3], end_rx_first[3];
  char end_rx[3][FAST_RX_CAP];
  uint32_t rx_bad;
  uint64_t col_base;
  uint32_t tile_bytes;
  unsigned long long raw_lo, raw_hi;    // byte span of the family's records in the blob
  uint32_t g_wcnt[2][3];                // gates: kept reads per wave and end
  uint32_t g_best[3], g_rxcnt[3], g_rxpos[3], g_rxbad[3];
  uint32_t scig[FAST_MAX_READS][WG_CIG_OPS];   // simplified CIGAR of each read (S, H, =, X folded into M, neighbours merged): len << 4 | kind
  uint8_t n_scig[FAST_MAX_READS];
  uint8_t b4_order[FAST_MAX_READS];             // alignment filter: members of one end, longest first
  uint16_t b4_mask[FAST_MAX_READS];             // alignment filter: groups a read belongs to
  uint32_t any_complex;                         // some read has more than one aligned block or clips
  int32_t name_rank[FAST_MAX_READS];            // --max-reads: fgbio name rank of each kept read
};

__device__ __forceinline__ void defer(Shared& S) { S.defer = 1; }

__device__ __forceinline__ uint32_t int_tag_width(uint32_t v) { return v <= 255 ? 1 : 2; }   // depth <= 32767: c / C / S

// Oriented, mask-aware view of read `r` at consensus position p.  Returns the 4-bit code (15 = N, also
// for masked bases) and the quality the reference's SourceRead would hold there.
__device__ __forceinline__ void oriented(const Shared& S, const uint8_t* lb, const uint8_t* lq, const ReadInfo& R, uint32_t p,
                                         uint32_t min_bq, uint8_t* code, uint8_t* qual) {
  bool rev = (R.flags & bam::F_REVERSE) != 0;
  uint32_t idx = rev ? (uint32_t)R.l_seq - 1 - p : p;
  uint8_t c = lb[R.row + idx];
  uint8_t q = lq[R.row + idx];
  if (rev) c = bam::code_complement(c);
  if (p < R.trim_to && q < min_bq) { c = 15; q = FGX_MIN_PHRED; }
  *code = c;
  *qual = q;
}

// fgbio_read_name_rank (raw-bam/hash.rs:14-89): Murmur3_32, seed 42, over the UTF-16 code units of the read name, as i32
__device__ inline int32_t name_rank(const uint8_t* name, uint32_t len) {
  auto rotl = [](uint32_t v, int r) { return (v << r) | (v >> (32 - r)); };
  auto mixk = [&](uint32_t k) { k *= 0xcc9e2d51u; k = rotl(k, 15); return k * 0x1b873593u; };
  uint32_t h = 42;
  for (uint32_t i = 1; i < len; i += 2) { h ^= mixk((uint32_t)name[i - 1] | ((uint32_t)name[i] << 16)); h = rotl(h, 13) * 5 + 0xe6546b64u; }
  if (len & 1) h ^= mixk(name[len - 1]);
  h ^= 2 * len;
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return (int32_t)h;
}

// ---- general CIGARs in the workgroup kernel ------------------------------------------------------------------------------------
// query offset of reference position x (1-based) in a read that starts at ref1, or -1 when x is not inside an aligned block or
// falls past the stored bases (ReadMateAndRefPosIterator, overlapping.rs:565-620)
__device__ __forceinline__ int32_t map_ref_to_query(const uint32_t* ops, uint32_t n, int64_t ref1, int64_t x, uint32_t l_seq) {
  int64_t ref = ref1, q = 0;
  for (uint32_t i = 0; i < WG_CIG_OPS; i++) {
    if (i >= n) break;
    const uint32_t t = ops[i] & 15;
    const int64_t len = ops[i] >> 4;
    if (t == 0 || t == 7 || t == 8) {
      if (x < ref + len) { if (x < ref) return -1; const int64_t qi = q + (x - ref); return qi < (int64_t)l_seq ? (int32_t)qi : -1; }
      ref += len; q += len;
    } else if (t == 1 || t == 4) q += len;
    else if (t == 2 || t == 3) ref += len;
  }
  return -1;
}
// SourceRead::simplified_cigar of read r: reversed for a reverse-strand read, truncated to its final length
// (create_source_read :1172-1176, truncate_simplified_cigar :1028-1062)
__device__ inline uint32_t oriented_truncated_cigar(const Shared& S, uint32_t r, uint32_t* out) {
  const ReadInfo& R = S.ri[r];
  const uint32_t n = S.n_scig[r];
  const bool rev = (R.flags & bam::F_REVERSE) != 0;
  uint32_t remaining = R.final_len, m = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (remaining == 0) break;
    const uint32_t v = S.scig[r][rev ? n - 1 - i : i], k = v & 15, len = v >> 4;
    if (k == 0 || k == 1) { const uint32_t take = len < remaining ? len : remaining; out[m++] = (take << 4) | k; remaining -= take; }
    else out[m++] = v;
  }
  return m;
}
__device__ inline bool cigar_is_prefix(const uint32_t* a, uint32_t na, const uint32_t* b, uint32_t nb) {   // clipper.rs:1212-1241
  if (na > nb) return false;
  for (uint32_t i = 0; i < na; i++) {
    if ((a[i] & 15) != (b[i] & 15)) return false;
    if (i + 1 == na) { if ((a[i] >> 4) > (b[i] >> 4)) return false; }
    else if ((a[i] >> 4) != (b[i] >> 4)) return false;
  }
  return true;
}
__device__ inline int cigar_cmp(const uint32_t* a, uint32_t na, const uint32_t* b, uint32_t nb) {   // vanilla_caller.rs:96-113: length, then op kind, then op count
  const uint32_t n = na < nb ? na : nb;
  for (uint32_t i = 0; i < n; i++) {
    if ((a[i] >> 4) != (b[i] >> 4)) return (a[i] >> 4) < (b[i] >> 4) ? -1 : 1;
    if ((a[i] & 15) != (b[i] & 15)) return (a[i] & 15) < (b[i] & 15) ? -1 : 1;
  }
  return na == nb ? 0 : (na < nb ? -1 : 1);
}
// filter_source_reads_by_alignment (vanilla_caller.rs:1242-1296) for the kept reads of end e, by one thread: stable sort by
// length (longest first), greedy multi-membership prefix groups, the largest group wins (ties: the smaller CIGAR, then the
// later group); everyone outside it is marked `minority`.
__device__ inline void alignment_filter(Shared& S, uint32_t e, uint32_t n) {
  uint32_t m = 0;
  bool single_block = true;
  for (uint32_t i = 0; i < n; i++)
    if (S.ri[i].end == e && !S.ri[i].zero_len) { S.b4_order[m++] = (uint8_t)i; if (S.n_scig[i] != 1) single_block = false; }
  if (m < 2 || single_block) return;        // (M, len) CIGARs are all prefixes of the longest one: a single group, nothing dropped
  for (uint32_t k = 1; k < m; k++) {        // stable insertion sort, longest first
    const uint8_t v = S.b4_order[k];
    const uint32_t lv = S.ri[v].final_len;
    uint32_t j = k;
    while (j > 0 && S.ri[S.b4_order[j - 1]].final_len < lv) { S.b4_order[j] = S.b4_order[j - 1]; j--; }
    S.b4_order[j] = v;
  }
  constexpr uint32_t MAX_GROUPS = 16;
  uint32_t ng = 0;
  uint8_t founder[MAX_GROUPS];
  uint32_t count[MAX_GROUPS];
  uint32_t ca[WG_CIG_OPS], cb[WG_CIG_OPS];
  for (uint32_t k = 0; k < m; k++) {
    const uint32_t r = S.b4_order[k];
    const uint32_t na = oriented_truncated_cigar(S, r, ca);
    uint32_t mask = 0;
    for (uint32_t g = 0; g < ng; g++) {
      const uint32_t nb = oriented_truncated_cigar(S, founder[g], cb);
      if (cigar_is_prefix(ca, na, cb, nb)) { count[g]++; mask |= 1u << g; }      // no break: a read joins every group it is a prefix of
    }
    if (!mask) {
      if (ng == MAX_GROUPS) { defer(S); return; }
      founder[ng] = (uint8_t)r; count[ng] = 1; mask = 1u << ng; ng++;
    }
    S.b4_mask[r] = (uint16_t)mask;
  }
  uint32_t best = 0;                         // Iterator::max_by keeps the LAST maximal element
  for (uint32_t i = 1; i < ng; i++) {
    int c;
    if (count[best] != count[i]) c = count[best] < count[i] ? -1 : 1;
    else {
      const uint32_t na = oriented_truncated_cigar(S, founder[i], ca), nb = oriented_truncated_cigar(S, founder[best], cb);
      c = cigar_cmp(ca, na, cb, nb);
    }
    if (c <= 0) best = i;
  }
  for (uint32_t k = 0; k < m; k++) { const uint32_t r = S.b4_order[k]; if (!((S.b4_mask[r] >> best) & 1)) S.ri[r].minority = 1; }
}


#include "chain_observe.inc"
// mask of the lanes l with p0 + l < limit (both scalar), on the scalar unit (k_simplex_wave2's lanes_below, which is defined after this kernel)
__device__ __forceinline__ unsigned long long fw_lanes_below(uint32_t limit, uint32_t p0) {
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

// ---- wavefront helpers, unaligned LDS words, the aux walk (shared by every family kernel) ----------------------------
constexpr int WAVES_PER_BLOCK = 4;
#ifndef FGX_W2_WPB_DEFAULT
#define FGX_W2_WPB_DEFAULT 3
#endif

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }   // v is the same in every lane: say so
__device__ __forceinline__ uint32_t rlane(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
// Wavefront reductions of a 32-bit value through the data-parallel primitives of the vector ALU: quad swap, quad-pair swap, half-row mirror,
// row mirror (every lane of a row of 16 then holds the row's result), row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3 — six
// instructions, each with its operation folded in, the total in lane 63, returned as a scalar.  (A butterfly of __shfl_xor is six LDS
// permutes + six operations + their addresses.)  `idn` = the operation's identity: what a lane outside a step's row mask contributes.
template <int CTRL, int ROWS> __device__ __forceinline__ uint32_t wave_dpp(uint32_t idn, uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)idn, (int)v, CTRL, ROWS, 0xF, false); }
#define FGX_WAVE_REDUCE(v, idn, OP) do { \
    v = OP(v, wave_dpp<0xB1, 0xF>(idn, v)); v = OP(v, wave_dpp<0x4E, 0xF>(idn, v)); v = OP(v, wave_dpp<0x141, 0xF>(idn, v)); v = OP(v, wave_dpp<0x140, 0xF>(idn, v)); \
    v = OP(v, wave_dpp<0x142, 0xA>(idn, v)); v = OP(v, wave_dpp<0x143, 0xC>(idn, v)); } while (0)
__device__ __forceinline__ uint32_t wr_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t wr_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t wr_add(uint32_t a, uint32_t b) { return a + b; }
__device__ __forceinline__ uint32_t wave_max(uint32_t v) { FGX_WAVE_REDUCE(v, 0u, wr_max); return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }
__device__ __forceinline__ uint32_t wave_min(uint32_t v) { FGX_WAVE_REDUCE(v, 0xFFFFFFFFu, wr_min); return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { FGX_WAVE_REDUCE(v, 0u, wr_add); return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }
__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v) { for (int o = 32; o > 0; o >>= 1) { unsigned long long t = __shfl_xor(v, o); v = t > v ? t : v; } return v; }
__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v) { for (int o = 32; o > 0; o >>= 1) { unsigned long long t = __shfl_xor(v, o); v = t < v ? t : v; } return v; }
__device__ __forceinline__ uint8_t comp_code(uint8_t c) { return (uint8_t)((0xF7B3D591E6A2C480ULL >> (4 * (c & 15))) & 15); }
// The overlap step skips a pair with an unmapped member (overlapping.rs:236-240), whatever ref_id / pos say — two unmapped mates at -1 / -1, or an
// unmapped read placed at its partner's position, would show a full shared span.  The simplex record kernels find a pair's span behind
// `ref_id == mate's ref_id`: an unmapped record `idx` (its index in the family) takes this value in place of its ref_id (which nothing else reads) —
// below every reference id, different for any two records — so that the test fails without a second flag word travelling across lanes.
__device__ __forceinline__ int32_t unmapped_ref_key(uint32_t idx) { return (int32_t)(0x80000000u | idx); }
// Does an end (fragments / R1s / R2s) of the family hold unmapped AND mapped records?  drop_unmapped_if_any_mapped (vanilla_caller.rs:1206-1232) then
// works from the final lengths: the streaming kernels hand such a family to k_family_wave<0>.  `bal(p)`: the family's part of a ballot (every lane takes part).
template <class Bal>
__device__ __forceinline__ bool mixed_unmapped_end(const bool act, const uint32_t flags, Bal&& bal) {
  const auto all = bal(act), um = bal(act && (flags & bam::F_UNMAPPED));
  const auto e0 = bal(act && !(flags & bam::F_PAIRED)), e1 = bal(act && (flags & bam::F_PAIRED) && (flags & bam::F_FIRST));
  const auto e2 = all & ~(e0 | e1), mp = all & ~um;
  return ((e0 & um) && (e0 & mp)) || ((e1 & um) && (e1 & mp)) || ((e2 & um) && (e2 & mp));
}

// unaligned LDS reads built from aligned dwords (v_alignbyte_b32)
__device__ __forceinline__ uint32_t ldsw(const uint8_t* W, uint32_t o) { return *(const uint32_t*)(W + o); }
#ifndef FGX_LDS_UNALIGNED
#define FGX_LDS_UNALIGNED 1   /* gfx950 LDS takes unaligned ds_read_b32 / b64: one instruction instead of two or three aligned reads + alignbyte */
#endif
__device__ __forceinline__ uint32_t ld32u(const uint8_t* W, uint32_t o) {
#if FGX_LDS_UNALIGNED
  uint32_t v;
  __builtin_memcpy(&v, W + o, 4);
  return v;
#else
  uint32_t a = o & ~3u;
  return __builtin_amdgcn_alignbyte(ldsw(W, a + 4), ldsw(W, a), o & 3);
#endif
}
__device__ __forceinline__ unsigned long long ld64u(const uint8_t* W, uint32_t o) {
#if FGX_LDS_UNALIGNED
  unsigned long long v;
  __builtin_memcpy(&v, W + o, 8);
  return v;
#else
  uint32_t a = o & ~3u, sh = o & 3;
  uint32_t w0 = ldsw(W, a), w1 = ldsw(W, a + 4), w2 = ldsw(W, a + 8);
  return (unsigned long long)__builtin_amdgcn_alignbyte(w1, w0, sh) | ((unsigned long long)__builtin_amdgcn_alignbyte(w2, w1, sh) << 32);
#endif
}
// unaligned reads of global memory (a record's fields lie at any byte offset).  record_writers.inc keeps a pair of its own with the same bodies (gld32u / gld64u):
// calling these from the writers instead changes k_emit's register allocation (profiles/record_core.md)
__device__ __forceinline__ uint32_t gld32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ unsigned long long gld64(const uint8_t* p) { unsigned long long v; __builtin_memcpy(&v, p, 8); return v; }
// offset of the first NUL in W[o, o+n), 8 bytes per step; -1 if none
__device__ __forceinline__ int find_nul64(const uint8_t* W, uint32_t o, uint32_t n) {
  for (uint32_t i = 0; i < n; i += 8) {
    unsigned long long v = ld64u(W, o + i);
    unsigned long long t = (v - 0x0101010101010101ULL) & ~v & 0x8080808080808080ULL;
    if (t) { uint32_t k = i + ((uint32_t)__builtin_ctzll(t) >> 3); return k < n ? (int)k : -1; }
  }
  return -1;
}

// Aux walk of one record per lane, in LDS (tags.rs:13-34): first occurrence of MC / <tag> / RX / <cell tag>.
// The walk keeps its state in integer lanes (bit 0 MC, 1 <tag>, 2 RX, 3 <cell tag>) and picks with selects: boolean state
// would live in scalar lane masks, and every `if` on it costs scalar mask instructions for all 64 records.
// (what the walk finds: AuxTags, record_core.h)
// cls: aux value type -> 1 / 2 / 4 (fixed size), 8 (Z), 16 (H), 32 (B), 0 (unknown).  The table lies in device memory, built at compile time
// (round 6): a wavefront copies it with one load and one LDS store.  Until round 5 every workgroup COMPUTED its 256 entries (a switch per
// entry: ~190 vector instructions per wavefront — a quarter of k_split_parse's instructions per family, whose wavefronts live for one round
// of 64 records).
struct TagClassTable {
  uint8_t v[256];
  constexpr TagClassTable() : v{} {
    v['A'] = 1; v['c'] = 1; v['C'] = 1; v['s'] = 2; v['S'] = 2; v['i'] = 4; v['I'] = 4; v['f'] = 4; v['Z'] = 8; v['H'] = 16; v['B'] = 32;
  }
};
__device__ const TagClassTable g_tag_classes = TagClassTable();
static_assert(TagClassTable().v['i'] == 4 && TagClassTable().v['Z'] == 8 && TagClassTable().v['x'] == 0, "tag classes");
__device__ __forceinline__ void fill_tag_classes(uint8_t* cls /* 256 bytes of LDS, 4-byte aligned */) {
  if (threadIdx.x < 64u) ((uint32_t*)cls)[threadIdx.x] = ((const uint32_t*)g_tag_classes.v)[threadIdx.x];
}
template <class ParamsT>
__device__ __forceinline__ void aux_walk(const uint8_t* W, const uint8_t* cls_of, uint32_t a0, uint32_t an, const ParamsT& P, AuxTags& A) {
  uint32_t q = 0, seen = 0, got = 0, oddw = 0;
  uint32_t pk_mc = 0, pk_mi = 0, pk_rx = 0, pk_cb = 0;
  const uint32_t key_mi = (uint32_t)(uint8_t)P.tag0 | ((uint32_t)(uint8_t)P.tag1 << 8);
  const uint32_t key_cb = P.cell0 ? ((uint32_t)(uint8_t)P.cell0 | ((uint32_t)(uint8_t)P.cell1 << 8)) : 0xFFFFFFFFu;   // (no key is > 0xFFFF)
  while (q + 3 <= an) {
    const uint32_t hd = ld32u(W, a0 + q);
    const uint32_t key = hd & 0xFFFF, cls = cls_of[(hd >> 16) & 0xFF];
    const uint32_t rem = an - (q + 3);
    uint32_t size = cls & 7, zend = 0;
    uint32_t stop = cls == 0 ? 1u : 0u;                    // a key match at an entry of unknown size still counts as seen
    if (cls & 24) {
      const int z = find_nul64(W, a0 + q + 3, rem);
      if (z < 0) break;                                    // unterminated: nothing here or after it is reachable
      zend = (uint32_t)z; size = zend + 1;
    }
    if (cls & 32) {
      if (rem < 5) break;
      const uint32_t es = cls_of[hd >> 24] & 7;
      const unsigned long long sz = 5ull + (unsigned long long)ld32u(W, a0 + q + 4) * (unsigned long long)es;
      if (sz > 0xFFFFFFFFull) break;
      size = (uint32_t)sz;
      stop = es == 0 ? 1u : 0u;
    }
    const uint32_t kb = (key == ('M' | ('C' << 8)) ? 1u : 0u) | (key == key_mi ? 2u : 0u) | (key == ('R' | ('X' << 8)) ? 4u : 0u) | (key == key_cb ? 8u : 0u);
    const uint32_t fresh = kb & ~seen;                     // first occurrence of its key
    seen |= kb;
    const uint32_t zb = cls == 8 ? fresh : 0u;             // ... with a Z value
    const uint32_t rec = zend > 255 ? (zb & 1u) : zb;      // values longer than 255 bytes: only MC may be (it is then not `<n>M`)
    oddw |= zb & ~rec;
    got |= rec;
    const uint32_t pk = (a0 + q + 3) | ((zend < 0xFFFFu ? zend : 0xFFFFu) << 16);
    pk_mc = (rec & 1u) ? pk : pk_mc; pk_mi = (rec & 2u) ? pk : pk_mi; pk_rx = (rec & 4u) ? pk : pk_rx; pk_cb = (rec & 8u) ? pk : pk_cb;
    const unsigned long long nq = (unsigned long long)q + 3 + size;
    if (stop || nq > an) break;
    q = (uint32_t)nq;
  }
  A.got = got; A.oddw = oddw; A.pk_mc = pk_mc; A.pk_mi = pk_mi; A.pk_rx = pk_rx; A.pk_cb = pk_cb;
}

#ifndef FGX_PHASE_TIMING
#define FGX_PHASE_TIMING 0   /* 1: per-phase s_memtime deltas of k_family_wave into g_phase (profiling builds only) */
#endif
#if FGX_PHASE_TIMING
__device__ unsigned long long g_phase[64 * 16];
#define PH(i) { unsigned long long _n = __builtin_amdgcn_s_memtime(); if (lane == 0) atomicAdd(&g_phase[(blockIdx.x & 63) * 16 + (i)], _n - _t); _t = _n; }
#else
#define PH(i)
#endif
#if FGX_PHASE_TIMING
#define PHB(i) { __syncthreads(); unsigned long long _n = __builtin_amdgcn_s_memtime(); if (threadIdx.x == 0) atomicAdd(&g_phase[(blockIdx.x & 63) * 16 + (i)], _n - _tb); _tb = _n; }
#else
#define PHB(i)
#endif
__global__ __launch_bounds__(NT) void k_family(FastParams P) {
  FGX_DYN_LDS(dyn);
  __shared__ Shared S;
  __shared__ __align__(16) double sPairB[94][2];   // {correct[q], error_per_alt[q]}: one LDS read per observation instead of two global ones
  __shared__ __align__(16) uint8_t sTagCls[256];   // aux value type classes (aux_walk)
  const uint32_t tid = threadIdx.x;
  if (tid < 94) { sPairB[tid][0] = P.T->t.correct[tid]; sPairB[tid][1] = P.T->t.error_per_alt[tid]; }
  fill_tag_classes(sTagCls);
  const uint32_t g = P.group_list ? P.group_list[blockIdx.x] : P.g0 + blockIdx.x;
  const uint32_t r0 = P.grp_first[g], r1 = P.grp_first[g + 1];
  const uint32_t n = r1 - r0;
  const uint32_t slot0 = 3 * g;

  if (tid < FGX_STATS_LEN) S.stats[tid] = 0;
  if (tid == 0) { S.defer = 0; S.n_ends = 0; S.rx_bad = 0; S.raw_lo = ~0ull; S.raw_hi = 0ull; S.any_complex = 0; }
  if (tid < 3) { P.ends[slot0 + tid].valid = 0; P.rec_sizes[slot0 + tid] = 0; }
  __syncthreads();

  // ---- group-level short circuit (simplex.rs:673-683) ---------------------------------------------
  if (n < P.min_reads) {
    if (tid == 0) {
      unsigned long long* st = P.stats + (size_t)(blockIdx.x & (STAT_SLOTS - 1)) * 32;
      atomicAdd(&st[0], (unsigned long long)n);
      atomicAdd(&st[2], (unsigned long long)n);
      atomicAdd(&st[3 + FGX_REJ_INSUFFICIENT_READS], (unsigned long long)n);
    }
    return;
  }
  if (n > FAST_MAX_READS) {
    if (tid == 0) { uint32_t k = atomicAdd(P.n_deferred, 1u); P.deferred[k] = g; }
    return;
  }

#if FGX_PHASE_TIMING
  unsigned long long _tb = __builtin_amdgcn_s_memtime();
#endif
  // ---- 0. the family's raw records into LDS with coalesced 16-byte loads: everything below (tag walk, name compares,
  // unpacking of bases and qualities) reads LDS instead of walking HBM byte by byte ------------------------------------
  {
    unsigned long long off = tid < n ? P.rec_off[r0 + tid] : ~0ull, end = tid < n ? P.rec_off[r0 + tid] + P.rec_len[r0 + tid] : 0ull;
    for (int o = 32; o > 0; o >>= 1) { unsigned long long a = __shfl_xor(off, o), b = __shfl_xor(end, o); off = a < off ? a : off; end = b > end ? b : end; }
    if ((tid & 63) == 0) { atomicMin(&S.raw_lo, off); atomicMax(&S.raw_hi, end); }
  }
  __syncthreads();
  const unsigned long long base16 = S.raw_lo & ~15ull;
  const uint32_t raw_bytes = (uint32_t)(((S.raw_hi - base16) + 15 + 16) & ~15ull);      // + slack for multi-byte reads past the last record
  if ((S.raw_hi - base16) + 32 > (unsigned long long)P.lds_tile_bytes || S.raw_hi > P.blob_len) {   // not even the raw span fits (or a record ends outside the blob)
    if (tid == 0) { uint32_t k = atomicAdd(P.n_deferred, 1u); P.deferred[k] = g; }
    return;
  }
  for (uint32_t i = tid * 16; i < raw_bytes - 16; i += NT * 16) *(uint4*)(dyn + i) = *(const uint4*)(P.blob + base16 + i);
  __syncthreads();
  const uint8_t* const blobL = dyn - base16;          // blobL + <offset in the blob> addresses the LDS copy

  PHB(9)
  // ---- 1. parse one record per lane -----------------------------------------------------------------
  if (tid < n) {
    ReadInfo R;
    memset(&R, 0, sizeof(R));
    R.mate = -1;
    R.end = 255;
    uint64_t off = P.rec_off[r0 + tid];
    uint32_t len = P.rec_len[r0 + tid];
    const uint8_t* p = blobL + off;
    R.goff = off;
    bool bad = len < 32;
    if (!bad) {
      uint32_t l_name = p[8], n_cig = rd16(p + 12), l_seq = rd32(p + 16);
      uint16_t flag = rd16(p + 14);
      uint64_t seq_off = 32ull + l_name + 4ull * n_cig;
      uint64_t qual_off = seq_off + ((uint64_t)l_seq + 1) / 2;
      uint64_t aux_off = qual_off + l_seq;
      if (aux_off > len || l_seq > 65535 || l_name == 0) bad = true;
      else {
        R.flags = flag; R.l_seq = (uint16_t)l_seq; R.seq_off = (uint16_t)seq_off; R.name_len = (uint16_t)(l_name - 1);
        R.pos = (int32_t)rd32(p + 4); R.ref_id = (int32_t)rd32(p);
        R.excluded = (flag & (bam::F_SECONDARY | bam::F_SUPPLEMENTARY)) ? 1 : 0;
        // CIGAR: up to WG_CIG_OPS ops of any kind (clips, indels, skips); consensus is called in query space, the CIGAR matters
        // for the mate clip, the overlap correction and the alignment filter
        uint32_t ops[WG_CIG_OPS];
        uint32_t n_ops = 0;
        for (uint32_t i = 0; i < WG_CIG_OPS; i++) ops[i] = 0;
        if (!R.excluded) {
          if ((flag & bam::F_UNMAPPED) || n_cig == 0 || n_cig > WG_CIG_OPS || l_seq == 0 || R.pos < 0) bad = true;
          else {
            uint64_t qsum = 0;
            uint32_t ns = 0;
            for (uint32_t i = 0; i < n_cig; i++) {
              const uint32_t o = rd32(p + 32 + l_name + 4 * i), t = o & 15;
              ops[i] = o;
              if (t > 8 || (o >> 4) > 0x3FFFFFu) bad = true;
              if (t == 0 || t == 1 || t == 4 || t == 7 || t == 8) qsum += o >> 4;
              const uint32_t k = (t == 4 || t == 5 || t == 7 || t == 8) ? 0u : t;      // simplify_cigar (clipper.rs:1183-1210)
              if (ns > 0 && (S.scig[tid][ns - 1] & 15) == k) S.scig[tid][ns - 1] += (o >> 4) << 4;
              else S.scig[tid][ns++] = ((o >> 4) << 4) | k;
            }
            n_ops = n_cig;
            S.n_scig[tid] = (uint8_t)ns;
            if (qsum != l_seq) bad = true;          // SEQ and CIGAR disagree: the general path decides
            if (n_cig != 1 || (ops[0] & 15) == 1) S.any_complex = 1;
          }
        }
        // aux walk: first occurrence of MC / <tag> / RX / <cell tag>; malformed aux stops the walk (tags.rs:13-34)
        const uint32_t lo_r = (uint32_t)(off - base16);            // LDS offset of this record
        if ((unsigned long long)lo_r + len > 65535ull) bad = true;  // (the walk packs LDS offsets into 16 bits: tiles beyond 64 KB defer)
        int mc_off = -1; uint32_t mc_len = 0;
        {
          AuxTags ax;
          aux_walk(dyn, sTagCls, lo_r + (uint32_t)aux_off, (uint32_t)(len - aux_off), P, ax);
          if (ax.oddw) bad = true;                                  // <tag> / RX / <cell tag> value longer than 255 bytes
          if (ax.got & 1u) { mc_off = (int)((ax.pk_mc & 0xFFFF) - lo_r); mc_len = ax.pk_mc >> 16; }
          const uint32_t mi_o = (ax.pk_mi & 0xFFFF) - lo_r, rx_o = (ax.pk_rx & 0xFFFF) - lo_r, cb_o = (ax.pk_cb & 0xFFFF) - lo_r;
          if (ax.got & 2u) { R.has_mi = 1; R.mi_off = (uint16_t)mi_o; R.mi_len = (uint8_t)(ax.pk_mi >> 16); }
          if (ax.got & 4u) { R.has_rx = 1; R.rx_off = (uint16_t)rx_o; R.rx_len = (uint8_t)(ax.pk_rx >> 16); }
          if (ax.got & 8u) { R.has_cb = 1; R.cb_off = (uint16_t)cb_o; R.cb_len = (uint8_t)(ax.pk_cb >> 16); }
        }
        if (!bad && !R.excluded) {
          // mate-overlap clip (raw-bam/overlap.rs:181-207)
          uint32_t mops[WG_MC_OPS];
          bool overflow = false;
          bam::Rec v{p, len};
          uint64_t clip = bam::mate_clip(v, ops, n_ops, mc_off >= 0 ? p + mc_off : nullptr, mc_len, mops, WG_MC_OPS, &overflow);
          if (overflow) bad = true;
          R.clip = (uint16_t)(clip > 65535 ? 65535 : clip);
          // name hash for mate pairing (a filter: candidates are compared word by word below)
          R.name_hash = record::name_hash30(R.name_len, [&](uint32_t o) { return ld32u(dyn, lo_r + 32 + o); }, [&](uint32_t o) { return ld64u(dyn, lo_r + 32 + o); });
        }
      }
    }
    if (bad) defer(S);
    S.ri[tid] = R;
  }
  __syncthreads();
  // UMI = MI tag of the first record (vanilla_caller.rs:1897-1908); missing → fatal in the reference
  if (tid == 0 && !S.defer) {
    if (!S.ri[0].has_mi) defer(S);
    else if ((uint32_t)P.prefix_len + 1 + S.ri[0].mi_len >= 255) defer(S);   // read name too long → fatal
    // LDS tile rows
    uint32_t row = 0;
    for (uint32_t i = 0; i < n; i++) { S.ri[i].row = row; if (!S.ri[i].excluded) row += ((uint32_t)S.ri[i].l_seq + 3) & ~3u; }
    S.tile_bytes = row;
    if ((unsigned long long)raw_bytes + 2ull * row > P.lds_tile_bytes && !S.defer) S.defer = P.retry ? 2 : 1;
  }
  __syncthreads();
  if (S.defer) {
    if (tid == 0) {
      if (S.defer == 2) { uint32_t k = atomicAdd(P.n_retry, 1u); P.retry[k] = g; }
      else { uint32_t k = atomicAdd(P.n_deferred, 1u); P.deferred[k] = g; }
    }
    return;
  }
  uint8_t* lb = dyn + raw_bytes;
  uint8_t* lq = lb + S.tile_bytes;

  PHB(10)
  // ---- 2. stage bases (unpacked 4-bit codes) and quals into LDS -------------------------------------
  for (uint32_t r = tid >> 6; r < n; r += NT / 64) {          // one wavefront per record: NT / 64 records in flight
    const ReadInfo& R = S.ri[r];
    if (R.excluded) continue;
    const uint8_t* p = blobL + R.goff;
    const uint8_t* sq = p + R.seq_off;
    const uint8_t* ql = sq + ((uint32_t)R.l_seq + 1) / 2;
    for (uint32_t i = tid & 63; i < R.l_seq; i += 64) {
      uint8_t b = sq[i >> 1];
      lb[R.row + i] = (i & 1) ? (b & 0xF) : (b >> 4);
      lq[R.row + i] = ql[i];
    }
  }
  // absent qualities (every byte 0xFF) are a fatal input error in the reference (:1119-1124) → general path
  __syncthreads();
  if (tid < n && !S.ri[tid].excluded) {
    // serial re-check only when the first qual is 0xFF (cheap early-out; the all-0xFF case is a fatal error)
    const ReadInfo& R = S.ri[tid];
    if (lq[R.row] == 0xFF) {
      bool all = true;
      for (uint32_t i = 0; i < R.l_seq; i++) if (lq[R.row + i] != 0xFF) { all = false; break; }
      if (all) defer(S);
    }
  }
  __syncthreads();
  if (S.defer) {
    if (tid == 0) { uint32_t k = atomicAdd(P.n_deferred, 1u); P.deferred[k] = g; }
    return;
  }

  PHB(11)
  // ---- 3. overlapping-bases pre-correction (overlapping.rs:236-336, 627-684) ------------------------
  if (P.overlap) {
    // pair map semantics: for each name the LAST primary record with FIRST set and the LAST with (not FIRST and) LAST set.
    // One wavefront per R1 candidate, the lanes test 64 records at a time (n <= 128: two steps).
    {
      const uint32_t wave_p = tid >> 6, lane_p = tid & 63;
      for (uint32_t a = wave_p; a < n; a += NT / 64) {
        const ReadInfo& R = S.ri[a];
        if (R.excluded || !(R.flags & bam::F_FIRST)) continue;
        const uint32_t rh = R.name_hash, rl_ = R.name_len;
        uint64_t later_r1[2], r2s[2];
        for (int c = 0; c < 2; c++) {
          const uint32_t u = lane_p + 64u * c;
          bool is_later_r1 = false, is_r2 = false;
          if (u < n) {
            const ReadInfo& O = S.ri[u];
            if (!O.excluded && O.name_hash == rh && O.name_len == rl_) {
              const bool first = (O.flags & bam::F_FIRST) != 0;
              const bool cand = first ? (u > a) : ((O.flags & bam::F_LAST) != 0);
              if (cand) {
                const uint32_t on = (uint32_t)(O.goff - base16) + 32, nn = (uint32_t)(R.goff - base16) + 32;
                unsigned long long diff = 0;                  // whole 8-byte steps + the last 8 bytes (names of one length)
                uint32_t i = 0;
                for (; i + 8 <= rl_; i += 8) diff |= ld64u(dyn, on + i) ^ ld64u(dyn, nn + i);
                if (i < rl_) {
                  if (rl_ >= 8) diff |= ld64u(dyn, on + rl_ - 8) ^ ld64u(dyn, nn + rl_ - 8);
                  else diff |= (ld64u(dyn, on) ^ ld64u(dyn, nn)) & ((1ULL << (8 * rl_)) - 1ULL);
                }
                const bool same = diff == 0;
                is_later_r1 = same && first; is_r2 = same && !first;
              }
            }
          }
          later_r1[c] = __ballot(is_later_r1); r2s[c] = __ballot(is_r2);
        }
        if (lane_p == 0 && !(later_r1[0] | later_r1[1])) {
          int m = -1;
          if (r2s[1]) m = 64 + (63 - __clzll((long long)r2s[1]));
          else if (r2s[0]) m = 63 - __clzll((long long)r2s[0]);
          S.ri[a].mate = (int16_t)m;
        }
      }
    }
    __syncthreads();
    uint32_t ov_bases = 0, ov_agree = 0, ov_dis = 0, ov_corr = 0;
    const uint32_t wave = tid >> 6, lane = tid & 63;
    for (uint32_t a = wave; a < n; a += NT / 64) {     // pairs are disjoint, so their order does not matter
      const ReadInfo& A = S.ri[a];
      if (A.mate < 0) continue;
      const ReadInfo& B = S.ri[A.mate];
      if (A.ref_id != B.ref_id) continue;
      // both CIGARs out of the LDS copy of the records; positions shared by two aligned blocks are corrected (overlapping.rs:236-336)
      uint32_t na = 1, nb = 1;
      uint32_t oa[WG_CIG_OPS], ob[WG_CIG_OPS];
      int32_t rla = A.l_seq, rlb = B.l_seq;
      oa[0] = (uint32_t)A.l_seq << 4; ob[0] = (uint32_t)B.l_seq << 4;     // family of single-block reads: <l_seq>M, nothing to look up
      if (S.any_complex) {
        const uint8_t* pa = blobL + A.goff;
        const uint8_t* pb = blobL + B.goff;
        na = rd16(pa + 12); nb = rd16(pb + 12);
        for (uint32_t i = 0; i < WG_CIG_OPS; i++) {
          oa[i] = i < na ? rd32(pa + 32 + A.name_len + 1 + 4 * i) : 0u;
          ob[i] = i < nb ? rd32(pb + 32 + B.name_len + 1 + 4 * i) : 0u;
        }
        rla = bam::ref_len_checked0(oa, na); rlb = bam::ref_len_checked0(ob, nb);
      }
      if (rla == 0 || rlb == 0) continue;
      const int64_t s1 = (int64_t)A.pos + 1, e1 = (int64_t)A.pos + rla, s2 = (int64_t)B.pos + 1, e2 = (int64_t)B.pos + rlb;
      const int64_t lo = s1 > s2 ? s1 : s2, hi = e1 < e2 ? e1 : e2;
      const bool plain = !S.any_complex;                     // both reads are one aligned block: query offset = x - start
      for (int64_t x = lo + lane; x <= hi; x += 64) {
        int32_t i1, i2;
        if (plain) { i1 = (int32_t)(x - s1); i2 = (int32_t)(x - s2); }
        else { i1 = map_ref_to_query(oa, na, s1, x, A.l_seq); i2 = map_ref_to_query(ob, nb, s2, x, B.l_seq); }
        if (i1 < 0 || i2 < 0) continue;
        const uint32_t ia = A.row + (uint32_t)i1, ib = B.row + (uint32_t)i2;
        uint8_t c1 = lb[ia], c2 = lb[ib];
        if (c1 == 15 || c2 == 15) continue;
        ov_bases++;
        uint8_t qa = lq[ia], qb = lq[ib];
        if (c1 == c2) {
          ov_agree++;
          uint32_t s = (uint32_t)qa + qb;
          uint8_t nq = (uint8_t)(s < 93 ? s : 93);
          lq[ia] = nq; lq[ib] = nq;
          if (nq != qa || nq != qb) ov_corr++;
        } else {
          ov_dis++;
          uint8_t cb, cq;
          if (qa == qb) { cb = 15; cq = FGX_MIN_PHRED; }
          else if (qa > qb) { cb = c1; cq = (uint8_t)(qa - qb); if (cq < FGX_MIN_PHRED) cq = FGX_MIN_PHRED; }
          else { cb = c2; cq = (uint8_t)(qb - qa); if (cq < FGX_MIN_PHRED) cq = FGX_MIN_PHRED; }
          lb[ia] = cb; lb[ib] = cb; lq[ia] = cq; lq[ib] = cq;
          ov_corr += 2;
        }
      }
    }
    if (ov_bases) atomicAdd(&S.stats[24], ov_bases);
    if (ov_agree) atomicAdd(&S.stats[25], ov_agree);
    if (ov_dis) atomicAdd(&S.stats[26], ov_dis);
    if (ov_corr) atomicAdd(&S.stats[27], ov_corr);
    __syncthreads();
  }

  PHB(12)
  // ---- 4. per-read source-read geometry (vanilla_caller.rs:1129-1160) ---------------------------------
  if (tid < n && !S.ri[tid].excluded) {
    ReadInfo& R = S.ri[tid];
    bool rev = (R.flags & bam::F_REVERSE) != 0;
    uint32_t L = R.l_seq;
    uint32_t trim_to = L;
    if (P.trim) {   // find_quality_trim_point on the oriented qualities (:992-1016)
      uint32_t tq = P.min_input_bq;
      if (tq < 1 || L == 0) trim_to = 0;
      else {
        int32_t score = 0, max_score = 0;
        uint32_t point = L;
        for (uint32_t i = L; i-- > 0;) {
          uint32_t idx = rev ? L - 1 - i : i;
          score += (int32_t)tq - (int32_t)lq[R.row + idx];
          if (score < 0) break;
          if (score > max_score) { max_score = score; point = i; }
        }
        trim_to = point;
      }
    }
    R.trim_to = (uint16_t)trim_to;
    uint32_t clip_pos = L > R.clip ? L - R.clip : 0;
    uint32_t fl = clip_pos < trim_to ? clip_pos : trim_to;
    while (fl > 0) {
      uint8_t c, q;
      oriented(S, lb, lq, R, fl - 1, P.min_input_bq, &c, &q);
      if (c != 15) break;
      fl--;
    }
    R.final_len = (uint16_t)fl;
    R.zero_len = fl == 0;
  }
  __syncthreads();

  PHB(13)
  // ---- 5. family gates (process_group :1329-1422, process_subgroup :1454-1646) -------------------------
  // One thread per record (n <= FAST_MAX_READS = 128: two wavefronts); counts are barrier-counts, the member lists are
  // built with ballots, and thread 0 only takes the scalar decisions.
  {
    if (tid < 3) { S.g_best[tid] = 0; S.g_rxcnt[tid] = 0; S.g_rxpos[tid] = 0xFFFFFFFFu; S.g_rxbad[tid] = 0; S.g_wcnt[0][tid] = 0; S.g_wcnt[1][tid] = 0; }
    const bool mine = tid < n;
    const bool exc = mine && S.ri[tid].excluded;
    const uint32_t n_sec = (uint32_t)__syncthreads_count(exc);
    const uint32_t n_reads = n - n_sec;
    bool go = n_reads > 0 && n_reads >= P.min_reads;
    uint32_t my_end = 255;
    bool my_zero = false;
    if (go && mine && !exc) {
      ReadInfo& R = S.ri[tid];
      if (!(R.flags & bam::F_PAIRED)) my_end = 0;
      else if (R.flags & bam::F_FIRST) my_end = 1;
      else if (R.flags & bam::F_LAST) my_end = 2;
      R.end = (uint8_t)my_end;
      my_zero = R.zero_len != 0;
    }
    uint32_t cnt[3], zero[3], rem[3], first[3] = {0, 0, 0};
    bool ok[3] = {false, false, false};
    for (int e = 0; e < 3; e++) {
      cnt[e] = (uint32_t)__syncthreads_count(my_end == (uint32_t)e);
      zero[e] = (uint32_t)__syncthreads_count(my_end == (uint32_t)e && my_zero);
      rem[e] = cnt[e] - zero[e];
    }
    // alignment filter (filter_source_reads_by_alignment :1242-1296): only when some read of the family has clips or indels —
    // reads with one aligned block all fall into one prefix-compatible group
    uint32_t minor[3] = {0, 0, 0};
    bool my_minor = false;
    if (go && S.any_complex) {
      if (tid == 0)
        for (uint32_t e = 0; e < 3; e++)
          if (cnt[e] >= P.min_reads && rem[e] >= P.min_reads && rem[e] >= 2) alignment_filter(S, e, n);
      __syncthreads();
      my_minor = my_end < 3 && !my_zero && S.ri[tid].minority != 0;
      for (int e = 0; e < 3; e++) minor[e] = (uint32_t)__syncthreads_count(my_minor && my_end == (uint32_t)e);
    }
    bool want_defer = false;
    uint32_t n_members = 0;
    uint32_t kept[3] = {0, 0, 0};               // reads of the end after the zero-length drop and the alignment filter
    uint32_t down[3] = {0, 0, 0};               // ... of which --max-reads drops
    bool bites = false;
    for (int e = 0; e < 3; e++) {
      if (!go || cnt[e] == 0 || cnt[e] < P.min_reads || rem[e] < P.min_reads) continue;
      kept[e] = rem[e] - minor[e];
      if (kept[e] >= P.min_reads && P.max_reads >= 0 && (int64_t)kept[e] > P.max_reads) bites = true;
    }
    bool my_down = false;
    if (bites) {   // downsample_filtered_source_reads (:902-932): the max_reads lowest fgbio name ranks stay, ties in file order
      const bool cand = my_end < 3 && !my_zero && !my_minor && kept[my_end] >= P.min_reads && (int64_t)kept[my_end] > P.max_reads;
      if (cand) S.name_rank[tid] = name_rank(blobL + S.ri[tid].goff + 32, S.ri[tid].name_len);
      __syncthreads();
      if (cand) {
        const int32_t rk = S.name_rank[tid];
        uint32_t before = 0;
        for (uint32_t j = 0; j < n; j++) {
          const ReadInfo& O = S.ri[j];
          if (j == tid || O.end != my_end || O.zero_len || O.minority) continue;
          const int32_t rj = S.name_rank[j];
          before += (rj < rk || (rj == rk && j < tid)) ? 1u : 0u;
        }
        my_down = (int64_t)before >= P.max_reads;
      }
      for (int e = 0; e < 3; e++) down[e] = (uint32_t)__syncthreads_count(my_down && my_end == (uint32_t)e);
    }
    uint32_t fin[3] = {0, 0, 0};                // reads of the end that go into the consensus
    for (int e = 0; e < 3; e++) {
      if (!go || cnt[e] == 0 || cnt[e] < P.min_reads || rem[e] < P.min_reads || kept[e] < P.min_reads) continue;
      fin[e] = kept[e] - down[e];
      if (fin[e] < P.min_reads) continue;
      ok[e] = true; first[e] = n_members; n_members += fin[e];
    }
    // member lists: file order inside an end
    const bool keep = my_end < 3 && ok[my_end] && !my_zero && !my_minor && !my_down;
    const uint32_t wv = tid >> 6, ln = tid & 63;
    uint32_t my_rank = 0;
    for (int e = 0; e < 3; e++) {
      const uint64_t bm = __ballot(keep && my_end == (uint32_t)e);
      if (wv < 2 && ln == 0) S.g_wcnt[wv][e] = (uint32_t)__popcll(bm);
      if (keep && my_end == (uint32_t)e) my_rank = (uint32_t)__popcll(bm & ((1ull << ln) - 1));
    }
    __syncthreads();
    uint32_t my_pos = 0;                      // position inside the end's member list
    if (keep) {
      my_pos = my_rank + (wv == 1 ? S.g_wcnt[0][my_end] : 0);
      S.members[first[my_end] + my_pos] = (uint16_t)tid;
      const ReadInfo& R = S.ri[tid];
      if (P.min_reads <= 1) atomicMax(&S.g_best[my_end], (uint32_t)R.final_len);      // consensus length = the longest kept read
      if (R.has_rx) { atomicAdd(&S.g_rxcnt[my_end], 1u); atomicMin(&S.g_rxpos[my_end], my_pos); }
    }
    __syncthreads();
    if (keep) {
      const ReadInfo& R = S.ri[tid];
      if (P.min_reads > 1) {                  // min_reads-th longest kept read (:1661-1669): every kept read ranks itself
        const uint32_t la = R.final_len;
        uint32_t ge = 0;
        for (uint32_t bq = 0; bq < fin[my_end]; bq++) if (S.ri[S.members[first[my_end] + bq]].final_len >= la) ge++;
        if (ge >= P.min_reads) atomicMax(&S.g_best[my_end], la);
      }
      if (R.has_rx) {                         // UMIs of unequal length (vanilla_caller.rs:1842-1856 → consensus_umis panics)
        const uint32_t len0 = S.ri[S.members[first[my_end] + S.g_rxpos[my_end]]].rx_len;
        if (R.rx_len != len0) S.g_rxbad[my_end] = 1;
      }
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t* st = S.stats;
      st[0] += n;
      if (n_sec) { st[2] += n_sec; st[3 + FGX_REJ_SECONDARY_OR_SUPPLEMENTARY] += n_sec; }
      if (n_reads > 0 && n_reads < P.min_reads) { st[2] += n_reads; st[3 + FGX_REJ_INSUFFICIENT_READS] += n_reads; }
      if (want_defer) defer(S);
      if (go && !want_defer) {
        for (int e = 0; e < 3; e++) {
          if (cnt[e] == 0) continue;
          if (cnt[e] < P.min_reads) { st[2] += cnt[e]; st[3 + FGX_REJ_INSUFFICIENT_READS] += cnt[e]; continue; }
          if (zero[e]) { st[2] += zero[e]; st[3 + FGX_REJ_ZERO_LENGTH_AFTER_TRIMMING] += zero[e]; }
          if (rem[e] < P.min_reads) { if (rem[e]) { st[2] += rem[e]; st[3 + FGX_REJ_INSUFFICIENT_READS] += rem[e]; } continue; }
          if (minor[e]) { st[2] += minor[e]; st[3 + FGX_REJ_MINORITY_ALIGNMENT] += minor[e]; }
          if (kept[e] < P.min_reads) { if (kept[e]) { st[2] += kept[e]; st[3 + FGX_REJ_INSUFFICIENT_READS] += kept[e]; } continue; }
          if (down[e]) { st[2] += down[e]; st[3 + FGX_REJ_DOWNSAMPLED] += down[e]; }
          if (fin[e] < P.min_reads && fin[e]) { st[2] += fin[e]; st[3 + FGX_REJ_INSUFFICIENT_READS] += fin[e]; }
        }
      }
      if (!S.defer) {
        uint32_t ne = 0;
        auto push_end = [&](uint32_t e) {
          S.end_type[ne] = e; S.end_first[ne] = first[e]; S.end_cnt[ne] = fin[e]; S.end_len[ne] = S.g_best[e];
          S.end_maxd[ne] = 0; S.end_mind[ne] = 0xFFFFFFFFu; S.end_sumd[ne] = 0; S.end_sume[ne] = 0;
          // UMIs carried by the kept reads of this end
          const uint32_t rc = S.g_rxcnt[e];
          const uint32_t fr = rc ? S.members[first[e] + S.g_rxpos[e]] : 0;
          const uint32_t len0 = rc ? S.ri[fr].rx_len : 0;
          S.end_rx_cnt[ne] = rc; S.end_rx_len[ne] = len0; S.end_rx_first[ne] = fr;
          if (rc > 1 && S.g_rxbad[e]) defer(S);          // consensus_umis panics on unequal lengths → general path reports it
          if (rc >= 1 && len0 > FAST_RX_CAP) defer(S);
          ne++;
        };
        if (ok[0]) { st[1] += 1; push_end(0); }
        if (ok[1] && ok[2]) { st[1] += 2; push_end(1); push_end(2); }
        else if (ok[1]) { st[2] += fin[1]; st[3 + FGX_REJ_ORPHAN_CONSENSUS] += fin[1]; }
        else if (ok[2]) { st[2] += fin[2]; st[3 + FGX_REJ_ORPHAN_CONSENSUS] += fin[2]; }
        uint32_t total = 0;
        for (uint32_t k = 0; k < ne; k++) { S.end_coloff[k] = total; total += S.end_len[k]; }
        S.n_ends = ne;
        S.col_base = P.col_base[g];   // deterministic scratch slot: exclusive scan of the per-family column bound
      }
    }
  }
  __syncthreads();
  if (S.defer) {
    if (tid == 0) { uint32_t k = atomicAdd(P.n_deferred, 1u); P.deferred[k] = g; }
    return;
  }

  PHB(14)
  // ---- 6. consensus columns (create_consensus_from_source_reads :1652-1755) -------------------------
  const DeviceTables* T = P.T;
  const uint32_t ne = S.n_ends;
  uint32_t total_cols = ne ? S.end_coloff[ne - 1] + S.end_len[ne - 1] : 0;
  for (uint32_t c = tid; c < total_cols; c += NT) {
    uint32_t k = 0;
    while (k + 1 < ne && c >= S.end_coloff[k + 1]) k++;
    uint32_t p = c - S.end_coloff[k];
    uint32_t m0 = S.end_first[k], mc = S.end_cnt[k];
    uint8_t ob, oq;
    uint32_t depth, err;
    if (mc == 1) {   // single-read consensus: LUT keyed by the unclamped quality (:1677-1708)
      uint8_t code, q;
      oriented(S, lb, lq, S.ri[S.members[m0]], p, P.min_input_bq, &code, &q);
      uint8_t adj = q < 94 ? T->single_input_quals[q] : 0;
      if (adj < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; } else { ob = code; oq = adj; }
      depth = code != 15 ? 1 : 0;
      err = 0;
    } else {
      ChainAcc acc;                             // two Kahan chains while the column shows one base (consensus_math.h)
      acc.reset();
      for (uint32_t a = 0; a < mc; a++) {
        const ReadInfo& R = S.ri[S.members[m0 + a]];
        if (p < R.final_len) {
          uint8_t code, q;
          oriented(S, lb, lq, R, p, P.min_input_bq, &code, &q);
          // N (incl. masked) and IUPAC codes contribute nothing: only the one-hot codes A C G T are observations
          const uint32_t qq = q < FGX_MAX_PHRED ? q : FGX_MAX_PHRED;
          const double2 pr = *(const double2*)&sPairB[qq][0];
          acc.add(__popc((uint32_t)code) == 1, code, pr.x, pr.y);
        }
      }
      double ll[4];
      uint32_t obs[4];
      acc.finish(ll, obs);
      int bi;
      uint8_t q;
      column_call(T->t, ll, obs, &bi, &q);
      depth = obs[0] + obs[1] + obs[2] + obs[3];
      err = depth - (bi == 0 ? obs[0] : bi == 1 ? obs[1] : bi == 2 ? obs[2] : bi == 3 ? obs[3] : 0u);
      const uint8_t LANE_CODE[4] = {1, 2, 4, 8};
      uint8_t code = bi >= 0 ? LANE_CODE[bi] : 15;
      if (depth < P.min_reads) { ob = 15; oq = 0; }
      else if (q < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; }
      else { ob = code; oq = q; }
    }
    uint32_t d16 = depth < 32767u ? depth : 32767u, e16 = err < 32767u ? err : 32767u;
    uint64_t o = S.col_base + c;
    P.col_code[o] = ob; P.col_qual[o] = oq; P.col_depth[o] = (uint16_t)d16; P.col_err[o] = (uint16_t)e16;
    atomicMax(&S.end_maxd[k], d16); atomicMin(&S.end_mind[k], d16); atomicAdd(&S.end_sumd[k], d16); atomicAdd(&S.end_sume[k], e16);
  }

  PHB(15)
  // ---- 7. consensus UMI per end (simple_umi.rs:46-117): Q20 observations at (Q90, Q90) -----------------
  {
    const DeviceTables* TU = P.TU;
    for (uint32_t w = tid; w < ne * FAST_RX_CAP; w += NT) {
      uint32_t k = w / FAST_RX_CAP, i = w % FAST_RX_CAP;
      uint32_t cnt = S.end_rx_cnt[k];
      if (cnt == 0 || i >= S.end_rx_len[k]) continue;
      if (cnt == 1) { const ReadInfo& R = S.ri[S.end_rx_first[k]]; S.end_rx[k][i] = (char)blobL[R.goff + R.rx_off + i]; continue; }
      ColumnAcc acc;
      acc.reset();
      uint32_t non_dna = 0, seen = 0;
      uint8_t fc = 0;
      bool mixed = false;
      for (uint32_t a = 0; a < S.end_cnt[k]; a++) {
        const ReadInfo& R = S.ri[S.members[S.end_first[k] + a]];
        if (!R.has_rx) continue;
        uint8_t ch = blobL[R.goff + R.rx_off + i];
        if (seen == 0) fc = ch;
        seen++;
        uint8_t up = (ch >= 'a' && ch <= 'z') ? (uint8_t)(ch - 32) : ch;
        bool dna = up == 'A' || up == 'C' || up == 'G' || up == 'T' || up == 'N';
        if (dna) { int lane = bam::ascii_to_lane(ch); if (lane != 255) acc.add(lane, TU->t.correct[20], TU->t.error_per_alt[20]); }
        else { non_dna++; if (ch != fc) mixed = true; }
      }
      char out;
      if (non_dna == 0) { int bi; uint8_t q; column_call(TU->t, acc.s, acc.obs, &bi, &q); out = bi >= 0 ? "ACGT"[bi] : 'N'; }
      else if (non_dna == seen && !mixed) out = (char)fc;
      else { out = '?'; S.rx_bad = 1; }      // the reference panics here
      S.end_rx[k][i] = out;
    }
  }
  __syncthreads();
  if (S.rx_bad) {   // undo: the general path raises the reference's error
    if (tid == 0) { uint32_t k = atomicAdd(P.n_deferred, 1u); P.deferred[k] = g; }
    return;
  }

  // ---- 8. descriptors + stats ---------------------------------------------------------------------------
  if (tid < ne) {
    uint32_t k = tid;
    EndDesc D;
    memset(&D, 0, sizeof(D));
    uint32_t Lc = S.end_len[k];
    D.col_off = S.col_base + S.end_coloff[k];
    D.cons_len = Lc;
    D.first_off = S.ri[0].goff;
    D.kept_off = S.ri[S.members[S.end_first[k]]].goff;
    D.type = (uint8_t)S.end_type[k];
    const uint32_t maxd = Lc ? S.end_maxd[k] : 0, mind = Lc ? S.end_mind[k] : 0;   // widths of the cD / cM integer tags
    D.mi_off = S.ri[0].mi_off; D.mi_len = S.ri[0].mi_len;
    const ReadInfo& F = S.ri[S.members[S.end_first[k]]];
    D.has_cb = (P.cell0 && F.has_cb) ? 1 : 0; D.cb_off = F.cb_off; D.cb_len = F.cb_len;
    D.has_rx = S.end_rx_cnt[k] > 0; D.rx_len = (uint8_t)S.end_rx_len[k];
    for (uint32_t i = 0; i < D.rx_len; i++) D.rx[i] = S.end_rx[k][i];
    D.valid = 1;
    uint32_t name_len = P.prefix_len + 1 + D.mi_len;
    uint32_t size = 32 + name_len + 1 + (Lc + 1) / 2 + Lc + (3 + P.rg_len + 1) + (3 + int_tag_width(maxd)) + (3 + int_tag_width(mind)) + 7 +
                    (P.per_base_tags ? 2 * (8 + 2 * Lc) : 0) + (3 + D.mi_len + 1) + (D.has_cb ? 3 + D.cb_len + 1 : 0) +
                    (D.has_rx ? 3 + D.rx_len + 1 : 0);
    D.rec_size = size;
    // emission order inside a family: fragment, R1, R2 → slot = end type
    P.ends[slot0 + D.type] = D;
    P.rec_sizes[slot0 + D.type] = (uint64_t)size + 4;
  }
  if (tid < FGX_STATS_LEN && S.stats[tid]) atomicAdd(&P.stats[(size_t)(blockIdx.x & (STAT_SLOTS - 1)) * 32 + tid], (unsigned long long)S.stats[tid]);
}

// -----------------------------------------------------------------------------------------------------
// k_family_wave — the common case: ONE WAVEFRONT PER FAMILY (≤ 64 records whose raw bytes fit the wave's
// LDS slice).  The family's records are contiguous in the BAM stream, so the wave copies that byte span
// into LDS with coalesced 16-byte loads (one pass over HBM at full line efficiency) and then does ALL
// parsing, aux-tag walking, overlap correction and column reads out of LDS.  Lane r owns record r; per-read
// state lives in lane r's registers and is broadcast with v_readlane, the family gates are ballots and
// popcounts — no serial lane-0 section and no block barrier.  Semantics identical to k_family below.
// -----------------------------------------------------------------------------------------------------
// column_call_fast for the wave kernel: same decisions as consensus_math.h's unanimous_fast_path, arranged for the
// GPU — the four likelihoods stay in registers (selects instead of dynamic indexing, which would go through scratch
// memory) and the bracket q with thresholds[q] <= gap < thresholds[q+1] comes from the qguess hint plus ONE parallel
// probe of five neighbouring thresholds instead of a 7-step dependent binary search through LDS.
__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long u) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
  return ((unsigned long long)hi << 32) | lo;
}
// Methylation-aware mode, the canonical second pass (FGX_METH_CANON=1): the reference runs of record `rec` of the batch — its canon::RefRuns as dwords, read
// through the scalar unit (constant address space: the canonical pass wrote them a kernel boundary ago) — or null when the batch carries none.  The
// table's address is the word behind the contig lengths (contig_len[n_ref]; fill_params writes it with every batch), so that FastParams stays as it is.
// `rec` is wave-uniform.
typedef const FGX_CONST_AS uint32_t* RefRunsPtr;
__device__ __forceinline__ RefRunsPtr meth_ref_runs(const FastParams& P, uint32_t rec) {
  const unsigned long long tab = uniform_u64(P.contig_len[P.n_ref]);
  if (!tab) return nullptr;
  return (RefRunsPtr)(uintptr_t)uniform_u64(tab + (unsigned long long)rec * sizeof(canon::RefRuns));
}
__device__ __forceinline__ double uniform_f64(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ double sel4(const double* v, uint32_t i) { return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3]; }
__device__ __forceinline__ bool column_call_fast_lds(const ConsensusTables& T, const CallConst& K, const double* ll, const uint32_t* obs,
                                                     int* base_idx, uint8_t* qual) {
  if (obs[0] + obs[1] + obs[2] + obs[3] == 0) { *base_idx = -1; *qual = FGX_MIN_PHRED; return true; }
  const uint32_t n_obs = (obs[0] > 0) + (obs[1] > 0) + (obs[2] > 0) + (obs[3] > 0);
  if (n_obs != 1) return false;
  const uint32_t observed = obs[3] > 0 ? 3u : obs[2] > 0 ? 2u : obs[1] > 0 ? 1u : 0u;
  const double w = sel4(ll, observed), l = sel4(ll, (observed + 1) & 3);
  const double gap = w - l;
  if (!(m_isfinite(gap) && gap > FGX_DBL_EPSILON)) return false;
  if (gap >= K.cap_threshold) {
    const double delta = unanimous_margin(w, l, 1.0);
    if (gap - K.cap_threshold >= FGX_LN_2 && delta < K.half_cerr_at_cap) { *base_idx = (int)observed; *qual = (uint8_t)K.cap; return true; }
    return false;
  }
  uint32_t lo;
  double thq, thq1;
  bool probed = false;
  if (gap < 32.0) {
    const uint32_t b = T.qguess[(uint32_t)(gap * 8.0)];            // thresholds[0..b) <= gap for sure; b >= 1 (thresholds[0] = 0)
    if (b >= 1) {
      double t[5];
#pragma unroll
      for (int j = 0; j < 5; j++) { uint32_t idx = b - 1 + j; t[j] = T.thresholds[idx < 93 ? idx : 93]; }
      const uint32_t c = (t[1] <= gap) + (t[2] <= gap) + (t[3] <= gap) + (t[4] <= gap);
      if (c < 4) { lo = b + c; thq = c == 0 ? t[0] : c == 1 ? t[1] : c == 2 ? t[2] : t[3]; thq1 = c == 0 ? t[1] : c == 1 ? t[2] : c == 2 ? t[3] : t[4]; probed = true; }
    }
  }
  if (!probed) {
    uint32_t a = 0, hi = 94;
    while (a < hi) { uint32_t mid = a + (hi - a) / 2; if (T.thresholds[mid] <= gap) a = mid + 1; else hi = mid; }
    lo = a; thq = T.thresholds[lo - 1]; thq1 = T.thresholds[lo];
  }
  const uint32_t q = lo - 1;
  const double margin = unanimous_margin(w, l, T.cerr_min[q]);
  if (gap - thq > margin && thq1 - gap > margin) { *base_idx = (int)observed; *qual = (uint8_t)q; return true; }
  return false;
}

#ifndef FGX_WAVE_OCC
#define FGX_WAVE_OCC 5   /* measured on MI355X, 1M depth-8 families: occ 4 19.2 ms, 5 17.2 ms, 6 18.1 ms */
#endif
// MODE 0: simplex (vanilla caller).  MODE 1: duplex — phases 1-4 are shared, the strand partition, the four single-strand
// column sets and the descriptors of the two duplex records replace phases 5-8 (see the MODE == 1 branch).
// What k_family_wave keeps in LDS beside the wave slices, as one block with a host-built image (FastPath::d_fwimg), copied like
// k_simplex_wave2's (W2Lds): 16-byte loads that leave with the family's first loads, LDS writes after the records are staged.
struct FwLds {
  ConsensusTables t;                 // thresholds / cerr_min / scalars (and the plain tables for reference)
  alignas(16) double pair[94][2];    // {correct[q], error_per_alt[q]} interleaved: one ds_read_b128 per observation
  uint8_t tagcls[256];               // aux value type classes (aux_walk)
};
static_assert(sizeof(FwLds) % 16 == 0 && sizeof(FwLds) <= 6 * 64 * 16, "FwLds is copied in 16-byte pieces, six per thread at most");
inline void build_fw_image(FwLds& L, const ConsensusTables& t) {
  memset(&L, 0, sizeof(L));
  L.t = t;
  for (uint32_t i = 0; i < 94; i++) { L.pair[i][0] = t.correct[i]; L.pair[i][1] = t.error_per_alt[i]; }
  for (uint32_t i = 0; i < 256; i++) { const int fx = bam::tag_fixed_size((uint8_t)i); L.tagcls[i] = (uint8_t)(fx ? fx : i == 'Z' ? 8 : i == 'H' ? 16 : i == 'B' ? 32 : 0); }
}

// METH 1 (duplex only): the methylation-aware mode — per read set the anchor read's place on the reference, the unconverted / converted counts of every
// column and converted bases read as unconverted ones before they are observed (see 6D); molecules with a record of more than one CIGAR op are deferred.
// CAP 1 (duplex): the build of a caller with --max-reads-per-strand — a read set above the cap is scored over its `cap` lowest name ranks, walked in
// (rank, file order), and the observations of ALL its reads are counted beside them for the duplex error recount (see 5D / 6D); CAP 0 is the kernel without any of it.
// METH 1 with CAP 1: the reference annotates and normalises a set AHEAD of the cap, so a capped set's anchor, its unconverted / converted counts and the recount's
// bases are those of every read (count_all), normalised; the scoring loops normalise what they observe and leave the counts alone.
// CAP 1 (CODEC): the build of a caller with --max-reads-per-strand — the R1 list and the R2 list are cut to their `cap` lowest name ranks ahead of the geometry (5C).
// Wave-aggregated append of the columns (and UMI characters) whose call needs call_full to the global FullItem lists (k_call_full works through them
// densely): one atomic with its return value per wavefront and list tried; a full list chains to the next one, only a globally full pool overflows.  Every
// lane of the wavefront takes part; `obs_packed`: the four observation counts, a byte each.  Returns: this lane's item found no room (list overflow).
__device__ __forceinline__ bool push_full_global(const FastParams& P, const uint32_t lane, const uint32_t my_list, const bool need, const uint64_t dest, const double* ll,
                                                 const uint32_t obs_packed, const uint32_t chains) {
  bool pending = need;
  uint32_t l = my_list;
  for (uint32_t tries = 0;; tries++) {
    const unsigned long long m = __ballot(pending);
    if (!m) return false;
    if (tries >= N_LISTS) return pending;
    const uint32_t cnt = (uint32_t)__popcll(m), leader = (uint32_t)__builtin_ctzll(m);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&P.full_count[l], cnt);
    base = (uint32_t)__shfl((int)base, (int)leader);
    if (pending) {
      const uint32_t idx = base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
      if (idx < P.full_cap) {
        FullItem* it = &P.full_items[(size_t)l * P.full_cap + idx];
        it->dest = dest; it->ll[0] = ll[0]; it->ll[1] = ll[1]; it->ll[2] = ll[2]; it->ll[3] = ll[3];
        it->obs = obs_packed; it->chains = chains;
        pending = false;
      }
    }
    l = (l + 1) & (N_LISTS - 1);
  }
}

template <int MODE, int METH = 0, int CAP = 0>
#ifndef FGX_WAVE_OCC_DUPLEX
#define FGX_WAVE_OCC_DUPLEX 4   /* the duplex branch holds four column sets' worth of state beside the record lanes: at 5 waves per SIMD (96 VGPRs) its
                                   member loop spilled */
#endif
__global__ __launch_bounds__(256, MODE == 1 ? FGX_WAVE_OCC_DUPLEX : FGX_WAVE_OCC) void k_family_wave(FastParams P, uint32_t n_grp_total) {
  FGX_DYN_LDS(dyn);
  __shared__ __align__(16) FwLds sL;
  ConsensusTables& sT = sL.t;
  double (&sPair)[94][2] = sL.pair;
  uint8_t* const sTagCls = sL.tagcls;
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t gi_raw = blockIdx.x * (blockDim.x >> 6) + wv;   // n_grp_total counts the groups of this launch (all of them, or a retry list)
  bool bail = gi_raw >= n_grp_total;                          // a wavefront without a group still takes part in the table copy
  const uint32_t gi = bail ? 0u : gi_raw;
  const uint32_t g = P.group_list ? P.group_list[gi] : P.g0 + gi;   // (asked for before the image: waiting for it does not wait for the image)
  // the table image: global -> registers now, registers -> LDS after the records have been staged (one barrier for both)
  constexpr uint32_t IMG_V = (uint32_t)(sizeof(FwLds) / 16);
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4* const img_src = (const u32x4*)P.fw_image;
  const uint32_t ii0 = threadIdx.x, ii1 = ii0 + blockDim.x, ii2 = ii1 + blockDim.x, ii3 = ii2 + blockDim.x, ii4 = ii3 + blockDim.x, ii5 = ii4 + blockDim.x;
  const u32x4 im0 = img_src[ii0 < IMG_V ? ii0 : 0u], im1 = img_src[ii1 < IMG_V ? ii1 : 0u], im2 = img_src[ii2 < IMG_V ? ii2 : 0u],
              im3 = img_src[ii3 < IMG_V ? ii3 : 0u], im4 = img_src[ii4 < IMG_V ? ii4 : 0u], im5 = img_src[ii5 < IMG_V ? ii5 : 0u];
  uint8_t* W = dyn + (size_t)wv * P.lds_wave_bytes;
  const uint32_t my_list = blockIdx.x & (N_LISTS - 1);
  bool list_overflow = false;
  auto push_full = [&](bool need, uint64_t dest, const double* ll, const uint32_t* obs) {
    list_overflow |= push_full_global(P, lane, my_list, need, dest, ll, obs[0] | (obs[1] << 8) | (obs[2] << 16) | (obs[3] << 24), 0u);
  };
  unsigned long long* st = P.stats + (size_t)(blockIdx.x & (STAT_SLOTS - 1)) * 32;
  const uint32_t r0 = P.grp_first[g], n = P.grp_first[g + 1] - r0;
  const uint32_t slot0 = 3 * g;
  if (!bail && lane < 3) { if (MODE == 0) P.ends[slot0 + lane].valid = 0; else if (MODE == 1) P.dends[slot0 + lane].valid = 0; else P.cends[slot0 + lane].valid = 0; P.rec_sizes[slot0 + lane] = 0; }

  if (MODE == 0 && !bail && n < P.min_reads) {   // simplex.rs:673-683
    if (lane == 0) { atomicAdd(&st[0], (unsigned long long)n); atomicAdd(&st[2], (unsigned long long)n); atomicAdd(&st[3 + FGX_REJ_INSUFFICIENT_READS], (unsigned long long)n); }
    bail = true;
  }
  auto to_defer = [&]() { if (lane == 0) { uint32_t k = atomicAdd(P.n_deferred, 1u); P.deferred[k] = g; } };
  // does not fit this launch's LDS slice: the next launch (bigger slices, fewer waves per CU) picks it up; after the last one
  // simplex families go to the workgroup-per-family kernel, duplex / CODEC molecules to the general path
  auto to_retry = [&]() { if (!P.retry) { to_defer(); return; } if (lane == 0) { uint32_t k = atomicAdd(P.n_retry, 1u); P.retry[k] = g; } };
  if (!bail && n > 64) {
    if (P.big) { if (lane == 0) { uint32_t k = atomicAdd(P.n_big, 1u); P.big[k] = g; } }   // k_family's, directly (duplex: duplex_deep.inc's list; CODEC: codec_deep.inc's)
    else if (MODE == 0) to_retry();
    else to_defer();
    bail = true;
  }
  // an empty group has no byte span (the minimum below would be ~0 and the staging loop would read the 16 bytes BEFORE the blob —
  // a fault when the blob starts an allocation): the general path emits its nothing
  if (!bail && n == 0) { to_defer(); bail = true; }

#if FGX_PHASE_TIMING
  unsigned long long _t = __builtin_amdgcn_s_memtime();
#endif
  // ---- 1. stage the family's raw records into LDS ------------------------------------------------------
  const bool act = !bail && lane < n;
  unsigned long long off = act ? P.rec_off[r0 + lane] : ~0ull;
  uint32_t len = act ? P.rec_len[r0 + lane] : 0;
  unsigned long long lo_off = wave_min64(off);
  unsigned long long hi_end = wave_max64(act ? off + len : 0ull);
  if (!bail && (__any(act && len < 32) || hi_end > P.blob_len)) { to_defer(); bail = true; }   // a record outside the blob: the general path raises the error
  unsigned long long base16 = lo_off & ~15ull;
  unsigned long long span = hi_end - base16;
  if (!bail && span + 16 > (unsigned long long)P.lds_wave_bytes) { to_retry(); bail = true; }   // +16: slack for the dword-composed reads
  const uint32_t span16 = bail ? 0u : ((uint32_t)span + 15) & ~15u;
  {
    const uint8_t* src = P.blob + base16;
    for (uint32_t i = lane * 16; i < span16; i += 64 * 16) *(uint4*)(W + i) = *(const uint4*)(src + i);
  }
  {
    u32x4* const img_dst = (u32x4*)&sL;
    if (ii0 < IMG_V) img_dst[ii0] = im0;
    if (ii1 < IMG_V) img_dst[ii1] = im1;
    if (ii2 < IMG_V) img_dst[ii2] = im2;
    if (ii3 < IMG_V) img_dst[ii3] = im3;
    if (ii4 < IMG_V) img_dst[ii4] = im4;
    if (ii5 < IMG_V) img_dst[ii5] = im5;
  }
  __syncthreads();                                            // the tables (workgroup) and this wavefront's records are in LDS
  if (bail) return;

  PH(1)
  // ---- 2. parse: lane r owns record r ---------------------------------------------------------------------
  const uint32_t lo = act ? (uint32_t)(off - base16) : 0;       // LDS offset of this lane's record
  uint32_t flags = 0, l_seq = 0, seq_lo = 0, qual_lo = 0, name_len = 0, clip = 0, hash = 0;
  int32_t pos = 0, ref_id = 0;
  uint32_t mi_lo = 0, mi_len = 0, rx_lo = 0, rx_len = 0, cb_lo = 0, cb_len = 0;   // LDS offsets of tag values
  bool has_mi = false, has_rx = false, has_cb = false, excluded = false, bad = false;
  bool long_cigar = false;          // simplex: more CIGAR ops than MAX_CIG_OPS — nothing below may index `ops` by them
  bool cplx = false;                // simplex: a CIGAR with I / D / N / P ops — the family goes to the workgroup-per-family kernel
  uint32_t lead_s = 0, m_len = 0;   // query offset of the first aligned base, length of the aligned block
  uint32_t tot_len = 0;             // (METH) the lengths of all the read's ops, hard clips included: the one M op simplify_cigar_from_raw makes of it
  bool multi = false;               // (METH) the record has more than one CIGAR op
  uint32_t strand = 0;   // duplex: 1 = MI ends in /A, 2 = /B
  if (act) {
    const record::FixedHeader H = record::decode_header(ld32u(W, lo), ld32u(W, lo + 4), ld32u(W, lo + 8), ld32u(W, lo + 12), ld32u(W, lo + 16));
    const record::Layout lay = record::layout(H, len);
    const uint32_t l_name = H.l_name, n_cig = H.n_cig;
    l_seq = H.l_seq; flags = H.flags;
    if (lay.odd) bad = true;
    else {
      name_len = l_name - 1;
      ref_id = H.ref_id; pos = H.pos;
      seq_lo = lo + lay.seq_off; qual_lo = lo + lay.qual_off;
      excluded = (flags & (bam::F_SECONDARY | bam::F_SUPPLEMENTARY)) != 0;
      if (MODE == 1 && excluded) bad = true;   // the duplex caller has no secondary/supplementary filter: general path
      // (methylation-aware mode: column p of a read set lies at the anchor's pos + p, or at pos + T - 1 - p, only when the reference makes ONE M op of the
      // read — clips around one aligned block, decided below; an indel read sends the molecule to the general path)
      if (MODE == 2 && (excluded || !(flags & bam::F_PAIRED))) bad = true;   // CODEC: fragments / non-primary records take the general path
      // CIGAR: one aligned block of M/=/X ops, optionally between soft / hard clips (what an aligner gives a read without
      // indels).  Such reads all simplify to (M, length) for the alignment filter; clips only shift query offsets.
      uint32_t ops[MAX_CIG_OPS];
      ops[0] = 0;
      // simplex: an unmapped record is a read without a CIGAR (create_source_read :1080-1190 looks at nothing else of it) — one block of l_seq query
      // bases, no clip against the mate, no part in the overlap step; ref_id / pos are never used (they may be -1 or the mate's values)
      const bool unm = MODE == 0 && METH == 0 && (flags & bam::F_UNMAPPED) && n_cig == 0;
      if (!excluded) {
        if (unm) { if (l_seq == 0) bad = true; m_len = l_seq; ref_id = unmapped_ref_key(lane); }
        else if ((flags & bam::F_UNMAPPED) || n_cig == 0 || l_seq == 0 || pos < 0) bad = true;
        else if (n_cig == 1) {
          ops[0] = ld32u(W, lo + 32 + l_name);
          const uint32_t ty = ops[0] & 15;
          if (!(ty == 0 || ty == 7 || ty == 8) || (ops[0] >> 4) != l_seq) bad = true;
          m_len = l_seq;
          if constexpr (METH != 0) tot_len = l_seq;
        } else if (MODE != 2 && n_cig <= MAX_CIG_OPS) {
          record::CigarBlock cb = record::cigar_block_start();   // clips around one aligned block; I, D, N, P (cplx): the workgroup kernel
#pragma unroll
          for (uint32_t i = 0; i < MAX_CIG_OPS; i++) {
            if (i >= n_cig) break;
            ops[i] = ld32u(W, lo + 32 + l_name + 4 * i);
            record::cigar_block_op(cb, ops[i]);
          }
          lead_s = cb.lead; m_len = cb.aln; cplx = cb.cplx;
          if constexpr (METH != 0) { tot_len = cb.tot; multi = true; }
          if (cplx && MODE == 0) { /* decided below: the whole family moves to the workgroup-per-family kernel */ }
          else if (!record::cigar_block_fits(cb, l_seq) || m_len > 65535) bad = true;
          if (METH != 0 && tot_len > 65535u) bad = true;
        } else if (MODE == 0 && n_cig <= WG_CIG_OPS) { cplx = true; long_cigar = true; }   // (more ops than this kernel reads: the workgroup kernel's)
        else bad = true;
      }
      // aux walk in LDS (tags.rs:13-34): first occurrence of MC / <tag> / RX / <cell tag>
      AuxTags ax;
      aux_walk(W, sTagCls, lo + lay.aux_off, len - lay.aux_off, P, ax);
      if (ax.oddw) bad = true;
      const record::TagFields tg = record::unpack_tags(ax);
      const bool has_mc = tg.has_mc;
      const uint32_t mc_lo = tg.mc_lo, mc_len = tg.mc_len;
      has_mi = tg.has_mi; mi_lo = tg.mi_lo; mi_len = tg.mi_len;
      has_rx = tg.has_rx; rx_lo = tg.rx_lo; rx_len = tg.rx_len;
      has_cb = tg.has_cb; cb_lo = tg.cb_lo; cb_len = tg.cb_len;
      if (MODE == 1) {   // strand from the MI suffix; every paired read needs `<id>/A` or `<id>/B` (duplex_caller.rs:2557-2566: fatal otherwise)
        if (has_mi && mi_len >= 2 && W[mi_lo + mi_len - 2] == '/') { const uint8_t sc = W[mi_lo + mi_len - 1]; strand = sc == 'A' ? 1u : sc == 'B' ? 2u : 0u; }
        if ((flags & bam::F_PAIRED) && (strand == 0 || P.prefix_len + 1 + (mi_len - 2) >= 255)) bad = true;
      }
      if (MODE == 2 && !bad) {   // is_fr_pair_raw of THIS record (overlap.rs:21-69); only the reverse record's answer is used
        const int32_t mpos = (int32_t)ld32u(W, lo + 24), mref = (int32_t)ld32u(W, lo + 20);
        if (pos >= record::POS_LIMIT || mpos < -1 || mpos >= record::POS_LIMIT) bad = true;
        const bool rv = (flags & bam::F_REVERSE) != 0, mrv = (flags & bam::F_MATE_REVERSE) != 0;
        const bool okp = !(flags & bam::F_MATE_UNMAPPED) && ref_id == mref && rv != mrv;
        strand = (okp && ((long long)mpos + 1 < (long long)pos + 1 + ((long long)l_seq - 1))) ? 1u : 0u;   // `strand` doubles as frself here
      }
      if (MODE != 2 && !bad && !excluded && !long_cigar && !unm) {
        // mate-overlap clip (raw-bam/overlap.rs:181-357).  Closed form when the MC tag is one M op and all
        // coordinates are in the ordinary range (no saturating arithmetic can trigger); general code otherwise.
        // (the guards of record::single_m_mate_clip: pos >= 0 and l_seq in 1 .. 65 535 hold for a record that is not bad, ML comes from at most seven digits)
        const uint32_t ML = (n_cig == 1 && has_mc) ? record::mc_single_m(mc_len, [&]() { return ld64u(W, mc_lo); }) : 0u;
        const record::MateFields M = record::decode_mate(ld32u(W, lo + 20), ld32u(W, lo + 24));
        if (ML != 0 && pos < record::POS_LIMIT && record::mate_in_range(M)) {
          clip = record::single_m_mate_clip(H, ref_id, M, (int32_t)ML);        // <= l_seq
        } else {
          uint32_t mops[MAX_MC_OPS];
          bool overflow = false;
          bam::Rec v{W + lo, len};
          unsigned long long cl = bam::mate_clip(v, ops, n_cig, has_mc ? W + mc_lo : nullptr, mc_len, mops, MAX_MC_OPS, &overflow);
          if (overflow) { if (MODE == 0) cplx = true; else bad = true; }   // (a mate of more ops than this kernel parses: the workgroup kernel's, which takes WG_MC_OPS)
          clip = (uint32_t)(cl > 65535 ? 65535 : cl);
        }
      }
      if (!bad && !excluded) {
        // name hash (8 bytes per step) for mate pairing
        unsigned long long h = 0x9E3779B97F4A7C15ULL ^ name_len;
        for (uint32_t i = 0; i < name_len; i += 8) {
          unsigned long long w = ld64u(W, lo + 32 + i);
          if (i + 8 > name_len) w &= (1ULL << (8 * (name_len - i))) - 1;
          h = (h ^ w) * 0xBF58476D1CE4E5B9ULL;
        }
        hash = (uint32_t)(h >> 32);
      }
    }
  }
  // first record must carry the MI tag and give a legal read name (vanilla_caller.rs:1897-1908, 1795-1797)
  const uint32_t mi0_lo = rlane(mi_lo, 0), mi0_len = rlane(mi_len, 0);
  if (MODE != 1 && lane == 0 && (!has_mi || P.prefix_len + 1 + mi_len >= 255)) bad = true;   // (CODEC without an MI names reads by a running counter: general path)
  // absent qualities (all 0xFF) are a fatal input error (:1119-1124)
  if (MODE != 2 && act && !bad && !excluded && W[qual_lo] == 0xFF) {
    bool all = true;
    for (uint32_t i = 0; i < l_seq; i++) if (W[qual_lo + i] != 0xFF) { all = false; break; }
    if (all) bad = true;
  }
  if (__any(bad)) { to_defer(); return; }
  if (MODE == 0 && __any(cplx)) { to_retry(); return; }
  const bool cand = act && !excluded;
  const bool rev = (flags & bam::F_REVERSE) != 0;
  const unsigned long long rxmask = __ballot(cand && has_rx), cbmask = __ballot(cand && has_cb);

  PH(2)
  // ---- 3. overlapping-bases pre-correction in LDS (overlapping.rs:236-336, 627-684) ----------------------
  uint32_t ov_bases = 0, ov_agree = 0, ov_dis = 0, ov_corr = 0;
  bool do_overlap = P.overlap != 0;
  if (MODE == 2) do_overlap = false;
  if (MODE == 1 && do_overlap && P.dmin_yx != 0)   // duplex.rs:786-795: only molecules with both strands when single-strand output is off
    do_overlap = n >= 2 && __any(act && strand == 1) && __any(act && strand == 2);
  if (do_overlap) {
    const bool is_r1 = cand && (flags & bam::F_FIRST);
    const bool is_r2 = cand && !(flags & bam::F_FIRST) && (flags & bam::F_LAST);
    // pair map: per name, the LAST R1-type and the LAST R2-type primary record
    int mate = -1;
    bool later_r1 = false;
    const unsigned long long r1mask = __ballot(is_r1), r2mask = __ballot(is_r2);
    // candidates of each R1 lane: the other R1/R2 lanes with the same (name hash, name length) — one compare per lane
    // pair here, the byte-wise name check below runs for all R1 lanes at once (usually a single round: the mate)
    uint32_t eq_lo = 0, eq_hi = 0;
    for (unsigned long long um = r1mask | r2mask; um; um &= um - 1) {
      const uint32_t u = (uint32_t)__builtin_ctzll(um);
      const uint32_t hash_u = rlane(hash, u), nlen_u = rlane(name_len, u);      // (both cross-lane reads by every lane: no short circuit between them)
      const bool eq = hash_u == hash && nlen_u == name_len && u != lane;
      if (u < 32) eq_lo |= (eq ? 1u : 0u) << u; else eq_hi |= (eq ? 1u : 0u) << (u - 32);
    }
    unsigned long long todo = is_r1 ? ((unsigned long long)eq_lo | ((unsigned long long)eq_hi << 32)) : 0ull;
    while (__any(todo != 0)) {
      const bool mine = todo != 0;
      const uint32_t u = mine ? (uint32_t)__builtin_ctzll(todo) : lane;
      todo &= todo - 1;
      const uint32_t lou = (uint32_t)__shfl((int)lo, (int)u);
      if (mine) {
        bool same = true;
        for (uint32_t i = 0; i < name_len; i += 8) {
          unsigned long long wa = ld64u(W, lou + 32 + i), wb = ld64u(W, lo + 32 + i);
          if (i + 8 > name_len) { unsigned long long mk = (1ULL << (8 * (name_len - i))) - 1; wa &= mk; wb &= mk; }
          if (wa != wb) { same = false; break; }
        }
        if (same) {
          if ((r1mask >> u) & 1) { if (u > lane) later_r1 = true; }
          else mate = (int)u;     // ascending u: the LAST R2-type record of the name wins
        }
      }
    }
    if (later_r1) mate = -1;
    // Every overlapping position of every pair is one work item; items are laid out pair after pair (exclusive scan
    // of the per-pair overlap lengths) and taken 64 at a time, so short overlaps of several pairs share an iteration.
    const int msrc = mate >= 0 ? mate : (int)lane;
    const int32_t pos_b = (int32_t)__shfl((int)pos, msrc), ref_b = (int32_t)__shfl((int)ref_id, msrc);
    const uint32_t aln_a = lead_s | (m_len << 16), aln_b = (uint32_t)__shfl((int)aln_a, msrc);   // query offset of the aligned block | its length
    const uint32_t dsc_a = seq_lo | (qual_lo << 16), dsc_b = (uint32_t)__shfl((int)dsc_a, msrc);
    uint32_t cntp = 0, off1 = 0, off2 = 0;
    if (mate >= 0 && ref_id == ref_b) {
      const long long s1 = (long long)pos + 1, e1 = (long long)pos + (aln_a >> 16), s2 = (long long)pos_b + 1, e2 = (long long)pos_b + (aln_b >> 16);
      const long long lox = s1 > s2 ? s1 : s2, hix = e1 < e2 ? e1 : e2;
      if (hix >= lox) { cntp = (uint32_t)(hix - lox + 1); off1 = (uint32_t)(lox - s1) + (aln_a & 0xFFFF); off2 = (uint32_t)(lox - s2) + (aln_b & 0xFFFF); }
    }
    uint32_t incl = cntp;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { uint32_t t = (uint32_t)__shfl_up((int)incl, o); if ((int)lane >= o) incl += t; }
    const uint32_t first_item = incl - cntp, n_items = rlane(incl, 63);
    for (uint32_t base = 0; base < n_items; base += 64) {
      const uint32_t w = base + lane;
      bool have = false;
      uint32_t i1 = 0, i2 = 0, sa = 0, sb = 0, qa0 = 0, qb0 = 0;
      for (unsigned long long pm = __ballot(cntp != 0 && first_item < base + 64 && first_item + cntp > base); pm; pm &= pm - 1) {
        const uint32_t a = (uint32_t)__builtin_ctzll(pm);
        const uint32_t st_a = rlane(first_item, a), cn_a = rlane(cntp, a), da = rlane(dsc_a, a), db = rlane(dsc_b, a);
        const uint32_t o1a = rlane(off1, a), o2a = rlane(off2, a);
        if (w >= st_a && w - st_a < cn_a) {
          have = true;
          i1 = o1a + (w - st_a); i2 = o2a + (w - st_a);
          sa = da & 0xFFFF; qa0 = da >> 16; sb = db & 0xFFFF; qb0 = db >> 16;
        }
      }
      if (have) {
        uint32_t o1 = sa + (i1 >> 1), o2 = sb + (i2 >> 1);
        uint8_t c1 = (i1 & 1) ? (W[o1] & 15) : (W[o1] >> 4), c2 = (i2 & 1) ? (W[o2] & 15) : (W[o2] >> 4);
        if (c1 != 15 && c2 != 15) {
          ov_bases++;
          uint8_t qa = W[qa0 + i1], qb = W[qb0 + i2];
          if (c1 == c2) {
            ov_agree++;
            uint32_t sm = (uint32_t)qa + qb;
            uint8_t nq = (uint8_t)(sm < 93 ? sm : 93);
            W[qa0 + i1] = nq; W[qb0 + i2] = nq;
            if (nq != qa || nq != qb) ov_corr++;
          } else {
            ov_dis++;
            uint8_t cb, cq;
            if (qa == qb) { cb = 15; cq = FGX_MIN_PHRED; }
            else if (qa > qb) { cb = c1; cq = (uint8_t)(qa - qb); if (cq < FGX_MIN_PHRED) cq = FGX_MIN_PHRED; }
            else { cb = c2; cq = (uint8_t)(qb - qa); if (cq < FGX_MIN_PHRED) cq = FGX_MIN_PHRED; }
            // nibble updates: neighbouring lanes own the other nibble of the same byte → 32-bit LDS atomics
            auto setn = [&](uint32_t o, uint32_t idx, uint8_t code) {
              uint32_t* wd = (uint32_t*)(W + (o & ~3u));
              uint32_t sh = 8 * (o & 3) + ((idx & 1) ? 0 : 4);
              atomicAnd(wd, ~(0xFu << sh));
              atomicOr(wd, (uint32_t)code << sh);
            };
            setn(o1, i1, cb); setn(o2, i2, cb);
            W[qa0 + i1] = cq; W[qb0 + i2] = cq;
            ov_corr += 2;
          }
        }
      }
    }
  }
  wave_sync();

  // Oriented, mask-aware view of one read at consensus position p.  d0 = seq_lo | qual_lo << 16, `rv` uniform.
  // Returns the 4-bit code in read orientation (15 = N / masked) and the SourceRead quality.
  auto view = [&](uint32_t s_lo, uint32_t q_lo, uint32_t L, bool rv, uint32_t trim_to, uint32_t p, uint32_t* code, uint32_t* qual) {
    uint32_t idx = rv ? L - 1 - p : p;
    uint32_t bb = W[s_lo + (idx >> 1)];
    uint32_t c = (bb >> ((~idx & 1) << 2)) & 15;
    uint32_t q = W[q_lo + idx];
    if (rv) c = comp_code((uint8_t)c);
    if (p < trim_to && q < P.min_input_bq) { c = 15; q = FGX_MIN_PHRED; }
    *code = c; *qual = q;
  };

  PH(3)
  // ---- 4. source-read geometry per lane (vanilla_caller.rs:1129-1160) -----------------------------------------
  uint32_t trim_to = l_seq, final_len = 0;
  if (MODE != 2 && cand && P.trim) {
    uint32_t tq = P.min_input_bq;
    if (tq < 1 || l_seq == 0) trim_to = 0;
    else {
      int32_t score = 0, max_score = 0;
      uint32_t point = l_seq;
      for (uint32_t i = l_seq; i-- > 0;) {
        uint32_t idx = rev ? l_seq - 1 - i : i;
        score += (int32_t)tq - (int32_t)W[qual_lo + idx];
        if (score < 0) break;
        if (score > max_score) { max_score = score; point = i; }
      }
      trim_to = point;
    }
  }
  if (MODE != 2) {
    uint32_t clip_pos = l_seq > clip ? l_seq - clip : 0;
    uint32_t fl = clip_pos < trim_to ? clip_pos : trim_to;
    bool tail_n = false;
    if (cand && fl > 0) { uint32_t c, q; view(seq_lo, qual_lo, l_seq, rev, trim_to, fl - 1, &c, &q); tail_n = (c == 15); }
    final_len = cand ? fl : 0;
    // reads ending in N / masked bases: strip the run 64 positions at a time (lanes scan backwards together)
    for (unsigned long long tm = __ballot(tail_n); tm; tm &= tm - 1) {
      const uint32_t r = (uint32_t)__builtin_ctzll(tm);
      uint32_t flr = rlane(final_len, r);
      const uint32_t s_r = rlane(seq_lo, r), q_r = rlane(qual_lo, r), L_r = rlane(l_seq, r), t_r = rlane(trim_to, r);
      const bool rv_r = (rlane(flags, r) & bam::F_REVERSE) != 0;
      while (flr > 0) {
        bool real = false;
        if (lane < flr) { uint32_t c, q; view(s_r, q_r, L_r, rv_r, t_r, flr - 1 - lane, &c, &q); real = (c != 15); }
        unsigned long long bm = __ballot(real);
        if (bm) { flr -= (uint32_t)__builtin_ctzll(bm); break; }
        flr -= flr < 64 ? flr : 64;
      }
      if (lane == r) final_len = flr;
    }
  }

  PH(4)
  if constexpr (MODE == 0) {
  // ---- 5. family gates with ballots (process_group :1329-1422, process_subgroup :1454-1646) -----------------
  uint32_t s_total = n, s_cons = 0, s_filtered = 0, s_sec = 0, s_insuf = 0, s_zero = 0, s_orphan = 0, s_down = 0, s_unm = 0;
  const uint32_t n_sec = (uint32_t)__popcll(__ballot(act && excluded));
  const uint32_t n_reads = n - n_sec;
  if (n_sec) { s_filtered += n_sec; s_sec = n_sec; }
  bool go = n_reads > 0;
  if (go && n_reads < P.min_reads) { s_filtered += n_reads; s_insuf += n_reads; go = false; }
  uint32_t my_end = 255;
  if (cand) { if (!(flags & bam::F_PAIRED)) my_end = 0; else if (flags & bam::F_FIRST) my_end = 1; else if (flags & bam::F_LAST) my_end = 2; }
  bool ok[3] = {false, false, false};
  unsigned long long mem[3] = {0, 0, 0};
  uint32_t surv[3] = {0, 0, 0}, clen[3] = {0, 0, 0};
  bool need_defer = false;
  if (go) {
#pragma unroll
    for (uint32_t e = 0; e < 3; e++) {
      unsigned long long in_e = __ballot(my_end == e);
      uint32_t cnt = (uint32_t)__popcll(in_e);
      if (cnt == 0) continue;
      if (cnt < P.min_reads) { s_filtered += cnt; s_insuf += cnt; continue; }
      unsigned long long kept = __ballot(my_end == e && final_len > 0);
      uint32_t rem = (uint32_t)__popcll(kept), zero = cnt - rem;
      if (zero) { s_filtered += zero; s_zero += zero; }
      if (rem < P.min_reads) { if (rem) { s_filtered += rem; s_insuf += rem; } continue; }
      {
        // drop_unmapped_if_any_mapped (:1206-1232), evaluated over the surviving source reads: an end that still holds a mapped read loses its
        // unmapped ones (Unmapped); everything below — alignment filter, --min-reads / --max-reads, consensus length, RX, cell barcode, orphan rule —
        // sees the mapped reads only, in file order.  An end whose mapped reads all trimmed to nothing keeps its unmapped reads.
        const unsigned long long un_e = __ballot(((kept >> lane) & 1) && (flags & bam::F_UNMAPPED));
        if (un_e != 0 && un_e != kept) {
          const uint32_t dropped = (uint32_t)__popcll(un_e);
          s_filtered += dropped; s_unm += dropped;
          kept &= ~un_e; rem -= dropped;
          if (rem < P.min_reads) { s_filtered += rem; s_insuf += rem; continue; }
        }
      }
      if (P.max_reads >= 0 && (long long)rem > P.max_reads) {
        // downsample_filtered_source_reads (:902-932): the max_reads lowest fgbio name ranks stay, ties in file order
        const int32_t rk = name_rank(W + lo + 32, name_len);
        const bool cand = (kept >> lane) & 1;
        uint32_t before = 0;
        for (unsigned long long m = kept; m; m &= m - 1) {
          const uint32_t j = (uint32_t)__builtin_ctzll(m);
          const int32_t rj = (int32_t)rlane((uint32_t)rk, j);
          before += (rj < rk || (rj == rk && j < lane)) ? 1u : 0u;
        }
        const unsigned long long stay = __ballot(cand && (long long)before < P.max_reads);
        const uint32_t dropped = rem - (uint32_t)__popcll(stay);
        s_filtered += dropped; s_down += dropped;
        kept = stay; rem = (uint32_t)__popcll(stay);
        if (rem < P.min_reads) { if (rem) { s_filtered += rem; s_insuf += rem; } continue; }
      }
      // consensus length = min_reads-th longest kept read
      bool mine = (kept >> lane) & 1;
      if (P.min_reads == 1) clen[e] = wave_max(mine ? final_len : 0);
      else {
        uint32_t ge = 0;
        for (unsigned long long m = kept; m; m &= m - 1) { uint32_t fj = rlane(final_len, (uint32_t)__builtin_ctzll(m)); ge += (fj >= final_len) ? 1 : 0; }
        clen[e] = wave_max((mine && ge >= P.min_reads) ? final_len : 0);
      }
      mem[e] = kept; surv[e] = rem; ok[e] = true;
    }
  }
  if (need_defer) { to_defer(); return; }
  // emitted ends in output order (Fragment, R1, R2), written with static indices only (a dynamically indexed local
  // array would live in scratch memory)
  uint32_t e_type[3], e_len[3], e_coloff[3];
  unsigned long long e_mem[3];
  const bool has_frag = ok[0], has_pair = ok[1] && ok[2];
  const uint32_t ne = (has_frag ? 1u : 0u) + (has_pair ? 2u : 0u);
  e_type[0] = has_frag ? 0u : 1u; e_len[0] = has_frag ? clen[0] : clen[1]; e_mem[0] = has_frag ? mem[0] : mem[1];
  e_type[1] = has_frag ? 1u : 2u; e_len[1] = has_frag ? clen[1] : clen[2]; e_mem[1] = has_frag ? mem[1] : mem[2];
  e_type[2] = 2u; e_len[2] = clen[2]; e_mem[2] = mem[2];
  if (has_frag) s_cons += 1;
  if (has_pair) s_cons += 2;
  else if (ok[1]) { s_filtered += surv[1]; s_orphan += surv[1]; }
  else if (ok[2]) { s_filtered += surv[2]; s_orphan += surv[2]; }
  uint32_t total_cols = 0;
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) if (k < ne) { e_coloff[k] = total_cols; total_cols += e_len[k]; }

  // UMIs carried by the kept reads of each end; unequal lengths → consensus_umis panics → general path
  uint32_t e_rx_cnt[3] = {0, 0, 0}, e_rx_len[3] = {0, 0, 0}, e_rx_first[3] = {0, 0, 0};
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    if (k >= ne) break;
    unsigned long long with = e_mem[k] & rxmask;
    uint32_t cnt = (uint32_t)__popcll(with);
    e_rx_cnt[k] = cnt;
    if (cnt) {
      uint32_t f = (uint32_t)__builtin_ctzll(with);
      e_rx_first[k] = f; e_rx_len[k] = rlane(rx_len, f);
      if (__any(((with >> lane) & 1) && rx_len != e_rx_len[k])) need_defer = true;
      if (e_rx_len[k] > FAST_RX_CAP) need_defer = true;
    }
  }
  if (need_defer) { to_defer(); return; }

  PH(5)
  // ---- 6. consensus columns: one lane per column, member reads walked in file order -------------------------
  // per-read descriptors packed for broadcast: d0 = seq_lo | qual_lo << 16 ; d1 = l_seq | final_len << 16 ; d2 = trim_to | rev << 16
  const uint32_t d0 = seq_lo | (qual_lo << 16), d1 = l_seq | (final_len << 16), d2 = trim_to | ((rev ? 1u : 0u) << 16);
  const DeviceTables* T = P.T;
  const uint64_t col_base = P.col_base[g];
  const uint32_t min_bq = P.min_input_bq;
  CallConst KC;   // wave-uniform, pinned into SGPRs (readfirstlane): no VGPRs held, nothing to spill
  KC.cap = (uint32_t)__builtin_amdgcn_readfirstlane((int)sT.cap);
  KC.cap_threshold = uniform_f64(sT.cap_threshold); KC.half_cerr_at_cap = uniform_f64(sT.half_cerr_at_cap);
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    if (k >= ne) break;
    const unsigned long long members = e_mem[k];
    const uint32_t mc = (uint32_t)__popcll(members);
    // (a wave-uniform trip count: the member loop reads lanes and push_full takes ballots — every lane takes part in the last pass too, `in` says whether it has a column)
    for (uint32_t p0 = 0; p0 < e_len[k]; p0 += 64) {
      const uint32_t p = p0 + lane;
      const bool in = p < e_len[k];
      uint8_t ob, oq;
      uint32_t depth, err;
      if (mc == 1) {   // single-read consensus: LUT keyed by the unclamped quality (:1677-1708)
        uint32_t r = (uint32_t)__builtin_ctzll(members);
        uint32_t code, q;
        view(rlane(seq_lo, r), rlane(qual_lo, r), rlane(l_seq, r), (rlane(flags, r) & bam::F_REVERSE) != 0, rlane(trim_to, r), in ? p : 0u, &code, &q);
        uint8_t adj = q < 94 ? T->single_input_quals[q] : 0;
        if (adj < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; } else { ob = (uint8_t)code; oq = adj; }
        depth = code != 15 ? 1 : 0;
        err = 0;
      } else {
        ChainAcc acc;                           // two Kahan chains while the column shows one base (consensus_math.h)
        acc.reset();
        for (unsigned long long m = members; m; m &= m - 1) {
          const uint32_t r = (uint32_t)__builtin_ctzll(m);
          const uint32_t x0 = rlane(d0, r), x1 = rlane(d1, r), x2 = rlane(d2, r);
          bool valid = p < (x1 >> 16);
          const bool rv = (x2 >> 16) != 0;
          const uint32_t idx = valid ? (rv ? (x1 & 0xFFFF) - 1 - p : p) : 0;
          const uint32_t bb = W[(x0 & 0xFFFF) + (idx >> 1)];
          const uint32_t c = (bb >> ((~idx & 1) << 2)) & 15;
          const uint32_t q = W[(x0 >> 16) + idx];
          // the code in read orientation (complement = bit reversal of the 4-bit code); only the one-hot codes A C G T count
          const uint32_t co = rv ? __builtin_bitreverse32(c) >> 28 : c;
          const bool masked = p < (x2 & 0xFFFF) && q < min_bq;
          valid = valid && __popc(co) == 1 && !masked;
          const uint32_t qq = q < FGX_MAX_PHRED ? q : FGX_MAX_PHRED;
          const double2 pr = *(const double2*)&sPair[qq][0];
          acc.add(valid, co, pr.x, pr.y);
        }
        double ll[4];
        uint32_t obs[4];
        acc.finish(ll, obs);
        int bi;
        uint8_t q;
        bool resolved = column_call_fast_lds(sT, KC, ll, obs, &bi, &q);
        depth = obs[0] + obs[1] + obs[2] + obs[3];
        uint64_t o = col_base + e_coloff[k] + p;
        uint32_t d16 = depth < 32767u ? depth : 32767u;
        if (in) P.col_depth[o] = (uint16_t)d16;
        push_full(in && !resolved, o, ll, obs);
        if (!in || !resolved) continue;    // code / qual / errors arrive from k_call_full
        err = depth - (bi == 0 ? obs[0] : bi == 1 ? obs[1] : bi == 2 ? obs[2] : bi == 3 ? obs[3] : 0u);
        uint8_t code = bi >= 0 ? (uint8_t)(1u << bi) : 15;
        if (depth < P.min_reads) { ob = 15; oq = 0; }
        else if (q < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; }
        else { ob = code; oq = q; }
        uint32_t e16 = err < 32767u ? err : 32767u;
        P.col_code[o] = ob; P.col_qual[o] = oq; P.col_err[o] = (uint16_t)e16;
        continue;
      }
      uint32_t d16 = depth < 32767u ? depth : 32767u, e16 = err < 32767u ? err : 32767u;
      uint64_t o = col_base + e_coloff[k] + p;
      if (in) { P.col_code[o] = ob; P.col_qual[o] = oq; P.col_depth[o] = (uint16_t)d16; P.col_err[o] = (uint16_t)e16; }
    }
  }

  PH(6)
  // ---- 7. consensus UMI per end (simple_umi.rs:46-117) ---------------------------------------------------------
  const DeviceTables* TU = P.TU;
  char my_rx[3] = {0, 0, 0};      // lane i holds character i of each end's consensus UMI
  bool rx_bad = false;
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    if (k >= ne) break;
    if (e_rx_cnt[k] == 0) continue;                     // uniform
    const bool mychar = lane < e_rx_len[k];
    if (e_rx_cnt[k] == 1) { if (mychar) my_rx[k] = (char)W[rlane(rx_lo, e_rx_first[k]) + lane]; continue; }
    // Byte-identical UMIs (the usual case) need no arithmetic: n >= 2 agreeing observations of base b leave b the
    // strict maximum of the four likelihoods whatever n is, so the call is the upper-cased base; a column of N/n has
    // no observations and calls 'N'; a non-DNA character shared by every string is kept (simple_umi.rs:69-103).
    {
      const uint32_t f_lo = rlane(rx_lo, e_rx_first[k]), ulen = e_rx_len[k];
      bool differs = false;
      if ((e_mem[k] & rxmask) >> lane & 1) {
        for (uint32_t i = 0; i < ulen; i += 8) {
          unsigned long long a = ld64u(W, rx_lo + i), b = ld64u(W, f_lo + i);
          if (i + 8 > ulen) { unsigned long long mk = (1ULL << (8 * (ulen - i))) - 1; a &= mk; b &= mk; }
          differs |= a != b;
        }
      }
      if (!__any(differs)) {
        if (mychar) {
          const uint8_t ch = W[f_lo + lane];
          const int bl = bam::ascii_to_lane(ch);
          my_rx[k] = bl != 255 ? "ACGT"[bl] : (ch == 'N' || ch == 'n') ? 'N' : (char)ch;
        }
        continue;
      }
    }
    // UMIs that differ (sequencing errors inside a family): per-character likelihood columns
    ColumnAcc acc;
    acc.reset();
    uint32_t non_dna = 0, seen = 0;
    uint8_t fc = 0;
    bool mixed = false;
    const double uc = TU->t.correct[20], ue = TU->t.error_per_alt[20];
    for (unsigned long long m = e_mem[k] & rxmask; m; m &= m - 1) {
      uint32_t r = (uint32_t)__builtin_ctzll(m);
      uint8_t ch = mychar ? W[rlane(rx_lo, r) + lane] : (uint8_t)'A';
      if (seen == 0) fc = ch;
      seen++;
      uint8_t up = (ch >= 'a' && ch <= 'z') ? (uint8_t)(ch - 32) : ch;
      bool dna = up == 'A' || up == 'C' || up == 'G' || up == 'T' || up == 'N';
      if (dna) { int bl = bam::ascii_to_lane(ch); if (bl != 255) acc.add(bl, uc, ue); }
      else { non_dna++; if (ch != fc) mixed = true; }
    }
    bool need_full = false;
    if (!mychar) { /* lanes past the UMI length only take part in the ballots below */ }
    else if (non_dna == 0) {
      int bi; uint8_t q;
      CallConst KU;
      KU.cap = TU->t.cap; KU.cap_threshold = TU->t.cap_threshold; KU.half_cerr_at_cap = TU->t.half_cerr_at_cap;
      bool resolved = column_call_fast_lds(TU->t, KU, acc.s, acc.obs, &bi, &q);
      my_rx[k] = bi >= 0 ? "ACGT"[bi] : 'N';
      need_full = !resolved;
    }
    else if (non_dna == seen && !mixed) my_rx[k] = (char)fc;
    else rx_bad = true;
    if (!mychar) { need_full = false; rx_bad = false; }
    push_full(need_full, (1ull << 63) | ((uint64_t)(slot0 + e_type[k]) << 8) | lane, acc.s, acc.obs);
  }
  if (__any(rx_bad) || __any(list_overflow)) { to_defer(); return; }

  PH(7)
  // ---- 8. descriptors + stats ---------------------------------------------------------------------------------------
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    if (k >= ne) break;
    uint32_t Lc = e_len[k];
    uint32_t slot = slot0 + e_type[k];
    EndDesc* D = &P.ends[slot];
    if (lane < e_rx_len[k] && e_rx_cnt[k]) D->rx[lane] = my_rx[k];
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
      D->has_rx = e_rx_cnt[k] > 0; D->rx_len = (uint8_t)e_rx_len[k];
      uint32_t nm = P.prefix_len + 1 + mi0_len;
      // cD / cM <= member count <= 64 → one-byte int tags (k_emit derives the values from the arrays)
      uint32_t size = 32 + nm + 1 + (Lc + 1) / 2 + Lc + (3 + P.rg_len + 1) + 4 + 4 + 7 +
                      (P.per_base_tags ? 2 * (8 + 2 * Lc) : 0) + (3 + mi0_len + 1) + (hcb ? 3 + fk_cb_len + 1 : 0) +
                      (e_rx_cnt[k] ? 3 + e_rx_len[k] + 1 : 0);
      D->rec_size = size;
      D->valid = 1;
      P.rec_sizes[slot] = (uint64_t)size + 4;
    }
  }
  ov_bases = wave_sum(ov_bases); ov_agree = wave_sum(ov_agree); ov_dis = wave_sum(ov_dis); ov_corr = wave_sum(ov_corr);
  if (lane == 0) {
    atomicAdd(&st[0], (unsigned long long)s_total);
    if (s_cons) atomicAdd(&st[1], (unsigned long long)s_cons);
    if (s_filtered) atomicAdd(&st[2], (unsigned long long)s_filtered);
    if (s_sec) atomicAdd(&st[3 + FGX_REJ_SECONDARY_OR_SUPPLEMENTARY], (unsigned long long)s_sec);
    if (s_insuf) atomicAdd(&st[3 + FGX_REJ_INSUFFICIENT_READS], (unsigned long long)s_insuf);
    if (s_zero) atomicAdd(&st[3 + FGX_REJ_ZERO_LENGTH_AFTER_TRIMMING], (unsigned long long)s_zero);
    if (s_orphan) atomicAdd(&st[3 + FGX_REJ_ORPHAN_CONSENSUS], (unsigned long long)s_orphan);
    if (s_down) atomicAdd(&st[3 + FGX_REJ_DOWNSAMPLED], (unsigned long long)s_down);
    if (s_unm) atomicAdd(&st[3 + FGX_REJ_UNMAPPED], (unsigned long long)s_unm);
    if (ov_bases) atomicAdd(&st[24], (unsigned long long)ov_bases);
    if (ov_agree) atomicAdd(&st[25], (unsigned long long)ov_agree);
    if (ov_dis) atomicAdd(&st[26], (unsigned long long)ov_dis);
    if (ov_corr) atomicAdd(&st[27], (unsigned long long)ov_corr);
  }
  PH(8)
  } else if constexpr (MODE == 1) {
  // =====================================================================================================================
  // MODE 1 — duplex.  Mirrors DuplexConsensusCaller::consensus_reads / process_group (duplex_caller.rs:2545-2624,
  // 1944-2540) for the molecules the device can decide exactly; anything else is deferred to duplex_host.cpp.
  // =====================================================================================================================
  // ---- 5D. fragments out, strand partition, min-reads and collision gates ------------------------------------------------
  const bool paired = act && (flags & bam::F_PAIRED);
  const unsigned long long pmask = __ballot(paired);
  const uint32_t n_frag = n - (uint32_t)__popcll(pmask);
  uint32_t s_cons = 0, s_filtered = n_frag, rj_insuf = 0, rj_coll = 0, rj_zero = 0;
  auto flush_stats = [&]() {
    ov_bases = wave_sum(ov_bases); ov_agree = wave_sum(ov_agree); ov_dis = wave_sum(ov_dis); ov_corr = wave_sum(ov_corr);
    if (lane == 0) {
      atomicAdd(&st[0], (unsigned long long)n);
      if (s_cons) atomicAdd(&st[1], (unsigned long long)s_cons);
      if (s_filtered) atomicAdd(&st[2], (unsigned long long)s_filtered);
      if (n_frag) atomicAdd(&st[3 + FGX_REJ_FRAGMENT_READ], (unsigned long long)n_frag);
      if (rj_insuf) atomicAdd(&st[3 + FGX_REJ_INSUFFICIENT_READS], (unsigned long long)rj_insuf);
      if (rj_coll) atomicAdd(&st[3 + FGX_REJ_POTENTIAL_COLLISION], (unsigned long long)rj_coll);
      if (rj_zero) atomicAdd(&st[3 + FGX_REJ_ZERO_LENGTH_AFTER_TRIMMING], (unsigned long long)rj_zero);
      if (ov_bases) atomicAdd(&st[24], (unsigned long long)ov_bases);
      if (ov_agree) atomicAdd(&st[25], (unsigned long long)ov_agree);
      if (ov_dis) atomicAdd(&st[26], (unsigned long long)ov_dis);
      if (ov_corr) atomicAdd(&st[27], (unsigned long long)ov_corr);
    }
    if constexpr (METH != 0) { const bool any_multi = __any(multi); if (lane == 0 && any_multi) atomicAdd(meth_clipped_counter(P), 1u); }
  };
  if (!pmask) { flush_stats(); return; }                                  // nothing but fragments: no MI to work from
  const bool is_r1 = paired && (flags & bam::F_FIRST), is_r2 = paired && (flags & bam::F_LAST);
  if (__any(paired && is_r1 == is_r2)) { to_defer(); return; }            // FIRST and LAST both set or both clear: general path
  const unsigned long long amask = __ballot(paired && strand == 1), bmask = __ballot(paired && strand == 2);
  const unsigned long long r1m = __ballot(is_r1), r2m = __ballot(is_r2);
  const uint32_t n_ab = (uint32_t)__popcll(amask | bmask);
  auto min_ok = [&](uint32_t x, uint32_t y) {                             // has_minimum_number_of_reads :824-862
    const uint32_t xy = x > y ? x : y, yx = x > y ? y : x;
    return P.dmin_total <= xy + yx && P.dmin_xy <= xy && P.dmin_yx <= yx;
  };
  if (!min_ok((uint32_t)__popcll(amask & r1m), (uint32_t)__popcll(bmask & r1m))) { rj_insuf = n_ab; s_filtered += n_ab; flush_stats(); return; }
  if (amask && bmask) {                                                   // /A R1 with /B R2 (and /A R2 with /B R1) must share a strand
    const unsigned long long revm = __ballot(paired && rev);
    const unsigned long long g1 = (amask & r1m) | (bmask & r2m), g2 = (amask & r2m) | (bmask & r1m);
    const bool same1 = (g1 & revm) == 0 || (g1 & revm) == g1, same2 = (g2 & revm) == 0 || (g2 & revm) == g2;
    if (!same1 || !same2) { rj_coll = n_ab; s_filtered += n_ab; flush_stats(); return; }
  }
  const unsigned long long nzm = __ballot(paired && final_len > 0);
  const uint32_t n_zero = (uint32_t)__popcll((amask | bmask) & ~nzm);     // ZeroLengthAfterTrimming (single-strand caller's stats)
  // the four single-strand read sets: 0 = AB-R1, 1 = AB-R2, 2 = BA-R1, 3 = BA-R2
  unsigned long long em[4];
  em[0] = uniform_u64(amask & r1m & nzm); em[1] = uniform_u64(amask & r2m & nzm); em[2] = uniform_u64(bmask & r1m & nzm); em[3] = uniform_u64(bmask & r2m & nzm);
  // --max-reads-per-strand (consensus_call, vanilla_caller.rs:706-779 with downsample_source_reads :970-980): a set above the cap is SCORED over its `cap`
  // lowest fgbio name ranks — bases, qualities, depths and single-strand errors, and so the consensus length (the longest scoring read) and the coverage
  // rules of 7D —, and the scoring reads enter the column in (rank, file order), not in file order.  Everything the reference computes from `source_reads`
  // keeps the whole set: the duplex error recount (the all-reads counts of 6D) and the consensus UMI (8D works from em[]).  sm[k]: the scoring reads of
  // set k; cap_ord: byte k of lane j holds the record that enters the columns of capped set k j-th.
  unsigned long long sm[4] = {em[0], em[1], em[2], em[3]};
  bool capped[4] = {false, false, false, false};
  bool any_capped = false;
  uint32_t cap_ord = 0;
  uint32_t elen[4], eoff[4];
  {
    bool cap_bites = false;
    uint32_t tot = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (P.dmax_reads >= 0 && (long long)__popcll(em[k]) > P.dmax_reads) cap_bites = true;
      if constexpr (CAP != 0) {
        if (P.dmax_reads > 0 && (long long)__popcll(em[k]) > P.dmax_reads) {
          const bool mine = (em[k] >> lane) & 1;
          const int32_t rk = mine ? name_rank(W + lo + 32, name_len) : 0;
          uint32_t before = 0;
          for (unsigned long long m = em[k]; m; m &= m - 1) {
            const uint32_t j = (uint32_t)__builtin_ctzll(m);
            const int32_t rj = (int32_t)rlane((uint32_t)rk, j);
            before += (rj < rk || (rj == rk && j < lane)) ? 1u : 0u;
          }
          sm[k] = uniform_u64(__ballot(mine && (long long)before < P.dmax_reads));
          // (the positions of a set's reads are a permutation of 0 .. |set| - 1: every step's ballot holds exactly one lane)
          for (uint32_t j = 0; j < (uint32_t)P.dmax_reads; j++) { const uint32_t r = (uint32_t)__builtin_ctzll(__ballot(mine && before == j)); if (lane == j) cap_ord |= r << (8 * k); }
          capped[k] = true; any_capped = true;
        }
      }
      elen[k] = sm[k] ? wave_max(((sm[k] >> lane) & 1) ? final_len : 0) : 0;
      eoff[k] = tot; tot += elen[k];
    }
    // without the CAP build, and with a cap of 0 (no set has a consensus): the general path
    if (cap_bites && (CAP == 0 || P.dmax_reads == 0)) { to_defer(); return; }
  }
  const uint32_t plen1 = (em[0] && em[3]) ? (elen[0] < elen[3] ? elen[0] : elen[3]) : 0;    // R1 duplex: AB-R1 with BA-R2
  const uint32_t plen2 = (em[1] && em[2]) ? (elen[1] < elen[2] ? elen[1] : elen[2]) : 0;    // R2 duplex: AB-R2 with BA-R1

  PH(5)
  // ---- 6D. the four single-strand column sets (ss caller: min_reads 1, min consensus base quality 2) ----------------------
  const uint32_t d0 = seq_lo | (qual_lo << 16), d1 = l_seq | (final_len << 16), d2 = trim_to | ((rev ? 1u : 0u) << 16);
  const DeviceTables* T = P.T;
  const uint64_t col_base = P.col_base[g];
  const uint32_t min_bq = P.min_input_bq;
  CallConst KC;
  KC.cap = (uint32_t)__builtin_amdgcn_readfirstlane((int)sT.cap);
  KC.cap_threshold = uniform_f64(sT.cap_threshold); KC.half_cerr_at_cap = uniform_f64(sT.half_cerr_at_cap);
  uint32_t dm_tr[4] = {0, 0, 0, 0}, dm_fu[4] = {0, 0, 0, 0};     // max depth over the paired (truncated) span / the whole strand
  bool odd_base = false;
  bool ann_set[4] = {false, false, false, false};                // methylation-aware mode: the set's call was annotated
  // A capped set's columns once more, counting only: the observations of EVERY read of the set (the scoring ones included) under the masking rule of the
  // column loops — what the duplex error recount of the record writers works from (duplex_consensus counts over source_reads, which the cap does not touch).
  // The same number of passes in every lane: the cross-lane reads stay in wave-uniform control flow.
  // The methylation-aware mode (METH with CAP) annotates here: annotate_and_normalize runs over the WHOLE set ahead of the cap, so the unconverted / converted
  // counts of a capped set's columns are these reads', and what is counted for the recount is the NORMALISED base (source_reads stays the normalised set);
  // `is_c_of`: the set's ref_is_c, `tc` / `vc`: its unconverted / converted code in consensus orientation.
  auto count_all = [&](unsigned long long all, uint32_t len_k, uint32_t off_k, auto&& is_c_of, uint32_t tc, uint32_t vc) {     // (by value: no dynamically indexed local array)
    for (uint32_t p0 = 0; p0 < len_k; p0 += 64) {
      const uint32_t p = p0 + lane;
      const bool incol = p < len_k;
      uint32_t cnt = 0;
      bool is_c = false;
      uint32_t mu = 0, mt = 0;
      if constexpr (METH != 0) is_c = incol && is_c_of(p);
      for (unsigned long long m = all; m; m &= m - 1) {
        const uint32_t r = (uint32_t)__builtin_ctzll(m);
        const uint32_t x0 = rlane(d0, r), x1 = rlane(d1, r), x2 = rlane(d2, r);
        const bool valid = incol && p < (x1 >> 16);
        const bool rv = (x2 >> 16) != 0;
        const uint32_t idx = valid ? (rv ? (x1 & 0xFFFF) - 1 - p : p) : 0;
        const uint32_t bb = W[(x0 & 0xFFFF) + (idx >> 1)];
        const uint32_t c = (bb >> ((~idx & 1) << 2)) & 15;
        const uint32_t q = W[(x0 >> 16) + idx];
        uint32_t co = rv ? __builtin_bitreverse32(c) >> 28 : c;
        const bool masked = p < (x2 & 0xFFFF) && q < min_bq;
        if constexpr (METH != 0) { if (is_c && valid && !masked) { if (co == tc) mu++; else if (co == vc) { mt++; co = tc; } } }
        if (valid && !masked && __popc(co) == 1) cnt += 1u << (8 * (uint32_t)__builtin_ctz(co));
      }
      if (incol) P.col_obs_all[col_base + off_k + p] = cnt;
      if constexpr (METH != 0) { if (incol) { const uint64_t o = col_base + off_k + p; P.meth_flag[o] = is_c ? 1 : 0; P.meth_u[o] = (uint16_t)mu; P.meth_t[o] = (uint16_t)mt; } }
    }
  };
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const unsigned long long members = sm[k];                      // the scoring reads: the whole set unless the cap bites
    if (!members) continue;
    const uint32_t mc = (uint32_t)__popcll(members);
    const uint32_t plen = (k == 0 || k == 3) ? plen1 : plen2;
    const bool by_rank = CAP != 0 && capped[k];                    // a capped set's reads enter a column in (rank, file order): cap_ord
    // Methylation-aware mode (annotate_and_normalize, vanilla_caller.rs:781-860; methylation.rs:193-242): the call's anchor is the LAST longest
    // source read of the set (max_by_key; file order = lane order), taken over ALL its reads: em[k], not the scoring reads a cap leaves — the anchor of a
    // capped set may be a read the cap drops, and longer than the consensus (the annotation is truncated to it: the columns end at elen[k]).  Every read here
    // is one aligned block, alone or between clips — to the reference ONE M op of T bases, T = the lengths of all its ops, hard clips included —, so column
    // p lies at the anchor's pos + p (forward) or at pos + T - 1 - p (reverse: the columns run in read orientation; with trailing clips that is NOT the
    // last aligned base).  The strand of the call is is_top_strand of the anchor's flags (methylation.rs:392-398): C / T against a reference C, else G / A
    // against a reference G.  No annotation (no tags from this call, nothing normalised) when the anchor names no contig of the genome handed over.
    // The canonical second pass of the mode (FGX_METH_CANON=1; meth_ref_runs) hands over records that no longer lie where they say — `<len>M`, R2 on another
    // reference id — with each record's REFERENCE RUNS (canon_core.h RefRuns: query_to_ref_positions on the original record): then the anchor's contig, strand
    // step and column -> reference position come from its runs, and a column outside every run (an insertion) is no reference cytosine.  The anchor is
    // wave-uniform, so its runs are read through a uniform address in a loop of uniform trip count.
    bool ann = false, a_rev = false;
    long long a_ref0 = 0;
    unsigned long long g_off = 0, g_len = 0;
    RefRunsPtr a_runs = nullptr;                                   // (METH) the anchor's RefRuns as dwords, when the batch carries them
    uint32_t a_nruns = 0;
    uint32_t tcode = 0, vcode = 0, target = 0;                     // unconverted / converted read base as 4-bit codes in consensus orientation; the reference base
    if constexpr (METH != 0) {
      unsigned long long lm = members & __ballot(final_len == elen[k]);
      if constexpr (CAP != 0) { if (by_rank) { const uint32_t alen = wave_max(((em[k] >> lane) & 1) ? final_len : 0); lm = em[k] & __ballot(final_len == alen); } }
      const uint32_t an = 63u - (uint32_t)__clzll((long long)lm);
      const uint32_t a_flags = rlane(flags, an), a_tot = rlane(tot_len, an);   // (T: l_seq of a read of one op; more with hard clips)
      const int32_t a_pos = (int32_t)rlane((uint32_t)pos, an), a_ref = (int32_t)rlane((uint32_t)ref_id, an);
      a_rev = (a_flags & bam::F_REVERSE) != 0;
      const bool a_top = a_rev == ((a_flags & bam::F_LAST) != 0);
      tcode = a_top ? 2u : 4u; vcode = a_top ? 8u : 1u; target = a_top ? (uint32_t)'C' : (uint32_t)'G';
      int32_t a_contig = a_ref;
      bool placed = a_pos >= 0;
      a_runs = meth_ref_runs(P, r0 + an);
      if (a_runs) {
        a_contig = (int32_t)uni(a_runs[0]);                        // the ORIGINAL reference id; -1: the record had no position
        a_nruns = uni(a_runs[1]) & 0xFFu;
        placed = a_contig >= 0;
      }
      ann = a_contig >= 0 && placed && (uint32_t)a_contig < P.n_ref;
      a_ref0 = a_rev ? (long long)a_pos + (long long)a_tot - 1 : (long long)a_pos;
      if (ann) { g_off = uniform_u64(P.contig_off[a_contig]); g_len = uniform_u64(P.contig_len[a_contig]); }
      ann_set[k] = ann;
    }
    auto ref_is_c = [&](uint32_t p) -> bool {                      // the reference shows a cytosine of the call's strand under column p
      if (!ann) return false;
      long long rp = a_rev ? a_ref0 - (long long)p : a_ref0 + (long long)p;
      if (a_runs) {
        rp = -1;
        for (uint32_t r = 0; r < a_nruns; r++) {                   // (uniform trip count; the runs are disjoint)
          const uint32_t q0 = a_runs[2 + 4 * r], rl = a_runs[3 + 4 * r];
          const long long f0 = (long long)(((unsigned long long)a_runs[5 + 4 * r] << 32) | a_runs[4 + 4 * r]);
          const uint32_t d = p - q0;
          if (p >= q0 && d < rl) rp = a_rev ? f0 - (long long)d : f0 + (long long)d;
        }
      }
      if (rp < 0 || (unsigned long long)rp >= g_len) return false;
      uint32_t rb = P.genome[g_off + (unsigned long long)rp];
      if (rb >= 'a' && rb <= 'z') rb -= 32;
      return rb == target;
    };
    // A REGULAR set — every member on one strand (reverse: one read length), untrimmed: the usual set — takes k_simplex_wave2's column
    // step (chain_observe.inc: ~20 vector instructions per observation instead of ~50; the lane's index into a member is the same for
    // every member, a member's final length is a scalar lane mask, the codes stay as stored and the chains' bases are complemented once
    // at the end).  Anything else: the general loop below.  (Final lengths DO differ inside a set: a read that ends in a base below
    // --min-input-base-quality loses it — 44 % of the benchmark's molecules have such a set.)
    bool regular = false;
    uint32_t Lrev = 0;
    bool set_rev = false;
    if (mc > 1) {
      const bool mine = (members >> lane) & 1;
      const unsigned long long rm = members & __ballot(rev);
      set_rev = rm != 0;
      if (rm) Lrev = rlane(l_seq, (uint32_t)__builtin_ctzll(rm));
      const bool oddm = mine && (trim_to != l_seq || (rm != 0 && l_seq != Lrev));
      regular = !__any(oddm) && (rm == 0 || rm == members);
    }
#ifdef FGX_DUPLEX_REQUIRE_REGULAR   /* measurement builds: a molecule with a set that is not regular is deferred — the bench line's deferred count says how many */
    if (mc > 1 && !regular) { to_defer(); return; }
#endif
#ifdef FGX_CAP_GENERAL_LOOP         /* measurement builds: a capped set takes the general loop below, the regular step serves file-order sets only (DESIGN.md 4 has the comparison) */
    if (by_rank) regular = false;
#endif
    if (regular) {
      const uint8_t* const pairs = (const uint8_t*)&sPair[0][0];
      for (uint32_t p0 = 0; p0 < elen[k]; p0 += 64) {
        const uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)p0) + lane;
        const bool incol = p < elen[k];
        const uint32_t ix = incol ? (set_rev ? Lrev - 1 - p : p) : 0u;
        const uint32_t iq = ix, is = ix >> 1, ish = (~ix & 1) << 2;
        double s1 = 0.0, c1 = 0.0, sR = 0.0, cR = 0.0, s2, c2, s3, c3;
        FGX_UNDEF4(s2, c2, s3, c3);   // (chains 2 / 3: written when opened)
        uint32_t allow = incol ? 0x116u : 0u, b1 = 0, b2 = 0, b3 = 0, n1 = 0, n2 = 0, n3 = 0, nR = 0;
        // methylation-aware mode: the codes stay as stored here, so a reverse set's unconverted / converted bases are the complements
        bool is_c = false;
        uint32_t mu = 0, mt = 0, tcs = 0, vcs = 0;
        if constexpr (METH != 0) {
          is_c = incol && ref_is_c(p);
          tcs = set_rev ? __builtin_bitreverse32(tcode) >> 28 : tcode; vcs = set_rev ? __builtin_bitreverse32(vcode) >> 28 : vcode;
        }
        uint32_t nth = 0;
        for (unsigned long long m = members; m;) {
          uint32_t r = (uint32_t)__builtin_ctzll(m);
          m &= m - 1;
#ifndef FGX_CAP_GENERAL_LOOP
          if constexpr (CAP != 0) { if (by_rank) r = (rlane(cap_ord, nth) >> (8 * k)) & 63u; nth++; }
#endif
          const uint32_t x0 = rlane(d0, r), x1 = rlane(d1, r);
          const bool in = __builtin_amdgcn_inverse_ballot_w64(fw_lanes_below(x1 >> 16, (uint32_t)__builtin_amdgcn_readfirstlane((int)p0)));   // inside this member's final length
          const uint32_t q = W[iq + (x0 >> 16)];
          uint32_t c = __builtin_amdgcn_ubfe((uint32_t)W[is + (x0 & 0xFFFF)], ish, 4u);
          if constexpr (METH != 0) {   // counted, and the converted base read as the unconverted one, BEFORE it is observed (a masked base is an N: not counted)
            if (is_c && in && q >= min_bq) { if (c == tcs) mu++; else if (c == vcs) { mt++; c = tcs; } }
          }
          W2_OBSERVE(0, in, q, c, *(const double2*)(pairs + (((q) < 93u ? (q) : 93u) << 4)));
        }
        if (allow != 0) b1 = (uint32_t)__builtin_ctz(allow);
        if (set_rev) { b1 = __builtin_bitreverse32(b1) >> 28; b2 = __builtin_bitreverse32(b2) >> 28; b3 = __builtin_bitreverse32(b3) >> 28; }
        double ll[4];
        uint32_t obs[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
          const uint32_t code = 1u << i;
          ll[i] = code == b1 ? s1 : code == b2 ? s2 : code == b3 ? s3 : sR;
          obs[i] = code == b1 ? n1 : code == b2 ? n2 : code == b3 ? n3 : nR;
        }
        const uint64_t o = col_base + eoff[k] + p;
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
          P.col_obs[o] = obs[0] | (obs[1] << 8) | (obs[2] << 16) | (obs[3] << 24);
          if constexpr (CAP != 0) { if (any_capped && !by_rank) P.col_obs_all[o] = obs[0] | (obs[1] << 8) | (obs[2] << 16) | (obs[3] << 24); }
          if constexpr (METH != 0) { if (!by_rank) { P.meth_flag[o] = is_c ? 1 : 0; P.meth_u[o] = (uint16_t)mu; P.meth_t[o] = (uint16_t)mt; } }   // (a capped set: count_all's, over every read)
          dm_fu[k] = depth > dm_fu[k] ? depth : dm_fu[k];
          if (p < plen) dm_tr[k] = depth > dm_tr[k] ? depth : dm_tr[k];
        }
      }
      if constexpr (CAP != 0) { if (by_rank) count_all(em[k], elen[k], eoff[k], ref_is_c, tcode, vcode); }
      continue;
    }
    // (a single-read set: the read's fields once, by every lane, ahead of the column loop — its trip count differs from lane to lane)
    uint32_t one_seq = 0, one_qual = 0, one_lseq = 0, one_flags = 0, one_trim = 0;
    if (mc == 1) {
      const uint32_t r = (uint32_t)__builtin_ctzll(members);
      one_seq = rlane(seq_lo, r); one_qual = rlane(qual_lo, r); one_lseq = rlane(l_seq, r); one_flags = rlane(flags, r); one_trim = rlane(trim_to, r);
    }
    for (uint32_t p = lane; p < elen[k]; p += 64) {
      const uint64_t o = col_base + eoff[k] + p;
      uint32_t depth, obs[4];
      bool is_c = false;
      uint32_t mu = 0, mt = 0;
      if constexpr (METH != 0) is_c = ref_is_c(p);
      if (mc == 1) {   // single-read consensus: LUT keyed by the unclamped quality (vanilla_caller.rs:1677-1708)
        uint32_t code, q;
        view(one_seq, one_qual, one_lseq, (one_flags & bam::F_REVERSE) != 0, one_trim, p, &code, &q);
        if constexpr (METH != 0) { if (is_c) { if (code == tcode) mu = 1; else if (code == vcode) { mt = 1; code = tcode; } } }   // (`view` gives the masked base as N)
        const uint8_t adj = q < 94 ? T->single_input_quals[q] : 0;
        const bool low = adj < FGX_MIN_PHRED;
        P.col_code[o] = low ? (uint8_t)15 : (uint8_t)code; P.col_qual[o] = low ? (uint8_t)FGX_MIN_PHRED : adj; P.col_err[o] = 0;
        obs[0] = code == 1; obs[1] = code == 2; obs[2] = code == 4; obs[3] = code == 8;
        depth = code != 15 ? 1u : 0u;
        if (depth && !(obs[0] | obs[1] | obs[2] | obs[3])) odd_base = true;     // IUPAC code in a lone read: general path
      } else {
        ChainAcc acc;                           // two Kahan chains while the column shows one base (consensus_math.h)
        acc.reset();
        uint32_t nth = 0;
        for (unsigned long long m = members; m; m &= m - 1) {
          uint32_t r = (uint32_t)__builtin_ctzll(m);
          if constexpr (CAP != 0) { if (by_rank) r = (rlane(cap_ord, nth) >> (8 * k)) & 63u; nth++; }
          const uint32_t x0 = rlane(d0, r), x1 = rlane(d1, r), x2 = rlane(d2, r);
          bool valid = p < (x1 >> 16);
          const bool rv = (x2 >> 16) != 0;
          const uint32_t idx = valid ? (rv ? (x1 & 0xFFFF) - 1 - p : p) : 0;
          const uint32_t bb = W[(x0 & 0xFFFF) + (idx >> 1)];
          const uint32_t c = (bb >> ((~idx & 1) << 2)) & 15;
          const uint32_t q = W[(x0 >> 16) + idx];
          uint32_t co = rv ? __builtin_bitreverse32(c) >> 28 : c;           // read orientation: complement = bit reversal of the code
          const bool masked = p < (x2 & 0xFFFF) && q < min_bq;
          if constexpr (METH != 0) { if (is_c && valid && !masked) { if (co == tcode) mu++; else if (co == vcode) { mt++; co = tcode; } } }
          valid = valid && __popc(co) == 1 && !masked;                      // only the one-hot codes A C G T are observations
          const uint32_t qq = q < FGX_MAX_PHRED ? q : FGX_MAX_PHRED;
          const double2 pr = *(const double2*)&sPair[qq][0];
          acc.add(valid, co, pr.x, pr.y);
        }
        double ll[4];
        acc.finish(ll, obs);
        int bi;
        uint8_t q;
        const bool resolved = column_call_fast_lds(sT, KC, ll, obs, &bi, &q);
        depth = obs[0] + obs[1] + obs[2] + obs[3];
        push_full(!resolved, o, ll, obs);
        if (resolved) {
          const uint32_t err = depth - (bi == 0 ? obs[0] : bi == 1 ? obs[1] : bi == 2 ? obs[2] : bi == 3 ? obs[3] : 0u);
          uint8_t ob, oq;
          if (depth < 1) { ob = 15; oq = 0; }
          else if (q < FGX_MIN_PHRED) { ob = 15; oq = FGX_MIN_PHRED; }
          else { ob = bi >= 0 ? (uint8_t)(1u << bi) : (uint8_t)15; oq = q; }
          P.col_code[o] = ob; P.col_qual[o] = oq; P.col_err[o] = (uint16_t)err;
        }
      }
      P.col_obs[o] = obs[0] | (obs[1] << 8) | (obs[2] << 16) | (obs[3] << 24);
      if constexpr (CAP != 0) { if (any_capped && !by_rank) P.col_obs_all[o] = obs[0] | (obs[1] << 8) | (obs[2] << 16) | (obs[3] << 24); }
      if constexpr (METH != 0) { if (!by_rank) { P.meth_flag[o] = is_c ? 1 : 0; P.meth_u[o] = (uint16_t)mu; P.meth_t[o] = (uint16_t)mt; } }
      dm_fu[k] = depth > dm_fu[k] ? depth : dm_fu[k];
      if (p < plen) dm_tr[k] = depth > dm_tr[k] ? depth : dm_tr[k];
    }
    if constexpr (CAP != 0) { if (by_rank) count_all(em[k], elen[k], eoff[k], ref_is_c, tcode, vcode); }
  }
  if (__any(odd_base)) { to_defer(); return; }
#pragma unroll
  for (int k = 0; k < 4; k++) { dm_fu[k] = wave_max(dm_fu[k]); dm_tr[k] = wave_max(dm_tr[k]); }

  PH(6)
  // ---- 7D. which records come out (duplex_consensus :931-1108, process_group :2400-2540) ------------------------------------
  // A duplex record takes strand `sa` (and `sb` when both strands are covered); a strand alone is passed through.
  struct Out { bool ok; bool has_ba; uint32_t sa, sb, len; };
  auto duplex_of = [&](int ka, int kb, uint32_t plen) {          // ka: AB-side set or -1, kb: BA-side set or -1
    Out r; r.ok = false; r.has_ba = false; r.sa = 0; r.sb = 0; r.len = 0;
    const bool have_a = ka >= 0, have_b = kb >= 0;
    const uint32_t da = have_a ? (have_b ? dm_tr[ka < 0 ? 0 : ka] : dm_fu[ka < 0 ? 0 : ka]) : 0;
    const uint32_t db = have_b ? (have_a ? dm_tr[kb < 0 ? 0 : kb] : dm_fu[kb < 0 ? 0 : kb]) : 0;
    const bool cov_a = have_a && da > 0, cov_b = have_b && db > 0;
    if (!cov_a && !cov_b) return r;
    if (cov_a && cov_b) { r.ok = min_ok(da, db); r.has_ba = true; r.sa = (uint32_t)ka; r.sb = (uint32_t)kb; r.len = plen; return r; }
    const int ks = cov_a ? ka : kb;                                 // one covered strand: copied whole, depth over its full length
    const uint32_t ds = dm_fu[ks < 0 ? 0 : ks];
    r.ok = min_ok(ds, 0); r.sa = (uint32_t)ks; r.sb = (uint32_t)ks; r.len = elen[ks < 0 ? 0 : ks];
    return r;
  };
  const bool h1 = em[0] != 0, h2 = em[1] != 0, h3 = em[2] != 0, h4 = em[3] != 0;
  Out o1, o2;
  o1.ok = o2.ok = false; o1.has_ba = o2.has_ba = false; o1.sa = o1.sb = o2.sa = o2.sb = 0; o1.len = o2.len = 0;
  if (h1 && h2 && h3 && h4) { o1 = duplex_of(0, 3, plen1); o2 = duplex_of(1, 2, plen2); }
  else if (h1 && h2 && !h3 && !h4) { if (P.dmin_yx == 0) { o1 = duplex_of(0, -1, 0); o2 = duplex_of(1, -1, 0); } }
  else if (!h1 && !h2 && h3 && h4) { if (P.dmin_yx == 0) { o1 = duplex_of(-1, 2, 0); o2 = duplex_of(-1, 3, 0); } }
  const bool emitted = o1.ok && o2.ok;
  // statistics (duplex_caller.rs:2587-2610 with the re-attribution of :1894-1926)
  if (emitted) { s_cons = 2; rj_zero = n_zero; s_filtered += n_zero; }
  else { rj_insuf = n_ab - n_zero; rj_zero = n_zero; s_filtered += n_ab; }

  // ---- 8D. consensus UMI and descriptor of each record ----------------------------------------------------------------------
  if (emitted) {
    const DeviceTables* TU = P.TU;
    const unsigned long long rxm = rxmask;
    // '-' structure of this lane's RX (flipping a paired UMI swaps the halves around the single dash)
    uint32_t n_dash = 0, dash_pos = 0;
    if (act && has_rx) for (uint32_t i = 0; i < rx_len; i++) if (W[rx_lo + i] == '-') { if (!n_dash) dash_pos = i; n_dash++; }
    const uint32_t fp = (uint32_t)__builtin_ctzll(pmask);                     // first paired record: MI → name and MI tag
    const uint32_t fp_mi_lo = rlane(mi_lo, fp), fp_mi_len = rlane(mi_len, fp) - 2, fp_lo = rlane(lo, fp);
    const uint32_t fc = amask ? (uint32_t)__builtin_ctzll(amask) : (uint32_t)__builtin_ctzll(bmask);   // cell barcode source
    const bool fc_has_cb = P.cell0 && ((cbmask >> fc) & 1);
    const uint32_t fc_cb_lo = rlane(cb_lo, fc), fc_cb_len = rlane(cb_len, fc), fc_lo = rlane(lo, fc);
    bool rx_fail = false;
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const Out& O = t == 0 ? o1 : o2;
      // source reads of this record's UMIs, A-side first (file order inside a side); a read is flipped when its FIRST flag
      // differs from the record's (duplex_read_into :1336-1368)
      unsigned long long sa_m = 0, sb_m = 0;
      if (h1 && h2 && h3 && h4) { sa_m = t == 0 ? em[0] : em[1]; sb_m = t == 0 ? em[3] : em[2]; }
      else if (h1) { sa_m = t == 0 ? em[0] : em[1]; }
      else { sb_m = t == 0 ? em[2] : em[3]; }
      sa_m &= rxm; sb_m &= rxm;
      const bool rec_first = t == 0;
      const uint32_t cnt = (uint32_t)__popcll(sa_m | sb_m);
      uint32_t ulen = 0;
      char my_ch = 0;
      if (cnt) {
        const uint32_t f = sa_m ? (uint32_t)__builtin_ctzll(sa_m) : (uint32_t)__builtin_ctzll(sb_m);
        ulen = rlane(rx_len, f);
        const bool in_set = ((sa_m | sb_m) >> lane) & 1;
        const bool flip_me = in_set && (((flags & bam::F_FIRST) != 0) != rec_first);
        if (__any(in_set && rx_len != ulen) || ulen > FAST_RX_CAP || __any(flip_me && n_dash > 1)) rx_fail = true;
        else {
          // character j of read r's UMI as it enters the consensus
          auto chr = [&](uint32_t r, uint32_t j) -> uint8_t {
            const uint32_t rlo = rlane(rx_lo, r), nd = rlane(n_dash, r), dp = rlane(dash_pos, r);
            const bool fl = (((rlane(flags, r) & bam::F_FIRST) != 0) != rec_first) && nd == 1;
            uint32_t src = j;
            if (fl) { const uint32_t ql = ulen - dp - 1; src = j < ql ? dp + 1 + j : j == ql ? dp : j - ql - 1; }
            return j < ulen ? W[rlo + src] : (uint8_t)'A';
          };
          const bool mychar = lane < ulen;
          const uint8_t c0 = chr(f, lane);
          bool differs = false;
          for (unsigned long long m = sa_m | sb_m; m; m &= m - 1) differs |= chr((uint32_t)__builtin_ctzll(m), lane) != c0;
          if (cnt == 1 || !__any(mychar && differs)) {
            const int bl = bam::ascii_to_lane(c0);
            my_ch = cnt == 1 ? (char)c0 : bl != 255 ? "ACGT"[bl] : (c0 == 'N' || c0 == 'n') ? 'N' : (char)c0;
          } else {
            ColumnAcc acc;
            acc.reset();
            uint32_t non_dna = 0, seen = 0;
            uint8_t fch = 0;
            bool mixed = false;
            const double uc = TU->t.correct[20], ue = TU->t.error_per_alt[20];
#pragma unroll
            for (int side = 0; side < 2; side++)
              for (unsigned long long m = side == 0 ? sa_m : sb_m; m; m &= m - 1) {
                const uint8_t ch = chr((uint32_t)__builtin_ctzll(m), lane);
                if (seen == 0) fch = ch;
                seen++;
                const uint8_t up = (ch >= 'a' && ch <= 'z') ? (uint8_t)(ch - 32) : ch;
                const bool dna = up == 'A' || up == 'C' || up == 'G' || up == 'T' || up == 'N';
                if (dna) { const int bl = bam::ascii_to_lane(ch); if (bl != 255) acc.add(bl, uc, ue); }
                else { non_dna++; if (ch != fch) mixed = true; }
              }
            bool need_full = false, bad_col = false;
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
            push_full(need_full, (1ull << 63) | ((uint64_t)(slot0 + 1 + t) << 8) | lane, acc.s, acc.obs);
          }
        }
      }
      const uint32_t slot = slot0 + 1 + t;
      DuplexDesc* D = &P.dends[slot];
      if (lane < ulen && cnt) D->rx[lane] = my_ch;
      if (lane == 0) {
        const uint32_t L = O.len;
        D->a_off = col_base + eoff[O.sa]; D->b_off = col_base + eoff[O.sb];
        D->len = L; D->first_rec = r0 + fp; D->cb_rec = r0 + fc;
        D->mi_off = (uint16_t)(fp_mi_lo - fp_lo); D->mi_len = (uint8_t)fp_mi_len;
        D->has_cb = fc_has_cb ? 1 : 0; D->cb_off = (uint16_t)(fc_cb_lo - fc_lo); D->cb_len = (uint8_t)fc_cb_len;
        D->has_rx = cnt > 0; D->rx_len = (uint8_t)ulen; D->type = (uint8_t)(1 + t); D->has_ba = O.has_ba ? 1 : 0;
        if constexpr (CAP != 0) D->capped = any_capped ? 1 : 0;
        if constexpr (METH != 0) {   // which strands carry an annotation; a lone strand passed through keeps the BA side's tag names (duplex_caller.rs:1338-1398)
          auto ann_of = [&](uint32_t kk) { return kk == 0 ? ann_set[0] : kk == 1 ? ann_set[1] : kk == 2 ? ann_set[2] : ann_set[3]; };
          D->meth = (uint8_t)((ann_of(O.sa) ? 1u : 0u) | ((O.has_ba && ann_of(O.sb)) ? 2u : 0u) | ((!O.has_ba && O.sa >= 2) ? 4u : 0u));
        }
        const uint32_t nm = P.prefix_len + 1 + fp_mi_len;
        const uint32_t per_strand = P.per_base_tags ? 2 * (3 + L + 1) + 2 * (8 + 2 * L) : 0;     // ac/aq strings + ad/ae arrays
        // every int tag holds a depth <= 128 here (<= 64 records per wavefront): 4 bytes each
        const uint32_t size = 32 + nm + 1 + (L + 1) / 2 + L + (3 + fp_mi_len + 1) + (fc_has_cb ? 3 + fc_cb_len + 1 : 0) + (3 + P.rg_len + 1) +
                              3 * (4 + 7 + 4) + per_strand + (O.has_ba ? per_strand : 0) + (cnt ? 3 + ulen + 1 : 0);
        D->rec_size = size;
        D->valid = 1;
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
  PH(8)
  } else {
  // =====================================================================================================================
  // MODE 2 — CODEC.  Mirrors CodecConsensusCaller::consensus_reads_raw (codec_caller.rs:625-1004) for molecules whose
  // records are all paired primary reads with a single M op, mates adjacent; everything else goes to codec_host.cpp.
  // The duplex-disagreement thresholds are at their defaults on this path (the host checks), so no molecule is rejected
  // after the strand combine and every record size is known here.
  // =====================================================================================================================
  // ---- 5C. templates: the partner of each record is the one other record with its read name ---------------------------------
  uint32_t s_filtered = 0, rj_notfr = 0, rj_insuf = 0, rj_overlap = 0, rj_indel = 0, rj_clipfail = 0, rj_down = 0, s_cons = 0;
  auto flush_stats = [&]() {
    if (lane == 0) {
      atomicAdd(&st[0], (unsigned long long)n);
      if (s_cons) atomicAdd(&st[1], (unsigned long long)s_cons);
      if (s_filtered) atomicAdd(&st[2], (unsigned long long)s_filtered);
      if (rj_notfr) atomicAdd(&st[3 + FGX_REJ_NOT_PRIMARY_FR_PAIR], (unsigned long long)rj_notfr);
      if (rj_insuf) atomicAdd(&st[3 + FGX_REJ_INSUFFICIENT_READS], (unsigned long long)rj_insuf);
      if (rj_overlap) atomicAdd(&st[3 + FGX_REJ_INSUFFICIENT_OVERLAP], (unsigned long long)rj_overlap);
      if (rj_indel) atomicAdd(&st[3 + FGX_REJ_INDEL_ERROR_BETWEEN_STRANDS], (unsigned long long)rj_indel);
      if (rj_clipfail) atomicAdd(&st[3 + FGX_REJ_CLIP_OVERLAP_FAILED], (unsigned long long)rj_clipfail);
      if (rj_down) atomicAdd(&st[3 + FGX_REJ_DOWNSAMPLED], (unsigned long long)rj_down);
    }
  };
  {
    uint32_t eq_lo = 0, eq_hi = 0;
    for (unsigned long long um = __ballot(act); um; um &= um - 1) {
      const uint32_t u = (uint32_t)__builtin_ctzll(um);
      const uint32_t hash_u = rlane(hash, u), nlen_u = rlane(name_len, u);      // (both cross-lane reads by every lane: no short circuit between them)
      const bool eq = hash_u == hash && nlen_u == name_len && u != lane;
      if (u < 32) eq_lo |= (eq ? 1u : 0u) << u; else eq_hi |= (eq ? 1u : 0u) << (u - 32);
    }
    unsigned long long todo = act ? ((unsigned long long)eq_lo | ((unsigned long long)eq_hi << 32)) : 0ull;
    uint32_t n_same = 0;
    bool neighbour = false;
    while (__any(todo != 0)) {
      const bool mine = todo != 0;
      const uint32_t u = mine ? (uint32_t)__builtin_ctzll(todo) : lane;
      todo &= todo - 1;
      const uint32_t lou = (uint32_t)__shfl((int)lo, (int)u);
      if (mine) {
        bool same = true;
        for (uint32_t i = 0; i < name_len; i += 8) {
          unsigned long long wa = ld64u(W, lou + 32 + i), wb = ld64u(W, lo + 32 + i);
          if (i + 8 > name_len) { unsigned long long mk = (1ULL << (8 * (name_len - i))) - 1; wa &= mk; wb &= mk; }
          if (wa != wb) { same = false; break; }
        }
        if (same) { n_same++; neighbour |= u == (lane ^ 1); }
      }
    }
    // exactly two records per name, mates adjacent (template order by first appearance is then the order of the R1s and of
    // the R2s — the order the likelihoods are summed in); singletons, triples, interleaved pairs: general path
    if (__any(act && (n_same != 1 || !neighbour))) { to_defer(); return; }
  }
  const bool first = (flags & bam::F_FIRST) != 0;
  const uint32_t m_flags = (uint32_t)__shfl((int)flags, (int)(lane ^ 1)), m_lseq = (uint32_t)__shfl((int)l_seq, (int)(lane ^ 1));
  const int32_t m_pos = (int32_t)__shfl((int)pos, (int)(lane ^ 1)), m_ref = (int32_t)__shfl((int)ref_id, (int)(lane ^ 1));
  const uint32_t m_frself = (uint32_t)__shfl((int)strand, (int)(lane ^ 1));
  if (__any(act && first == ((m_flags & bam::F_FIRST) != 0))) { to_defer(); return; }          // both mates FIRST or neither
  // is_primary_fr_pair_raw (overlap.rs:83-108): mapped, mates mapped, one reference, opposite strands, FR by the reverse record
  const bool m_rev = (m_flags & bam::F_REVERSE) != 0;
  const bool fr = act && !(flags & bam::F_MATE_UNMAPPED) && !(m_flags & bam::F_MATE_UNMAPPED) && ref_id == m_ref && rev != m_rev &&
                  (rev ? strand : m_frself) != 0;
  const uint32_t n_notfr = (uint32_t)__popcll(__ballot(act && !fr));
  rj_notfr = n_notfr; s_filtered += n_notfr;
  // overlap clip against the mate in hand (overlap.rs:223-357 for two single-M alignments)
  if (fr) {
    // (the parse refused pos outside [0, 2^30) and l_seq outside 1 .. 65 535 for this record and for its mate: the closed form's ranges)
    clip = record::single_m_overlap_clip(rev, pos, (int32_t)l_seq, m_pos, (int32_t)m_lseq);
  }
  // ClippedRecordInfo (:1006-1040): hard clip at the 3' end; a reverse read loses its start and moves right
  const uint32_t clen = fr ? (l_seq > clip ? l_seq - clip : 0) : 0;                 // clipped_seq_len = reference span of the clipped M
  const unsigned long long adj = (unsigned long long)((long long)pos + 1) + (rev ? (clip < l_seq ? clip : l_seq) : 0);
  unsigned long long r1set = uniform_u64(__ballot(fr && first)), r2set = uniform_u64(__ballot(fr && !first));
  uint32_t n_strand = (uint32_t)__popcll(r1set | r2set);
  if (!r1set) { flush_stats(); return; }
  auto reject_all = [&](uint32_t& counter) { counter += n_strand; s_filtered += n_strand; flush_stats(); };
  if ((uint32_t)__popcll(r1set) < P.cmin_reads) { reject_all(rj_insuf); return; }
  // most common alignment: with one M op per read the simplified clipped CIGAR is (M, l_seq) — equal read lengths ⇒ one group
  {
    const uint32_t l1ref = rlane(l_seq, (uint32_t)__builtin_ctzll(r1set)), l2ref = rlane(l_seq, (uint32_t)__builtin_ctzll(r2set));
    if (__any(fr && l_seq != (first ? l1ref : l2ref))) { to_defer(); return; }
  }
  // --max-reads-per-strand (codec_caller.rs:765-802, cap_infos_to_lowest_ranking :1060-1072): after the alignment filter and the min-reads check, the
  // R1 list and the R2 list each keep their `cap` lowest fgbio name ranks (ties in file order; the lists need not keep the same templates), the
  // survivors stay in file order, and what is dropped is counted as Downsampled — never routed to --rejects.  Everything below sees the survivors only.
  if (P.cmax_reads >= 0) {
    if (P.cmax_reads == 0) { reject_all(rj_insuf); return; }
    if constexpr (CAP != 0) if ((long long)__popcll(r1set) > P.cmax_reads || (long long)__popcll(r2set) > P.cmax_reads) {
      const int32_t rk = fr ? name_rank(W + lo + 32, name_len) : 0;
      const unsigned long long mine = first ? r1set : r2set;                   // the list this lane's record is in
      uint32_t before = 0;
      for (unsigned long long m = r1set | r2set; m; m &= m - 1) {
        const uint32_t j = (uint32_t)__builtin_ctzll(m);
        const int32_t rj = (int32_t)rlane((uint32_t)rk, j);
        before += (((mine >> j) & 1) && (rj < rk || (rj == rk && j < lane))) ? 1u : 0u;
      }
      const unsigned long long stay = uniform_u64(__ballot(fr && (long long)before < P.cmax_reads));
      rj_down = n_strand - (uint32_t)__popcll(stay);
      s_filtered += rj_down;
      r1set &= stay; r2set &= stay; n_strand = (uint32_t)__popcll(stay);
    }
    // (the build without the cap never sees one — the launch pairs a cap with CAP 1 —; if it ever does, the general path decides the molecule)
    if constexpr (CAP == 0) if ((long long)__popcll(r1set) > P.cmax_reads || (long long)__popcll(r2set) > P.cmax_reads) { to_defer(); return; }
  }
  // this lane's record is a surviving R1 / R2 (CAP 0, the build of a caller without a cap: the FR records as they are)
  const bool fr1 = CAP != 0 ? (bool)((r1set >> lane) & 1) : (fr && first), fr2 = CAP != 0 ? (bool)((r2set >> lane) & 1) : (fr && !first);
  // longest R1 / R2 by clipped reference length (first maximum)
  const uint32_t mx1 = wave_max(fr1 ? clen + 1 : 0), mx2 = wave_max(fr2 ? clen + 1 : 0);
  const uint32_t L1 = (uint32_t)__builtin_ctzll(__ballot(fr1 && clen + 1 == mx1)), L2 = (uint32_t)__builtin_ctzll(__ballot(fr2 && clen + 1 == mx2));
  const bool r1_neg = (rlane(flags, L1) & bam::F_REVERSE) != 0, r2_neg = (rlane(flags, L2) & bam::F_REVERSE) != 0;
  const uint32_t adj_lo = (uint32_t)adj, adj_hi = (uint32_t)(adj >> 32);
  auto adj_of = [&](uint32_t r) { return ((unsigned long long)rlane(adj_hi, r) << 32) | rlane(adj_lo, r); };
  const uint32_t Lp = r1_neg ? L2 : L1, Ln = r1_neg ? L1 : L2;
  const unsigned long long adj_p = adj_of(Lp), adj_n = adj_of(Ln), adj_1 = adj_of(L1), adj_2 = adj_of(L2);
  const uint32_t rl_p = rlane(clen, Lp), rl_n = rlane(clen, Ln), rl_1 = rlane(clen, L1), rl_2 = rlane(clen, L2);
  const unsigned long long pos_end = adj_p + (rl_p ? rl_p - 1 : 0), neg_end = adj_n + (rl_n ? rl_n - 1 : 0);
  const unsigned long long ov_s = adj_n > adj_p ? adj_n : adj_p, ov_e = pos_end < neg_end ? pos_end : neg_end;
  const long long duplex_len = (long long)ov_e - (long long)ov_s + 1;
  if (duplex_len < (long long)P.cmin_duplex_len) { reject_all(rj_overlap); return; }
  // read_pos_at_ref_pos_raw (cigar.rs:461-500) on [H?] M [H?]: 1-based query position, 0 = htsjdk's out-of-range sentinel
  auto read_pos = [](unsigned long long a, uint32_t rl, unsigned long long p) -> long long { return (p >= a && rl && p <= a + rl - 1) ? (long long)(p - a + 1) : 0; };
  if (read_pos(adj_1, rl_1, ov_s) - read_pos(adj_2, rl_2, ov_s) != read_pos(adj_1, rl_1, ov_e) - read_pos(adj_2, rl_2, ov_e)) { reject_all(rj_indel); return; }
  const long long prp = read_pos(adj_p, rl_p, ov_e), nrp = read_pos(adj_n, rl_n, ov_e);
  if (prp == 0 || nrp == 0) { reject_all(rj_indel); return; }
  if (prp + (long long)rl_n < nrp) { to_defer(); return; }                       // the general path raises the error
  const uint32_t cons_len = (uint32_t)(prp + (long long)rl_n - nrp);
  const uint32_t len1 = wave_max(fr1 ? clen : 0), len2 = wave_max(fr2 ? clen : 0);
  if (cons_len < len1 || cons_len < len2) { reject_all(rj_clipfail); return; }

  PH(5)
  // ---- 6C. the two single-strand column sets (ss caller: min_reads 1, no quality masking, min consensus base quality 0) ----------
  final_len = clen;
  const uint32_t d0 = seq_lo | (qual_lo << 16), d1 = l_seq | (final_len << 16), d2 = (rev ? 1u : 0u) << 16;
  const DeviceTables* T = P.T;
  const uint64_t col_base = P.col_base[g];
  CallConst KC;
  KC.cap = (uint32_t)__builtin_amdgcn_readfirstlane((int)sT.cap);
  KC.cap_threshold = uniform_f64(sT.cap_threshold); KC.half_cerr_at_cap = uniform_f64(sT.half_cerr_at_cap);
  bool odd_base = false;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const unsigned long long members = k == 0 ? r1set : r2set;
    const uint32_t mc = (uint32_t)__popcll(members), elen = k == 0 ? len1 : len2, eoff = k == 0 ? 0 : len1;
    // (the column loop runs the SAME number of passes in every lane — a lane past the end of the set takes part in the cross-lane reads of a pass and
    // stores nothing —, and a single-read set reads its read's fields once ahead of it: cross-lane operations stay in wave-uniform control flow, which
    // tests/wavemu checks)
    uint32_t one_seq = 0, one_qual = 0, one_lseq = 0, one_flags = 0;
    if (mc == 1) {
      const uint32_t r = (uint32_t)__builtin_ctzll(members);
      one_seq = rlane(seq_lo, r); one_qual = rlane(qual_lo, r); one_lseq = rlane(l_seq, r); one_flags = rlane(flags, r);
    }
    for (uint32_t p0 = 0; p0 < elen; p0 += 64) {
      const uint32_t p = p0 + lane;
      const bool incol = p < elen;
      const uint64_t o = col_base + eoff + p;
      if (mc == 1) {   // single-read consensus: LUT keyed by the unclamped quality (vanilla_caller.rs:1677-1708)
        if (incol) {
          uint32_t code, q;
          view(one_seq, one_qual, one_lseq, (one_flags & bam::F_REVERSE) != 0, 0, p, &code, &q);
          const uint8_t adjq = q < 94 ? T->single_input_quals[q] : 0;
          P.col_code[o] = (uint8_t)code; P.col_qual[o] = adjq; P.col_depth[o] = code != 15 ? 1 : 0; P.col_err[o] = 0;
          if (code != 15 && code != 1 && code != 2 && code != 4 && code != 8) odd_base = true;   // IUPAC code in a lone read: general path
        }
      } else {
        ChainAcc acc;                           // two Kahan chains while the column shows one base (consensus_math.h)
        acc.reset();
        for (unsigned long long m = members; m; m &= m - 1) {
          const uint32_t r = (uint32_t)__builtin_ctzll(m);
          const uint32_t x0 = rlane(d0, r), x1 = rlane(d1, r), x2 = rlane(d2, r);
          bool valid = incol && p < (x1 >> 16);
          const bool rv = (x2 >> 16) != 0;
          const uint32_t idx = valid ? (rv ? (x1 & 0xFFFF) - 1 - p : p) : 0;
          const uint32_t bb = W[(x0 & 0xFFFF) + (idx >> 1)];
          const uint32_t c = (bb >> ((~idx & 1) << 2)) & 15;
          const uint32_t q = W[(x0 >> 16) + idx];
          const uint32_t co = rv ? __builtin_bitreverse32(c) >> 28 : c;     // read orientation: complement = bit reversal of the code
          valid = valid && __popc(co) == 1;                                 // only the one-hot codes A C G T are observations
          const uint32_t qq = q < FGX_MAX_PHRED ? q : FGX_MAX_PHRED;
          const double2 pr = *(const double2*)&sPair[qq][0];
          acc.add(valid, co, pr.x, pr.y);
        }
        double ll[4];
        uint32_t obs[4];
        acc.finish(ll, obs);
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

  PH(6)
  // ---- 7C. consensus UMI over EVERY record of the group that carries RX (codec_caller.rs:1725-1744) -----------------------------
  const DeviceTables* TU = P.TU;
  const unsigned long long with = rxmask;
  const uint32_t rx_cnt = (uint32_t)__popcll(with);
  uint32_t ulen = 0;
  char my_ch = 0;
  bool rx_fail = false;
  const uint32_t slot = slot0 + 1;
  if (rx_cnt) {
    const uint32_t f = (uint32_t)__builtin_ctzll(with);
    ulen = rlane(rx_len, f);
    if (__any(((with >> lane) & 1) && rx_len != ulen) || ulen > FAST_RX_CAP) rx_fail = true;
    else {
      const bool mychar = lane < ulen;
      const uint32_t f_lo = rlane(rx_lo, f);
      const uint8_t c0 = mychar ? W[f_lo + lane] : (uint8_t)'A';
      bool differs = false;
      if ((with >> lane) & 1) {
        for (uint32_t i = 0; i < ulen; i += 8) {
          unsigned long long a = ld64u(W, rx_lo + i), b = ld64u(W, f_lo + i);
          if (i + 8 > ulen) { unsigned long long mk = (1ULL << (8 * (ulen - i))) - 1; a &= mk; b &= mk; }
          differs |= a != b;
        }
      }
      if (rx_cnt == 1 || !__any(differs)) {
        const int bl = bam::ascii_to_lane(c0);
        my_ch = rx_cnt == 1 ? (char)c0 : bl != 255 ? "ACGT"[bl] : (c0 == 'N' || c0 == 'n') ? 'N' : (char)c0;
      } else {
        ColumnAcc acc;
        acc.reset();
        uint32_t non_dna = 0, seen = 0;
        uint8_t fch = 0;
        bool mixed = false;
        const double uc = TU->t.correct[20], ue = TU->t.error_per_alt[20];
        for (unsigned long long m = with; m; m &= m - 1) {
          const uint32_t r = (uint32_t)__builtin_ctzll(m);
          const uint8_t ch = mychar ? W[rlane(rx_lo, r) + lane] : (uint8_t)'A';
          if (seen == 0) fch = ch;
          seen++;
          const uint8_t up = (ch >= 'a' && ch <= 'z') ? (uint8_t)(ch - 32) : ch;
          const bool dna = up == 'A' || up == 'C' || up == 'G' || up == 'T' || up == 'N';
          if (dna) { const int bl = bam::ascii_to_lane(ch); if (bl != 255) acc.add(bl, uc, ue); }
          else { non_dna++; if (ch != fch) mixed = true; }
        }
        bool need_full = false, bad_col = false;
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
        push_full(need_full, (1ull << 63) | ((uint64_t)slot << 8) | lane, acc.s, acc.obs);
      }
    }
  }
  if (rx_fail || __any(list_overflow)) { to_defer(); return; }

  // ---- 8C. descriptor ------------------------------------------------------------------------------------------------------------
  {
    CodecDesc* D = &P.cends[slot];
    bool rx_empty = true;                                    // an all-empty consensus UMI is not written (:1740-1743)
    if (rx_cnt && ulen) rx_empty = false;
    if (lane < ulen && rx_cnt) D->rx[lane] = my_ch;
    // cell barcode: first record, R1s then R2s, that carries a non-empty value (:1708-1722)
    const unsigned long long cbm = __ballot(act && has_cb && cb_len > 0);
    const unsigned long long c1 = cbm & r1set, c2 = cbm & r2set;
    const bool any_cb = P.cell0 && (c1 | c2);
    const uint32_t fc = c1 ? (uint32_t)__builtin_ctzll(c1) : c2 ? (uint32_t)__builtin_ctzll(c2) : 0;
    const uint32_t fc_cb_lo = rlane(cb_lo, fc), fc_cb_len = rlane(cb_len, fc), fc_lo = rlane(lo, fc);
    if (lane == 0) {
      const uint32_t C = cons_len;
      D->s1_off = col_base; D->s2_off = col_base + len1; D->l1 = len1; D->l2 = len2; D->cons_len = C;
      D->first_rec = r0; D->cb_rec = r0 + fc;
      D->mi_off = (uint16_t)(mi_lo - lo); D->mi_len = (uint8_t)mi_len;                 // lane 0 = record 0
      D->has_cb = any_cb ? 1 : 0; D->cb_off = (uint16_t)(fc_cb_lo - fc_lo); D->cb_len = (uint8_t)fc_cb_len;
      D->has_rx = rx_empty ? 0 : 1; D->rx_len = (uint8_t)ulen; D->flags = (uint8_t)((r1_neg ? 1 : 0) | (r2_neg ? 2 : 0));
      const uint32_t nm = P.prefix_len + 1 + mi_len;
      // every int tag holds a depth <= 128 (<= 64 records per wavefront): 4 bytes each
      const uint32_t size = 32 + nm + 1 + (C + 1) / 2 + C + (3 + P.rg_len + 1) + (3 + mi_len + 1) + 3 * (4 + 4 + 7) +
                            (P.per_base_tags ? 4 * (8 + 2 * C) + 4 * (3 + C + 1) : 0) + (any_cb ? 3 + fc_cb_len + 1 : 0) + (rx_empty ? 0 : 3 + ulen + 1);
      D->rec_size = size;
      D->valid = 1;
      P.rec_sizes[slot] = (uint64_t)size + 4;
    }
  }
  s_cons = 1;
  flush_stats();
  PH(8)
  }
}

// -----------------------------------------------------------------------------------------------------
// k_call_full — the columns (and UMI characters) the fast path could not establish, compacted by the
// family kernels into N_LISTS append lists: one lane per item, every lane busy with the full
// log-sum-exp chain (call_full, base_builder.rs:1023-1054) on the glibc-compatible device libm.
// -----------------------------------------------------------------------------------------------------
struct FullParams {
  const FullItem* items; const uint32_t* count; uint32_t cap;
  const DeviceTables* T; const DeviceTables* TU;
  uint32_t min_reads; uint8_t min_cons_bq;
  uint8_t* col_code; uint8_t* col_qual; uint16_t* col_err;
  char* rx_base; uint32_t rx_stride;   // consensus-UMI characters: rx_base + slot * rx_stride + index
  uint16_t* col_depth; uint32_t min_input_bq;   // observation items (k_split_cols): the column's depth is counted here
  // direct records (FullItem.dest & FULL_DEST_DIRECT): the column is patched in the record k_split_cols wrote
  uint8_t* out; const SlotDesc* slot_desc; uint32_t* slot_err; uint32_t rg_len, per_base_tags;
  // the answers the pair writer applies (fastpath.h, FullResult): slot list * cap + i of `res` for the items of the families flagged in `flag` (null: every answer is scattered)
  FullResult* res; const uint8_t* flag; uint32_t n_flag; unsigned long long* stats;
};

// A column of a directly written record (fastpath.h: SlotDesc): the sequence nibble is OR-ed into the word that holds its byte (k_split_cols
// left it 0; the other nibble of the byte may be patched by another lane), quality, cd (observation items: the depth is counted here) and
// ce entries are stored, and the column's errors are added to the record's count for k_fix_ce.
__device__ __forceinline__ void full_patch_direct(const FullParams& P, uint64_t dest, uint32_t ob, uint32_t oq, uint32_t err, uint32_t depth, bool with_depth) {
  const uint32_t slot = (uint32_t)(dest >> 16), p = (uint32_t)dest & 0xFFFFu;
  const SlotDesc sd = P.slot_desc[slot];
  uint8_t* const rec = P.out + sd.out_off;
  const uint32_t Lc = sd.lc_seq & 0xFFFFu, o_seq = sd.lc_seq >> 16;
  const uint32_t o_qual = o_seq + ((Lc + 1u) >> 1), o_cd = o_qual + Lc + 3u + P.rg_len + 1u + 15u + 8u, o_ce = o_cd + 2u * Lc + 8u;
  const uintptr_t a = (uintptr_t)(rec + o_seq + (p >> 1));
  atomicOr((unsigned int*)(a & ~(uintptr_t)3), ob << (8u * (uint32_t)(a & 3) + ((p & 1u) ? 0u : 4u)));
  rec[o_qual + p] = (uint8_t)oq;
  const uint32_t e16 = err < 32767u ? err : 32767u;
  if (P.per_base_tags) {
    if (with_depth) { const uint16_t d16 = (uint16_t)depth; __builtin_memcpy(rec + o_cd + 2u * p, &d16, 2); }
    const uint16_t w = (uint16_t)e16; __builtin_memcpy(rec + o_ce + 2u * p, &w, 2);
  }
  if (e16) atomicAdd(&P.slot_err[slot], e16);
}
struct DirCast { __host__ __device__ __forceinline__ uint64_t operator()(const uint32_t& v) const { return (uint64_t)v; } };
typedef hipcub::TransformInputIterator<uint64_t, DirCast, const uint32_t*> DirSizeIn;
// a chunk's record offsets: its exclusive scan + the bytes of the chunks before; the last family leaves the next chunk's base
__global__ void k_dir_carry(uint64_t* __restrict__ off, const uint32_t* __restrict__ size, uint32_t n, uint64_t* __restrict__ base) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t b = base[0], local = off[i];
  off[i] = local + b;
  if (i == n - 1) base[1] = b + local + size[i];
}
// cE of the directly written records whose columns had errors: f32(total errors) / f32(total depth) (vanilla_caller.rs:1805-1808); the
// value sits 11 bytes into the cD cM cE block that follows the RG tag
__global__ void k_fix_ce(const SlotDesc* __restrict__ slot_desc, const uint32_t* __restrict__ slot_err, uint32_t n_slots, uint8_t* __restrict__ out, uint32_t rg_len) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_slots) return;
  const uint32_t e = slot_err[i];
  if (!e) return;
  const SlotDesc sd = slot_desc[i];
  const uint32_t Lc = sd.lc_seq & 0xFFFFu, o_seq = sd.lc_seq >> 16;
  const uint32_t o_t3 = o_seq + ((Lc + 1u) >> 1) + Lc + 3u + rg_len + 1u;
  const float rate = sd.sum_depth > 0 ? (float)e / (float)sd.sum_depth : 0.0f;
  const uint32_t u = __float_as_uint(rate);
  uint8_t* const q = out + sd.out_off + o_t3 + 11u;
  q[0] = (uint8_t)u; q[1] = (uint8_t)(u >> 8); q[2] = (uint8_t)(u >> 16); q[3] = (uint8_t)(u >> 24);
}
// The merge of a batch in which some families left the split pipeline (or were deferred): the directly written records of family g lie at
// dir_off[g] in `dir`; they move to their place in the final stream (the scan of ALL record sizes), a wavefront per family.
__global__ __launch_bounds__(256) void k_dir_copy(const SplitOut* __restrict__ split_out, const uint64_t* __restrict__ dir_off, const uint64_t* __restrict__ out_off,
                                                  const uint64_t* __restrict__ sizes, const uint8_t* __restrict__ dir, uint8_t* __restrict__ out, uint32_t n_grp) {
  const uint32_t g = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6)), lane = threadIdx.x & 63;
  if (g >= n_grp) return;
  if (split_out[g].status != 1) return;
  const uint64_t bytes = sizes[3 * (size_t)g] + sizes[3 * (size_t)g + 1] + sizes[3 * (size_t)g + 2];
  const uint8_t* const src = dir + dir_off[g];
  uint8_t* const dst = out + out_off[3 * (size_t)g];
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  uint64_t i = 16ull * lane;
  for (; i + 16 <= bytes; i += 1024) { u32x4 v; __builtin_memcpy(&v, src + i, 16); __builtin_memcpy(dst + i, &v, 16); }
  const uint64_t whole = bytes & ~15ull;
  if (lane < (uint32_t)(bytes - whole)) dst[whole + lane] = src[whole + lane];
}

// Round 5: two phases per workgroup.  Phase 1 (a thread per item): the sums of an observation item, then the TABLE answer of a column that
// shows one base (try_unanimous_fast_path, base_builder.rs:883-994) — most observation items of k_split_cols's packed pass are such columns
// (one base seen fewer times than its gate-free depth) and end here.  What needs the log-sum-exp chain (call_full: several hundred f64
// instructions through the libm port) is appended to a list in LDS, and phase 2 runs it with the list's entries side by side in the
// lanes: a wavefront pays for call_full only when it holds such columns, and then with all its lanes busy — before, one such item in
// 64 kept the whole wavefront in the chain.
__global__ __launch_bounds__(256) void k_call_full(FullParams P) {
  __shared__ double sLL[256][4];
  __shared__ unsigned long long sDest[256];
  __shared__ uint32_t sObs[256];         // observation counts, a byte each, in the order of sLL; bit 31 of sKind: an observation item (depth counted here)
  __shared__ uint32_t sKind[256];
  __shared__ uint32_t sSlot[256];        // where the answer goes: the item's slot of the result array, or NO_SLOT (scattered into the planes)
  __shared__ uint32_t sCnt;
  __shared__ double sTab[94][2];         // {correct, error_per_alt} by quality: an observation item reads a pair per observation (from global memory that is a dependent ~1 us chain per item)
  const uint32_t list = blockIdx.y;
  uint32_t cnt = P.count[list];
  if (cnt > P.cap) cnt = P.cap;
  if (blockIdx.x * blockDim.x >= cnt) return;      // (the grid covers every list's capacity: most workgroups have nothing)
  if (threadIdx.x == 0) sCnt = 0;
  if (threadIdx.x < 94) { sTab[threadIdx.x][0] = P.T->t.correct[threadIdx.x]; sTab[threadIdx.x][1] = P.T->t.error_per_alt[threadIdx.x]; }
  __syncthreads();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  // what a decided column leaves (vanilla_caller.rs:1711-1748); `is_obs`: an observation item — its depth is written too
  constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;
  uint32_t n_arr = 0, n_scat = 0;                  // (fgx_debug_last_full_results) column answers of this thread: through the result array / scattered
  auto finish = [&](uint64_t dest, int bi, uint8_t q, uint32_t o0, uint32_t o1, uint32_t o2, uint32_t o3, bool is_obs, uint32_t slot) {
    const uint32_t depth = o0 + o1 + o2 + o3;
    const uint32_t err = depth - (bi == 0 ? o0 : bi == 1 ? o1 : bi == 2 ? o2 : bi == 3 ? o3 : 0u);
    const uint8_t code = bi >= 0 ? (uint8_t)(1u << bi) : 15;
    uint8_t ob, oq;
    if (depth < P.min_reads) { ob = 15; oq = 0; }
    else if (q < P.min_cons_bq) { ob = 15; oq = FGX_MIN_PHRED; }
    else { ob = code; oq = q; }
    if (dest & FULL_DEST_DIRECT) { full_patch_direct(P, dest, ob, oq, err, depth, is_obs); return; }
    if (slot != NO_SLOT) {   // the family's writer applies it (observation items only: the depth travels too)
      FullResult r;
      r.w0 = ((uint32_t)dest & 0xFFFFu) | ((uint32_t)ob << 16) | ((uint32_t)oq << 24); r.w1 = (err < 32767u ? err : 32767u) | (depth << 16);
      P.res[slot] = r;
      n_arr++;
      return;
    }
    n_scat++;
    P.col_code[dest] = ob; P.col_qual[dest] = oq; P.col_err[dest] = (uint16_t)(err < 32767u ? err : 32767u);
    if (is_obs) P.col_depth[dest] = (uint16_t)depth;
  };
  auto push = [&](uint64_t dest, const double* ll, uint32_t obs, uint32_t kind, uint32_t slot) {
    const uint32_t k = atomicAdd(&sCnt, 1u);
    sLL[k][0] = ll[0]; sLL[k][1] = ll[1]; sLL[k][2] = ll[2]; sLL[k][3] = ll[3];
    sDest[k] = dest; sObs[k] = obs; sKind[k] = kind; sSlot[k] = slot;
  };
  if (i < cnt) {
    FullItem it = P.items[(size_t)list * P.cap + i];
    // an observation or continuation item of the packed build carries its family's index + 1 in `obs`: does the pair writer apply that family's answers?
    const bool obs_kind = it.chains == FULL_ITEM_CONT || (it.chains & FULL_ITEM_OBS) != 0;
    const uint32_t slot = (P.flag && obs_kind && it.obs != 0u && it.obs <= P.n_flag && P.flag[it.obs - 1u]) ? list * P.cap + i : NO_SLOT;
    if (it.chains == FULL_ITEM_CONT) {   // observations 16 .. of the column whose head item sits before it (or padding): no answer of its own
      if (slot != NO_SLOT) { FullResult r; r.w0 = FULL_RESULT_NONE << 16; r.w1 = 0u; P.res[slot] = r; }
    }
    else if (it.chains & FULL_ITEM_OBS) {
      // a column k_split_cols did not answer: its observations in file order, 16 bits each — the four-lane Kahan sum of
      // ConsensusBaseBuilder::add (base_builder.rs:836-868), then the call.  More than 16 of them: the following items hold the rest.
      const uint32_t m = it.chains & 0xFF;
      ColumnAcc acc;
      acc.reset();
      const ConsensusTables& TT = P.T->t;
      for (uint32_t k0 = 0; k0 < m; k0 += 16) {
        uint16_t ob16[16];
        if (k0 == 0) __builtin_memcpy(ob16, it.ll, 32);
        else __builtin_memcpy(ob16, P.items[(size_t)list * P.cap + i + (k0 >> 4)].ll, 32);
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) {
          if (k0 + j < m) {
            const uint32_t o = ob16[j], q = o & 0xFF, code = (o >> 8) & 15;
            const int bl = bam::code_to_lane((uint8_t)code);
            if (bl != 255 && q >= P.min_input_bq) { const uint32_t qq = q < 93 ? q : 93; acc.add(bl, sTab[qq][0], sTab[qq][1]); }
          }
        }
      }
      int bi = -1;
      uint8_t q = FGX_MIN_PHRED;
      if (acc.contributions() == 0 || unanimous_fast_path(TT, acc.s, acc.obs, &bi, &q)) finish(it.dest, bi, q, acc.obs[0], acc.obs[1], acc.obs[2], acc.obs[3], true, slot);
      else push(it.dest, acc.s, acc.obs[0] | (acc.obs[1] << 8) | (acc.obs[2] << 16) | (acc.obs[3] << 24), 0x80000000u, slot);
    } else {
      if (it.chains) {   // chains by order of appearance (k_simplex_wave2 / k_simplex_seg): the bases are sorted out here, once per item
        const uint32_t b1 = it.chains & 15, b2 = (it.chains >> 4) & 15, b3 = (it.chains >> 8) & 15;
        const double c1 = it.ll[0], c2 = it.ll[1], c3 = it.ll[2], cR = it.ll[3];
        const uint32_t n1 = it.obs & 0xFF, n2 = (it.obs >> 8) & 0xFF, n3 = (it.obs >> 16) & 0xFF, nR = it.obs >> 24;
        uint32_t packed = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
          const uint32_t code = 1u << k;
          it.ll[k] = code == b1 ? c1 : code == b2 ? c2 : code == b3 ? c3 : cR;
          packed |= (code == b1 ? n1 : code == b2 ? n2 : code == b3 ? n3 : nR) << (8 * k);
        }
        it.obs = packed;
      }
      push(it.dest, it.ll, it.obs, 0u, NO_SLOT);       // (the kernels that send these have run their gates already)
    }
  }
  __syncthreads();
  const uint32_t todo = sCnt;
  if (threadIdx.x < todo) {
    const uint32_t k = threadIdx.x;
    const uint64_t dest = sDest[k];
    const double ll[4] = {sLL[k][0], sLL[k][1], sLL[k][2], sLL[k][3]};
    const uint32_t ob = sObs[k];
    const bool is_rx = (dest >> 63) != 0;
    const ConsensusTables& T = is_rx ? P.TU->t : P.T->t;
    int bi;
    uint8_t q;
    call_full(T, ll, &bi, &q);
    if (is_rx) {
      const uint64_t d = dest & ~(1ull << 63);
      P.rx_base[(size_t)(d >> 8) * P.rx_stride + (d & 0xFF)] = bi >= 0 ? "ACGT"[bi] : 'N';
    } else finish(dest, bi, q, ob & 0xFF, (ob >> 8) & 0xFF, (ob >> 16) & 0xFF, ob >> 24, (sKind[k] >> 31) != 0, sSlot[k]);
  }
  if (P.stats) {   // one atomic per wavefront and counter, spread over the slots
    const uint32_t t_arr = wave_sum(n_arr), t_scat = wave_sum(n_scat);
    if ((threadIdx.x & 63) == 0) {
      unsigned long long* fs = P.stats + (size_t)((blockIdx.x * 4 + blockIdx.y + (threadIdx.x >> 6)) & (STAT_SLOTS - 1)) * FULL_STATS_STRIDE;
      if (t_arr) atomicAdd(&fs[0], (unsigned long long)t_arr);
      if (t_scat) atomicAdd(&fs[1], (unsigned long long)t_scat);
    }
  }
}

// -----------------------------------------------------------------------------------------------------
// pass B: one wavefront per consensus read
// -----------------------------------------------------------------------------------------------------
#include "record_writers.inc"

#include "simplex_wave2.inc"
#include "simplex_seg.inc"
#include "simplex_split.inc"
#include "simplex_deep.inc"
#include "duplex_deep.inc"
#include "codec_deep.inc"
#include "simplex_wide.inc"
#include "duplex_meth.inc"

// Upper bound on the consensus columns a batch can produce: a family yields at most three ends, each no
// longer than its longest read, and l_seq <= (block_size - 33) * 2 / 3.
// Per family: the scratch-column bound, and a descriptor {byte offset of its first record, bytes up to the end of its last record,
// record count} — with it k_simplex_wave2 starts loading the family's bytes one memory round trip earlier (it needs neither
// grp_first nor rec_off to know where they are; it checks afterwards that every record lies inside that span).
// (+ how many records sit in families of at most 32 records: what decides between the two heads of the simplex launch chain)
__global__ void k_col_bound(const uint32_t* __restrict__ grp_first, const uint32_t* __restrict__ rec_len, const uint64_t* __restrict__ rec_off, uint32_t n_grp,
                            uint64_t* __restrict__ bound, uint32_t max_ends, uint4* __restrict__ fam_desc, unsigned long long* __restrict__ small_recs, uint64_t* __restrict__ sizes_tail) {
  uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  {
    uint32_t mine = 0;
    if (g < n_grp) { const uint32_t n = grp_first[g + 1] - grp_first[g]; mine = (grp_first[g + 1] >= grp_first[g] && n <= 64u) ? n : 0u; }
    // one global atomic per WORKGROUP (a wavefront's sum goes through LDS first): 78 k same-address atomics per 5 M families were most of this kernel's 1 ms
    __shared__ unsigned int s_tot;
    if (threadIdx.x == 0) s_tot = 0;
    __syncthreads();
    const uint32_t tot = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && tot) atomicAdd(&s_tot, tot);
    __syncthreads();
    if (threadIdx.x == 0 && s_tot) atomicAdd(small_recs, (unsigned long long)s_tot);
  }
  if (g >= n_grp) return;
  if (g == n_grp - 1) { bound[n_grp] = 0; *sizes_tail = 0; }  // (both scans of the step run over one element more, a zero: their last element is the total)
  uint32_t a = grp_first[g], b = grp_first[g + 1], mx = 0;
  {   // the family's longest record: four lengths per load where the table allows it (a thread-per-family loop of single loads cost 1 ms per 80 M records)
    uint32_t r = a;
    if (((uintptr_t)rec_len & 15u) == 0) {
      for (; r < b && (r & 3u); r++) { const uint32_t l = rec_len[r]; mx = l > mx ? l : mx; }
      for (; r + 4 <= b; r += 4) {
        const uint4 v = *(const uint4*)(rec_len + r);
        const uint32_t m01 = v.x > v.y ? v.x : v.y, m23 = v.z > v.w ? v.z : v.w, m4 = m01 > m23 ? m01 : m23;
        mx = m4 > mx ? m4 : mx;
      }
    }
    for (; r < b; r++) { const uint32_t l = rec_len[r]; mx = l > mx ? l : mx; }
  }
  uint32_t lb = mx > 33 ? (mx - 33) * 2 / 3 + 1 : 1;
  uint32_t ends = (b - a) < max_ends ? (b - a) : max_ends;
  bound[g] = (uint64_t)ends * lb + COL_BOUND_PAD;
  uint64_t lo = 0;
  uint32_t span = 0xFFFFFFFFu;                               // no usable span (empty group, descending or far-apart records)
  if (b > a) {
    lo = rec_off[a];
    const uint64_t hi = rec_off[b - 1] + rec_len[b - 1];
    if (hi >= lo && hi - lo < 0xFFFFFFFFull) span = (uint32_t)(hi - lo);
  }
  fam_desc[g] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), span, b - a);
}

__global__ void k_reduce_stats(const unsigned long long* __restrict__ slots, unsigned long long* __restrict__ out, const unsigned long long* __restrict__ full_stats, uint32_t full_out) {
  uint32_t k = threadIdx.x;   // one thread per counter; the slots' entries 28 .. 31 are diagnostics (k_split_finish: families per build) and go to out[40 ..]
  if (k >= 32 && k < 32 + FULL_STATS_N + OV_STATS_N) {    // the counters of the result array (fastpath.h, FullResult) and, behind them, of the packed overlap step: slots of their own
    unsigned long long v = 0;
    for (int i = 0; i < STAT_SLOTS; i++) v += full_stats[(size_t)i * FULL_STATS_STRIDE + (k - 32)];
    out[full_out + (k - 32)] = v;
  }
  if (k >= 32) return;
  unsigned long long v = 0;
  for (int i = 0; i < STAT_SLOTS; i++) v += slots[(size_t)i * 32 + k];
  out[k < FGX_STATS_LEN ? k : 40 + (k - FGX_STATS_LEN)] = v;
}

}  // namespace

#include "canon_deep.inc"

// -----------------------------------------------------------------------------------------------------
// host driver
// -----------------------------------------------------------------------------------------------------
// diagnostics of a batch (fgx_debug_last_chain: bench.py's share_of_8 block): kernel launches and host synchronisations of run_once
#define FGX_SYNC(st) do { fp.last_host_syncs++; hip_check(hipStreamSynchronize(st), "sync"); } while (0)
// every kernel launch of the driver: counted, and a refused launch is reported under its own kernel's name
// (a macro around hipLaunchKernelGGL: tests/wavemu redefines that name to run the kernels on the CPU)
#define FGX_LAUNCH(kernel, grid, block, lds, st, ...) do { fp.last_launches++; hipLaunchKernelGGL((kernel), grid, block, lds, st, __VA_ARGS__); hip_check(hipGetLastError(), #kernel " launch"); } while (0)

void FastPath::release() {
  for (DevBuf* b : {&d_ends, &d_sizes, &d_offsets, &d_code, &d_qual, &d_depth, &d_err, &d_misc, &d_deferred, &d_out, &d_scan_tmp, &d_strings, &d_obs, &d_obs_all, &d_retry2,
                    &d_retry, &d_bound, &d_colbase, &d_statslots, &d_full_items, &d_full_count, &d_full_res, &d_full_flag, &d_retry_old, &d_w2img, &d_famdesc, &d_fwimg,
                    &d_split_rec, &d_split_fam, &d_split_out, &d_route, &d_s2img, &d_dir_size, &d_dir_off, &d_dir_base, &d_slot_desc, &d_slot_err, &d_out2, &d_scan_tmp2, &d_big, &d_deep_sizes, &d_deep_row0, &d_deep_rows, &d_deep_walk, &d_deep_fams, &d_deep_out, &d_deep_out2, &d_wide_scratch, &d_wide_pass, &d_wide_pass0, &d_wide_depth, &d_mflag, &d_mu, &d_mt, &d_mslot, &d_mcontigs})
    b->free_();
  for (int i = 0; i < 4; i++) if (ev[i]) { (void)hipEventDestroy(ev[i]); ev[i] = nullptr; }
  if (s2) {
    (void)hipStreamDestroy(s2); s2 = nullptr;
    for (int i = 0; i < MAX_CHUNKS; i++) { if (ev_chunk[i]) { (void)hipEventDestroy(ev_chunk[i]); ev_chunk[i] = nullptr; } if (ev_cols[i]) { (void)hipEventDestroy(ev_cols[i]); ev_cols[i] = nullptr; } }
    if (ev_fin) { (void)hipEventDestroy(ev_fin); ev_fin = nullptr; }
    if (ev_sample) { (void)hipEventDestroy(ev_sample); ev_sample = nullptr; }
  }
}

namespace {

// ---- d_misc: the batch's counters, one 64-bit word each (a kernel gets the address of a word; u32 counters use its low half) ----------
enum MiscWord : uint32_t {
  MISC_STATS = 0,            // [0, FGX_STATS_LEN): the caller's counters, k_reduce_stats's sums over the slots; [1] = consensus reads written
  MISC_COLS_USED = 28,
  MISC_N_DEFERRED = 29,      // families on the deferred list
  MISC_N_METH_CLIPPED = 30,  // methylation-aware mode: decided families / molecules with a record of more than one CIGAR op (meth_clipped_counter); high half: deep_clipped_counter
  MISC_N_RETRY = 31,         // the retry list of the launch under way
  MISC_N_RETRY_OLD = 32,     // k_simplex_wave2 → k_family_wave<0>
  MISC_N_ROUTE = 33,         // k_split_cols → k_simplex_wave2
  MISC_SMALL_RECS = 35,      // records in families of at most 64 records (k_col_bound)
  MISC_DIR_FLAGS = 36,       // direct records: low half families whose records differ in size from the prediction, high half records past the room
  MISC_N_BIG = 37,           // families of more than 64 records: k_family's list
  MISC_N_DEEP = 38,          // families a pass of the streaming kernels hands on; duplex_deep.inc / codec_deep.inc: low half the molecules it decided, high half those of them a strand cap bit
  MISC_BUILD_FAMILIES = 40,  // [40, 44): the slots' diagnostics (k_reduce_stats): families finished by k_split_cols's packed build, by its classic builds, by the packed build's clean / general row loop
  MISC_N_SLOW = 44,          // duplex / CODEC: records the fast writer leaves to the per-field kernel
  MISC_FULL_RESULTS = 46,    // [46, 51): items answered through the result array, items scattered, families the writer applies, families refused as not in one piece, families refused for more than 64 items
  MISC_PACKED_OVERLAP = 51,  // [51, 54): behind them in the same slots — packed-build families whose overlapping mates the packed step corrected, the byte-wise steps, of those voted out by the guard
  MISC_READ_BACK = 54,       // words the end of a batch copies to the host
  MISC_WORDS = 56
};
constexpr uint32_t MISC_SPLIT_WINDOW = MISC_N_BIG - MISC_N_RETRY + 1;   // retry, route and big counts of a split stage come back as ONE copy
static_assert(FGX_STATS_LEN <= MISC_COLS_USED && MISC_BUILD_FAMILIES == 40 && MISC_BUILD_FAMILIES + (32 - FGX_STATS_LEN) <= MISC_N_SLOW,
              "k_reduce_stats writes words [0, FGX_STATS_LEN) and 40 .. of misc");
static_assert(MISC_N_METH_CLIPPED == MISC_N_DEFERRED + 1 && MISC_N_METH_CLIPPED < MISC_READ_BACK, "meth_clipped_counter: the word behind the deferred count");
static_assert(MISC_PACKED_OVERLAP == MISC_FULL_RESULTS + FULL_STATS_N && MISC_PACKED_OVERLAP + OV_STATS_N <= MISC_READ_BACK, "k_reduce_stats writes the overlap counters behind the result counters");
static_assert(MISC_N_RETRY < MISC_N_ROUTE && MISC_N_ROUTE < MISC_N_BIG && MISC_SPLIT_WINDOW == 7 && MISC_N_SLOW < MISC_READ_BACK && MISC_READ_BACK <= MISC_WORDS, "misc layout");

// ---- environment switches ---------------------------------------------------------------------------------------------------------------
// fgx_knob: measurement knobs, a constant nullptr in the product library (engine.h); getenv: switches of the product
inline bool env_not0(const char* e) { return !(e && e[0] == '0'); }
inline bool env_is1(const char* e) { return e && e[0] == '1'; }
inline int env_int(const char* e, int dflt) { return e ? atoi(e) : dflt; }
inline uint32_t env_in(const char* e, int lo, int hi, uint32_t dflt) { const int v = e ? atoi(e) : 0; return v >= lo && v <= hi ? (uint32_t)v : dflt; }

struct ProcessSwitches {   // read once per process, at the first batch
  const bool v2 = env_not0(fgx_knob("FGX_V2")), seg = env_not0(fgx_knob("FGX_SEG"));
  // (two families per wavefront measured slower than one at depth 8 — 14.9 vs 10.7 ms per 1 M families: the column phase costs
  // the same per family and a CU holds 12 instead of 20 wavefronts; kept behind FGX_SEG2=1 for experiments)
  const bool seg2 = env_is1(fgx_knob("FGX_SEG2"));
  const bool early = env_not0(fgx_knob("FGX_S2_EARLY"));                 // 0: the first chunk's record kernel behind the column bound
  const int chunks = env_int(getenv("FGX_SPLIT_CHUNKS"), 0);             // >= 1: chunks of the split pipeline
  const int nosum = env_int(fgx_knob("FGX_S2_NOSUM"), 1);                // 0: every end through the f32 sums
  const int packed = env_int(getenv("FGX_S2_PACKED"), 1);                // 0: the 64-column passes only
  const bool clean_rows = env_not0(getenv("FGX_S2_CLEAN_ROWS"));         // 0: the packed pass reads the qualities of every family (no clean test)
  const bool packed_overlap = env_not0(getenv("FGX_S2_PACKED_OVERLAP")); // 0: the overlap of every family is corrected byte by byte (no packed step)
  const bool full_results = FGX_FULL_RESULTS_DEFAULT ? env_not0(getenv("FGX_FULL_RESULTS")) : env_is1(getenv("FGX_FULL_RESULTS"));   // k_call_full's answers through the result array (fastpath.h, FullResult)
  const int s2_debug = env_int(fgx_knob("FGX_S2_DEBUG"), 0);
  const int pace = env_int(fgx_knob("FGX_S2_PACE"), 1);                  // 0: all record kernels up front
  const uint32_t s2_bytes = env_in(fgx_knob("FGX_S2_BYTES"), 2048, 32768, 0) & ~15u, s2_wpb = env_in(fgx_knob("FGX_S2_WPB"), 1, 4, 0);
  const int s2_partner = env_int(fgx_knob("FGX_S2_PARTNER"), -1);        // 1: always both first-stage kernels, 0: never
  const int s2_fixed = env_int(fgx_knob("FGX_S2_FIXED"), -1);            // 0 / 1: the generic / the 160 + 80 build
  const bool later_packed = env_not0(fgx_knob("FGX_S2_LATER_PACKED"));   // 0: the classic build in the later stages, as in round 5
  const bool verbose = env_is1(fgx_knob("FGX_S2_VERBOSE"));
  // wavefronts per workgroup of the first launch of k_simplex_seg / k_simplex_wave2 / k_family_wave.  k_simplex_wave2: the LDS of a workgroup
  // is freed when its SLOWEST wavefront is done, so small workgroups keep more wavefronts running
  const uint32_t seg_wpb = env_in(fgx_knob("FGX_SEG_WPB"), 1, WAVES_PER_BLOCK, WAVES_PER_BLOCK), w2_wpb = env_in(fgx_knob("FGX_W2_WPB"), 1, WAVES_PER_BLOCK, FGX_W2_WPB_DEFAULT),
                 fw_wpb = env_in(fgx_knob("FGX_FW_WPB"), 1, WAVES_PER_BLOCK, WAVES_PER_BLOCK);
};
struct BatchSwitches {     // read at the start of every batch: tests and tools switch these inside one process
  const char* const split_env = getenv("FGX_SPLIT");
  const bool split = env_not0(split_env);                                // FGX_SPLIT=0 / 2: never / always the split pipeline
  const int split_mode = env_int(split_env, 1);
  const bool direct = env_is1(getenv("FGX_DIRECT"));                     // (tools/direct_check.py switches it between two runs of one process)
  const bool deep = env_not0(getenv("FGX_DEEP"));
  const bool duplex_deep = env_not0(getenv("FGX_DUPLEX_DEEP"));          // 0: duplex molecules of more than 64 records are deferred, as before duplex_deep.inc
  const char* const deep_wide_env = getenv("FGX_DEEP_WIDE");
  const bool deep_wide = deep_wide_env && deep_wide_env[0] && deep_wide_env[0] != '0';   // default OFF (it does not follow FGX_OPT_IN_ALL): the wide kernels behind the streaming ones (simplex_wide.inc)
  const char* const duplex_deep_cap_env = getenv("FGX_DUPLEX_DEEP_CAP");
  const bool duplex_deep_cap = duplex_deep_cap_env && duplex_deep_cap_env[0] && duplex_deep_cap_env[0] != '0';   // default OFF (it does not follow FGX_OPT_IN_ALL): the CAP builds of duplex_deep.inc
  const char* const codec_deep_env = getenv("FGX_CODEC_DEEP");
  const bool codec_deep = codec_deep_env && codec_deep_env[0] && codec_deep_env[0] != '0';   // default OFF (it does not follow FGX_OPT_IN_ALL): CODEC molecules of more than 64 records on the device (codec_deep.inc)
  const char* const deep_clips_env = getenv("FGX_DEEP_CLIPS");
  const bool deep_clips = deep_clips_env && deep_clips_env[0] && deep_clips_env[0] != '0';   // default OFF (it does not follow FGX_OPT_IN_ALL): the clip-taking builds of k_deep_parse (plain mode) and k_duplex_deep_parse
  const char* const deep_indels_env = getenv("FGX_DEEP_INDELS");
  const bool deep_indels = deep_indels_env && deep_indels_env[0] && deep_indels_env[0] != '0';   // default OFF (it does not follow FGX_OPT_IN_ALL): the deep duplex kernels also in the canonical second pass (canon_deep.inc feeds it)
  const uint32_t seg_bytes = env_in(fgx_knob("FGX_SEG_BYTES"), 4096, 32768, 11776) & ~63u;   // 4 wavefronts x 11776 B + the static tables = 3 workgroups per CU
  const uint32_t wave_bytes = env_in(fgx_knob("FGX_WAVE_BYTES"), 1024, 22016, 0) & ~15u;     // tuning knobs (0: the FastPath's own value)
  const uint32_t lds_tile_large = env_in(fgx_knob("FGX_LDS_TILE_LARGE"), 16384, 163840, 0) & ~15u;
  const uint32_t split_fpw = env_in(fgx_knob("FGX_SPLIT_FPW"), 1, 32, 0);
};

#define FGX_LDS_ATTR(bytes, ...) lds_attr((const void*)__VA_ARGS__, bytes, #__VA_ARGS__)
void lds_attr(const void* kernel, int bytes, const char* name) {
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) hip_check(e, (std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize) for ") + name + ": the device refused the dynamic LDS size").c_str());
}

struct Slice { uint32_t bytes, wpb; int build; };   // one launch of a chain: LDS slice of a wavefront, wavefronts per workgroup, which build of the kernel

// ---- k_split_cols: which builds, over which slices -------------------------------------------------------------------------------------
struct SplitBuild { bool packed, partner; std::vector<Slice> stages; };   // (Slice.build: 1 = rows of 160 + 80 bytes as immediates)
// From the tile strides of a sample of families (64 spread evenly over the first chunk: the head of a coordinate-sorted file need not look
// like the rest) and the caller's options.  `packed_ok`: the options allow the packed pass at all.
SplitBuild choose_split_build(const SplitFam* sample, uint32_t n_sample, double mean_recs, bool packed_ok, uint32_t nsafe, const ProcessSwitches& ps) {
  SplitBuild B;
  // which of the two first-stage kernels the batch needs (a family of the other kind still finds its way: the packed kernel without a
  // partner hands it to the next launch, the partner kernel alone IS the classic kernel)
  uint32_t n_pk = 0, n160 = 0;
  for (uint32_t i = 0; i < n_sample; i++) {
    const SplitFam& F = sample[i];
    auto ok = [&](uint32_t m) { return m < 2u || (m >= nsafe && m <= S2_PACKED_MAX_ROWS); };
    n_pk += (packed_ok && ok(F.m_a) && ok(F.m_b) && ((F.len_a + 7u) >> 3) + ((F.len_b + 7u) >> 3) <= 64u) ? 1u : 0u;
    n160 += (F.qs == 160 && F.ss == 80) ? 1u : 0u;
  }
  B.packed = packed_ok && !(n_sample && 100ull * n_pk < (unsigned long long)n_sample);   // under 1 % of its shape: the classic kernel alone
  B.partner = B.packed && (ps.s2_partner >= 0 ? ps.s2_partner != 0 : 100ull * n_pk < 99ull * n_sample);
  // LDS slice of the first launch: the MEAN family's tile (rows of 160 + 80 bytes) + room for its k_call_full items, at least the
  // 4352 bytes of a 16-record family — a deeper library starts at the slice its families need instead of failing the first launch
  // as a whole (depth 12: every family took two launches, 32 ms per 1 M families).
  // (round 5: the packed pass sends every column it does not answer itself to k_call_full — also the one-base columns of too few
  // observations, which run_cols's gates answer — and keeps an 8-byte descriptor per such column at the top of the slice: 56 bytes per
  // column, ~14 columns per depth-8 family of `simulate` data: the room behind the tile is S2_ROOM_PACKED, fastpath.h)
  uint32_t bytes0 = s2_first_slice_bytes(mean_recs, B.packed);
  if (ps.s2_bytes) bytes0 = ps.s2_bytes;
  const uint32_t wpb0 = ps.s2_wpb ? ps.s2_wpb : (bytes0 <= 6528u ? 4u : bytes0 <= 13056u ? 2u : 1u);
  // rows of 160 + 80 bytes (reads up to 160 bases) have their own build: member rows at immediate offsets in the column loop.  Every slice
  // size in that build, then ONE launch of the generic build for the families with other strides (round 3 ran the generic build from the
  // second slice on — a long-tail batch spends most of its column time there)
  const int fixed = (ps.s2_fixed >= 0 ? ps.s2_fixed != 0 : 2 * n160 > n_sample) ? 1 : 0;
  const Slice all[5] = {{bytes0, wpb0, fixed}, {std::max(2 * bytes0, 8704u), 2u, fixed}, {17408u, 1u, fixed}, {34816u, 1u, fixed}, {34816u, 1u, 0}};
  for (int i = 0; i < (fixed ? 5 : 4); i++)   // (a slice no larger than the one before it, in the same build, has nothing to add)
    if (i == 0 || all[i - 1].build != all[i].build || all[i].bytes > all[i - 1].bytes) B.stages.push_back(all[i]);
  return B;
}

// ---- one batch ---------------------------------------------------------------------------------------------------------------------------
// What the stages of a batch share: the caller and its input, both streams, the route the batch takes, the kernels' base parameters, and
// the family list that one stage hands to the next.  A stage enqueues on `s` (the split pipeline also on the second stream `fp.s2`).
struct Batch {
  // (an aggregate: run_once gives the first line, the rest follows from it)
  FastPath& fp; fgx_caller* const c; const uint8_t* const d_blob; const uint64_t blob_len; const uint64_t* const d_rec_off; const uint32_t* const d_rec_len; const uint32_t n_rec;
  const uint32_t* const d_grp_first; const uint32_t n_grp; FastResult* const res; const ProcessSwitches& ps;
  const BatchSwitches sw{};
  const fgx_options& o = c->opt;
  const hipStream_t s = c->stream;
  // ---- the route ----
  const bool duplex = o.caller_kind == FGX_CALLER_DUPLEX, codec = o.caller_kind == FGX_CALLER_CODEC;
  const bool meth_on = !o.trim && o.methylation_mode != FGX_METHYLATION_DISABLED && c->genome != nullptr;
  // Methylation-aware mode (simplex, a reference set, no --trim): the streaming kernels of simplex_deep.inc are the whole pipeline — every
  // family on their list, the reference lookup / counts / normalisation in k_deep_cols<1>, MM / ML / cu / ct behind the standard record
  // (k_meth_sizes, k_meth_tail); a family outside their shape is deferred to the general path, which knows the mode.
  const bool meth_dev = !duplex && !codec && meth_on;
  // The duplex caller in the mode: the wavefront kernel's <1, 1> build annotates and normalises the four read sets of a molecule in its column
  // loops, the record writers' <1> builds apply the conversion-artifact rule, am/au/at, bm/bu/bt, MM/ML/cu/ct follow RX (duplex_meth.inc).
  const bool meth_dup = duplex && meth_on;
  const bool dup_cap = duplex && o.duplex_max_reads_per_strand > 0;   // the CAP builds of k_family_wave<1> and of the duplex record writers
  // Duplex molecules of more than 64 records (duplex_deep.inc): k_family_wave<1> lists them instead of deferring them, and k_duplex_deep_parse +
  // k_duplex_deep_cols decide the list.  Not under --trim or --rejects, not in the methylation-aware mode, and in the canonical second pass only with
  // FGX_DEEP_INDELS=1, where the canonical molecules of 65 .. 512 records are theirs (FGX_DUPLEX_DEEP=0: off)
  const bool dup_deep = duplex && sw.duplex_deep && !o.trim && !o.track_rejects && !fp.rejects_pass && !meth_dup && (!fp.canon_second_pass || sw.deep_indels);
  // ... and their CAP builds, which decide a --max-reads-per-strand that bites a set of such a molecule (FGX_DUPLEX_DEEP_CAP=1; off: it is deferred)
  const bool dup_deep_cap = dup_deep && dup_cap && sw.duplex_deep_cap;
  // CODEC molecules of more than 64 records (codec_deep.inc; FGX_CODEC_DEEP=1): k_family_wave<2> lists them instead of deferring them, and k_codec_deep_parse +
  // k_codec_deep_cols decide the list — up to 254 records.  Not under --trim or --rejects, not in the canonical second pass.  (The CODEC caller has no
  // methylation-aware mode, and the host keeps non-default duplex-disagreement thresholds off the whole device path.)
  const bool codec_deep = codec && sw.codec_deep && !o.trim && !o.track_rejects && !fp.rejects_pass && !fp.canon_second_pass;
  // Simplex without --trim: which head of the launch chain?  Shallow families (the mean family fits a quarter of a wave's LDS
  // slice) start at k_simplex_seg<4>; everything else at the split pipeline (k_split_parse + k_split_cols, simplex_split.inc),
  // whose record kernel also leaves what k_col_bound would (column bound, byte-span descriptor).
  const bool simplex_v2 = !duplex && !codec && !o.trim && ps.v2 && !meth_dev;
  const double mean_span = (double)blob_len / (double)n_grp + 48.0;   // mean bytes of a family + alignment / read-ahead slack
  const double mean_recs = (double)n_rec / (double)n_grp;
  const bool seg4 = simplex_v2 && ps.seg && mean_span + (16 * 8 + 64) <= sw.seg_bytes / 4;
  bool use_split = false, direct = false;   // (known after the column bound's synchronisation)
  // ---- sizes, buffers ----
  const uint32_t n_slots = 3 * n_grp;       // simplex: Fragment, R1, R2 of each family; duplex: slot 0 unused, R1, R2
  uint64_t col_cap = 0, dir_cap = 0; uint32_t full_cap = 0;
  bool full_results = false;                // k_call_full's answers of this batch go to the pair writer through fp.d_full_res (fastpath.h, FullResult)
  static constexpr size_t FULL_STATS_BYTES = (size_t)STAT_SLOTS * FULL_STATS_STRIDE * 8;
  FullResult* full_res() const { return (FullResult*)((uint8_t*)fp.d_full_res.p + FULL_STATS_BYTES); }
  unsigned long long* misc = nullptr;
  uint32_t* cnt(MiscWord w) const { return (uint32_t*)(misc + w); }
  FastParams P;                             // the kernels' parameters; a launch works on a copy with its list and slice
  uint64_t runs_word = 0;                   // methylation-aware mode: the word behind the contig table (meth_ref_runs)
  // the split pipeline: families per wavefront of the record kernel, chunks, families per chunk; the record kernel's parameters
  uint32_t fpw = 0, n_chunks = 0, chunk_fam_raw = 0, chunk_fam = 0;
  FastParams PK;
  bool early_parse = false;
  bool s2_busy = false, s2_joining = false;   // work enqueued on the second stream / `s` waits for the last of it, the host has not yet waited for `s`
  // ---- what a stage hands to the next ----
  // the list of families the next stage takes (nullptr: all, in file order), and the two retry lists the stages fill in turn
  uint32_t* lists[2] = {nullptr, nullptr};
  const uint32_t* cur_list = nullptr; uint32_t n_cur = 0; int out_list = 0;
  uint32_t h_route_seen = 0, h_big_seen = 0; bool split_counts_seen = false;   // what the split stages' last synchronisation read
  uint32_t n_big = 0; const uint32_t* big_list = nullptr;                      // families of more than 64 records
  uint64_t n_full = 0;
  bool dir_pure = false; uint32_t dir_routed = 0; uint64_t dir_total = 0;      // direct records
  uint64_t out_len = 0; uint8_t* out_ptr = nullptr;

  // A stage that throws (a refused allocation, a failed call) unwinds while the second stream may still read the caller's records and
  // write the split descriptors: wait for it.  Nothing to do on the regular ways out: they lie behind a synchronisation of `s` that
  // followed the join.
  ~Batch() { if (s2_busy) (void)hipStreamSynchronize(fp.s2); }

  void sync() { FGX_SYNC(s); if (s2_joining) { s2_busy = false; s2_joining = false; } }
  void join_s2(hipEvent_t ev) { hip_check(hipStreamWaitEvent(s, ev, 0), "wait"); s2_joining = true; }
  void scan_u64(uint64_t* in, uint64_t* out, uint32_t n, const char* what) {
    size_t tb = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)n, s);
    fp.d_scan_tmp.reserve(tb);
    hip_check(hipcub::DeviceScan::ExclusiveSum(fp.d_scan_tmp.p, tb, in, out, (int)n, s), what);
  }
  // The tables of a caller never change: one image of a kernel's LDS tables per FastPath, built on the host by the first batch that needs it
  template <class Image> const void* table_image(DevBuf& d, void (*build)(Image&, const ConsensusTables&), const char* what) {
    if (!d.p) {
      const auto img = std::make_unique<Image>();
      build(*img, c->h_tables.t);
      d.reserve(sizeof(Image));
      hip_check(hipMemcpyAsync(d.p, img.get(), sizeof(Image), hipMemcpyHostToDevice, s), what);
      sync();   // (the host copy ends with this scope)
    }
    return d.p;
  }
  // a launch over the current list with an LDS slice of `bytes` per wavefront (`retry`: what does not fit goes on the other list; else it is deferred)
  FastParams stage_params(uint32_t bytes, bool retry) {
    hip_check(hipMemsetAsync(cnt(MISC_N_RETRY), 0, 4, s), "memset");
    FastParams PS = P;
    PS.group_list = cur_list; PS.lds_wave_bytes = bytes;
    PS.retry = retry ? lists[out_list] : nullptr; PS.n_retry = cnt(MISC_N_RETRY);
    return PS;
  }
  void next_list(uint32_t n) { cur_list = lists[out_list]; n_cur = n; out_list ^= 1; }

  // ---- buffers, counters, events ----
  void set_up() {
    fp.last_meth_device = 0; fp.last_meth_clipped = 0; fp.last_direct = 0; fp.last_split_chunks = 0;
    if (!fp.canon_second_pass) fp.last_deep_indels = fp.last_deep_clipped = fp.last_duplex_deep = fp.last_duplex_deep_capped = fp.last_codec_deep = fp.last_codec_deep_capped = 0;   // (the second pass belongs to the batch whose first pass counted)
    fp.last_routed = 0; fp.last_big_families = 0; fp.last_deep_families = 0; fp.last_wide_families = 0; fp.last_packed_families = 0; fp.last_classic_families = 0; fp.last_packed_clean = 0; fp.last_packed_general = 0; for (uint64_t& v : fp.last_packed_overlap) v = 0; for (uint64_t& v : fp.last_full_results) v = 0; fp.last_split_build = 0; fp.last_first_stage_retries = 0;
    fp.d_ends.reserve((size_t)n_slots * (duplex ? sizeof(DuplexDesc) : codec ? sizeof(CodecDesc) : sizeof(EndDesc)));
    fp.d_sizes.reserve(((size_t)n_slots + 1) * 8);            // (+ 1: a zero behind the last size, so that the scan's last element IS the total — one small copy fewer per step)
    fp.d_offsets.reserve(((size_t)n_slots + 1) * 8);
    fp.d_deferred.reserve((size_t)n_grp * 4);
    fp.d_misc.reserve(MISC_WORDS * 8);
    hip_check(hipMemsetAsync(fp.d_misc.p, 0, MISC_WORDS * 8, s), "memset");
    misc = fp.d_misc.as<unsigned long long>();
    const std::string strs = c->prefix + c->rg;   // strings: prefix | rg
    fp.d_strings.reserve(strs.size() + 16);
    if (!strs.empty()) hip_check(hipMemcpyAsync(fp.d_strings.p, strs.data(), strs.size(), hipMemcpyHostToDevice, s), "H2D strings");
    for (int i = 0; i < 4; i++) if (!fp.ev[i]) hip_check(hipEventCreate(&fp.ev[i]), "hipEventCreate");
    // column scratch: deterministic per-family slots from an exclusive scan of the column bound
    fp.d_bound.reserve(((size_t)n_grp + 1) * 8); fp.d_colbase.reserve(((size_t)n_grp + 1) * 8);
    fp.d_statslots.reserve((size_t)STAT_SLOTS * 32 * 8);
    hip_check(hipMemsetAsync(fp.d_statslots.p, 0, (size_t)STAT_SLOTS * 32 * 8, s), "memset");
    fp.d_famdesc.reserve((size_t)n_grp * 16);
    hip_check(hipEventRecord(c->ev0, s), "event");
    hip_check(hipEventRecord(fp.ev[0], s), "event");   // the family stage: record kernel / column bound, scan, family kernels, k_call_full
    // split pipeline: as many families per wavefront of the record kernel as fill its 64 lanes on average;
    // chunks of at least ~150 000 families (a column kernel of 37 500 workgroups: 20 rounds of the chip's resident workgroups, so that its tail — the
    // last round runs with a part of the chip — stays a few per cent), eight at most: one rank's share of an 8-way strong-scaling run (625 000
    // families) took 8 chunks of 78 000 until round 6 and spent a third of its step in launch gaps and kernel tails (bench.py share_of_8)
    fpw = mean_recs >= 1.0 ? (uint32_t)(64.0 / mean_recs) : 16u;
    fpw = fpw < 1u ? 1u : fpw > 16u ? 16u : fpw;
    if (sw.split_fpw) fpw = sw.split_fpw;
    n_chunks = ps.chunks >= 1 ? (uint32_t)ps.chunks : std::min<uint32_t>(8u, std::max<uint32_t>(1u, n_grp / 150000u));
    if (n_chunks > (uint32_t)FastPath::MAX_CHUNKS - 1) n_chunks = FastPath::MAX_CHUNKS - 1;   // (the last event marks where the second stream starts)
    chunk_fam_raw = (n_grp + n_chunks - 1) / n_chunks;
    chunk_fam = ((chunk_fam_raw + 4 * fpw - 1) / (4 * fpw)) * (4 * fpw);      // whole workgroups of both kernels per chunk
  }

  // ---- column bound, its scan, and the one synchronisation every batch has: which route, how much room ----
  void bound_columns() {
    FGX_LAUNCH(k_col_bound, dim3((n_grp + 1023) / 1024), dim3(1024), 0, s, d_grp_first, d_rec_len, d_rec_off, n_grp, fp.d_bound.as<uint64_t>(), duplex ? 4u : codec ? 2u : 3u,
               fp.d_famdesc.as<uint4>(), misc + MISC_SMALL_RECS, fp.d_sizes.as<uint64_t>() + n_slots);
    scan_u64(fp.d_bound.as<uint64_t>(), fp.d_colbase.as<uint64_t>(), n_grp + 1, "scan bound");
    // (round 6: every small device-to-host copy costs the stream ~25 us, timeline of the 625 000-family step — so the total is the scan's own last element)
    uint64_t col_total = 0;
    hip_check(hipMemcpyAsync(&col_total, fp.d_colbase.as<uint64_t>() + n_grp, 8, hipMemcpyDeviceToHost, s), "D2H");
    unsigned long long small_recs = 0;
    hip_check(hipMemcpyAsync(&small_recs, misc + MISC_SMALL_RECS, 8, hipMemcpyDeviceToHost, s), "D2H");
    sync();
    // The split pipeline is the faster head for every family it keeps (depth 8: 25.7 against 37 ms per 5 M families) — since round 4 that is
    // every family of up to 64 records in the common shape (an end of more than 16 reads sends its disagreeing columns to k_call_full as
    // several items); larger families it only measures and hands to k_family.  Split when at least half of the reads sit in families of
    // at most 64 records (FGX_SPLIT=0 / 2: never / always).
    use_split = simplex_v2 && sw.split && !seg4 && (sw.split_mode == 2 || (double)small_recs >= 0.5 * (double)n_rec);
    // Direct records (fastpath.h): the split pipeline's column kernel writes the consensus records itself (FGX_DIRECT=1).  Byte-identical on
    // the GPU (tools/direct_check.py, tests/test_gpu_direct_records.py), but NOT the default: measured on 5 M depth-8 families the column kernel
    // pays for the emission what k_emit cost as a kernel of its own (k_split_cols 2.82 -> 3.82 ms per chunk, k_split_parse 0.94 -> 1.41 ms with the
    // size prediction; step 33.7 -> 40.2 ms with the merge, ~34 ms without: profiles/r04_experiments.md) — vector-instruction issue is what the
    // stage is short of, and the record's constant bytes cost as many instructions written from here as from there.
    direct = use_split && sw.direct && !fp.direct_off && !meth_dev;
    if (early_parse && !use_split) join_s2(fp.ev_chunk[0]);   // (its descriptors are not used; nothing of this batch may still run when the call returns)
    col_cap = col_total + 64;
    if (direct) {
      // room for the records: 6 bytes per column of the (generous) column bound covers sequence + qualities + cd + ce twice over for
      // simulate-shaped reads; names and tags come on top.  A batch that needs more says so (dir_flags[1]) and runs again with what it asked for.
      dir_cap = std::max<uint64_t>(col_cap * 6 + (uint64_t)n_slots * 64 + 4096, fp.dir_cap_min);
      fp.d_out.reserve(dir_cap + 64);
      fp.d_dir_size.reserve((size_t)n_grp * 4 + 64); fp.d_dir_off.reserve((size_t)n_grp * 8 + 64); fp.d_dir_base.reserve((FastPath::MAX_CHUNKS + 2) * 8);
      fp.d_slot_desc.reserve((size_t)n_slots * sizeof(SlotDesc)); fp.d_slot_err.reserve((size_t)n_slots * 4);
      hip_check(hipMemsetAsync(fp.d_dir_size.p, 0, (size_t)n_grp * 4, s), "memset");
      hip_check(hipMemsetAsync(fp.d_dir_base.p, 0, (FastPath::MAX_CHUNKS + 2) * 8, s), "memset");
      hip_check(hipMemsetAsync(fp.d_slot_err.p, 0, (size_t)n_slots * 4, s), "memset");
      hip_check(hipMemsetAsync(fp.d_sizes.p, 0, ((size_t)n_slots + 1) * 8, s), "memset");
    }
    fp.d_code.reserve(col_cap + 64); fp.d_qual.reserve(col_cap + 64); fp.d_err.reserve(col_cap * 2 + 64);   // (+ slack: k_emit reads whole dwords)
    if (meth_dev || meth_dup) {
      fp.d_mflag.reserve(col_cap + 64); fp.d_mu.reserve(col_cap * 2 + 64); fp.d_mt.reserve(col_cap * 2 + 64);
      fp.d_mslot.reserve((size_t)n_slots * (meth_dup ? sizeof(DuplexMethSlot) : sizeof(MethSlot)) + 64);
    }
    if (duplex) fp.d_obs.reserve(col_cap * 4); else fp.d_depth.reserve(col_cap * 2 + 64);
    if (dup_cap) fp.d_obs_all.reserve(col_cap * 4);   // the all-reads counts of the molecules the cap bites: only a caller with a cap pays for them
  }

  // ---- the kernels' base parameters, the call_full pool, the retry lists ----
  void fill_params() {
    memset(&P, 0, sizeof(P));
    P.blob = d_blob; P.rec_off = d_rec_off; P.rec_len = d_rec_len; P.grp_first = d_grp_first;
    P.blob_len = blob_len;
    P.T = c->d_tables.as<DeviceTables>(); P.TU = c->d_umi_tables.as<DeviceTables>();
    P.fw_image = table_image<FwLds>(fp.d_fwimg, build_fw_image, "H2D fw image");   // k_family_wave's LDS block
    P.min_reads = o.min_reads; P.max_reads = o.max_reads;
    P.min_input_bq = o.min_input_base_quality; P.min_cons_bq = o.min_consensus_base_quality;
    // k_split_cols's sum-free observation step: from how many agreeing observations a column is the cap whatever their qualities (gate_core.h)
    P.s2_packed = (ps.packed ? 1u : 0u) | ((ps.packed && ps.s2_debug) ? 2u : 0u) | ((ps.packed && ps.clean_rows) ? 4u : 0u) | ((ps.packed && ps.packed_overlap) ? 8u : 0u);
    P.s2_nsafe = ps.nosum ? unanimous_cap_depth(c->h_tables.t, (uint32_t)o.min_input_base_quality & 0xFFu, 64u) : FGX_NEVER_CAP;
    P.trim = o.trim; P.overlap = o.overlapping_consensus;
    if (duplex) {   // single-strand caller of the duplex caller (duplex_caller.rs:474-489): min_reads 1, min consensus base quality 2
      P.min_reads = 1; P.max_reads = -1; P.min_cons_bq = FGX_MIN_PHRED;
      P.dmin_total = o.duplex_min_reads[0]; P.dmin_xy = o.duplex_min_reads[1]; P.dmin_yx = o.duplex_min_reads[2];
      P.dmax_reads = o.duplex_max_reads_per_strand;
      P.col_obs = fp.d_obs.as<uint32_t>(); P.dends = fp.d_ends.as<DuplexDesc>();
      if (dup_cap) P.col_obs_all = fp.d_obs_all.as<uint32_t>();
    }
    if (codec) {    // single-strand caller of the CODEC caller (codec_caller.rs:374-397): min_reads 1, no cap, min consensus base quality 0
      P.min_reads = 1; P.max_reads = -1; P.min_cons_bq = 0; P.trim = 0; P.overlap = 0;
      P.cends = fp.d_ends.as<CodecDesc>(); P.cmin_reads = o.codec_min_reads_per_strand; P.cmax_reads = o.codec_max_reads_per_strand;
      P.cmin_duplex_len = o.codec_min_duplex_length;
    }
    P.per_base_tags = o.produce_per_base_tags; P.track_rejects = o.track_rejects;
    P.tag0 = (duplex || codec) ? 'M' : o.tag[0]; P.tag1 = (duplex || codec) ? 'I' : o.tag[1]; P.cell0 = o.cell_tag[0]; P.cell1 = o.cell_tag[1];
    P.prefix_len = (uint32_t)c->prefix.size(); P.rg_len = (uint32_t)c->rg.size();
    P.ends = fp.d_ends.as<EndDesc>(); P.rec_sizes = fp.d_sizes.as<uint64_t>();
    P.col_code = fp.d_code.as<uint8_t>(); P.col_qual = fp.d_qual.as<uint8_t>(); P.col_depth = fp.d_depth.as<uint16_t>(); P.col_err = fp.d_err.as<uint16_t>();
    if (meth_dev || meth_dup) {
      const GenomeRef* gr = c->genome.get();
      const uint32_t n_ref = (uint32_t)gr->off.size();
      fp.d_mcontigs.reserve((size_t)(n_ref + 1) * 16 + 64);
      if (n_ref) {
        hip_check(hipMemcpyAsync(fp.d_mcontigs.p, gr->off.data(), (size_t)n_ref * 8, hipMemcpyHostToDevice, s), "H2D contig offsets");
        hip_check(hipMemcpyAsync(fp.d_mcontigs.as<uint64_t>() + n_ref, gr->len.data(), (size_t)n_ref * 8, hipMemcpyHostToDevice, s), "H2D contig lengths");
      }
      runs_word = (uint64_t)(uintptr_t)fp.ref_runs;      // behind the lengths: the batch's reference runs (meth_ref_runs), null outside the canonical second pass
      hip_check(hipMemcpyAsync(fp.d_mcontigs.as<uint64_t>() + 2 * (size_t)n_ref, &runs_word, 8, hipMemcpyHostToDevice, s), "H2D reference runs table");
      P.meth_mode = o.methylation_mode; P.n_ref = n_ref; P.genome = (const uint8_t*)gr->d_genome.p;
      P.contig_off = fp.d_mcontigs.as<uint64_t>(); P.contig_len = fp.d_mcontigs.as<uint64_t>() + n_ref;
      P.meth_flag = fp.d_mflag.as<uint8_t>(); P.meth_u = fp.d_mu.as<uint16_t>(); P.meth_t = fp.d_mt.as<uint16_t>();
    }
    P.col_base = fp.d_colbase.as<uint64_t>();
    if (direct) {
      P.dir_size = fp.d_dir_size.as<uint32_t>(); P.dir_off = fp.d_dir_off.as<uint64_t>(); P.out = fp.d_out.as<uint8_t>(); P.out_cap = dir_cap;
      P.out_off = fp.d_offsets.as<uint64_t>(); P.slot_desc = fp.d_slot_desc.as<SlotDesc>(); P.slot_err = fp.d_slot_err.as<uint32_t>();
      P.strings = fp.d_strings.as<char>(); P.dir_flags = cnt(MISC_DIR_FLAGS);
    }
    P.stats = fp.d_statslots.as<unsigned long long>(); P.n_deferred = cnt(MISC_N_DEFERRED);
    P.deferred = fp.d_deferred.as<uint32_t>();
    fp.d_retry.reserve((size_t)n_grp * 4);
    P.retry = fp.d_retry.as<uint32_t>(); P.n_retry = cnt(MISC_N_RETRY);
    // append lists for the columns that need call_full: room for 1 / pool_div of the column bound (overflow → general path)
    const uint64_t full_total = col_cap / fp.pool_div + (uint64_t)N_LISTS * fp.pool_slack;
    full_cap = (uint32_t)std::min<uint64_t>(full_total / N_LISTS, 0x7FFFFFFFull);
    fp.d_full_items.reserve((size_t)full_cap * N_LISTS * sizeof(FullItem));
    fp.d_full_count.reserve((size_t)N_LISTS * 4);
    hip_check(hipMemsetAsync(fp.d_full_count.p, 0, (size_t)N_LISTS * 4, s), "memset");
    P.full_items = fp.d_full_items.as<FullItem>(); P.full_count = fp.d_full_count.as<uint32_t>(); P.full_cap = full_cap;
    // the answers the pair writer applies (fastpath.h, FullResult): a slot per slot of the pool, a flag per family, four slot-spread counters.
    // Simplex on the scratch path only, and a pool whose slots a 32-bit index reaches.
    // (never without its only reader: a build without the pair writer, FGX_EMIT_PAIR=0, reads the planes)
    full_results = ps.full_results && FGX_EMIT_PAIR != 0 && !duplex && !codec && !direct && !meth_dev && (uint64_t)full_cap * N_LISTS <= 0xFFFFFFFFull;
    fp.d_full_res.reserve(FULL_STATS_BYTES + (full_results ? (size_t)full_cap * N_LISTS * sizeof(FullResult) : 0));   // (the counters in front of the slots)
    hip_check(hipMemsetAsync(fp.d_full_res.p, 0, FULL_STATS_BYTES, s), "memset");
    P.full_stats = fp.d_full_res.as<unsigned long long>();
    if (full_results) {
      fp.d_full_flag.reserve((size_t)n_grp + 16);
      hip_check(hipMemsetAsync(fp.d_full_flag.p, 0, (size_t)n_grp, s), "memset");
      P.full_results = 1; P.full_flag = fp.d_full_flag.as<uint8_t>();
    }
    P.lds_wave_bytes = sw.wave_bytes ? sw.wave_bytes : duplex ? fp.lds_wave_bytes_duplex : codec ? fp.lds_wave_bytes_codec : fp.lds_wave_bytes;
    P.lds_tile_bytes = fp.lds_tile_bytes_large;
    if (!fp.lds_attr_set) {
      FGX_LDS_ATTR(WAVES_PER_BLOCK * 22016, k_family_wave<0>);
      FGX_LDS_ATTR(WAVES_PER_BLOCK * 22016, k_family_wave<1>);
      FGX_LDS_ATTR(WAVES_PER_BLOCK * 22016, k_family_wave<2>);
      FGX_LDS_ATTR(WAVES_PER_BLOCK * 22016, k_family_wave<1, 1>);
      FGX_LDS_ATTR(WAVES_PER_BLOCK * 22016, k_family_wave<1, 0, 1>);
      FGX_LDS_ATTR(WAVES_PER_BLOCK * 22016, k_family_wave<1, 1, 1>);
      FGX_LDS_ATTR(WAVES_PER_BLOCK * 22016, k_family_wave<2, 0, 1>);
      fp.lds_attr_set = true;
    }
    fp.d_retry2.reserve((size_t)n_grp * 4);
    lists[0] = fp.d_retry.as<uint32_t>(); lists[1] = fp.d_retry2.as<uint32_t>();
    // simplex families of more than 64 records: no wavefront-per-family kernel takes them — the first kernel that sees one puts it on
    // k_family's list (round 3 walked them through k_simplex_wave2 and three k_family_wave<0> launches first: 2 ms per 1 M long-tail families)
    // (not with direct records: their merge pass walks ONE list of the families that left the split pipeline — the route list)
    if (!duplex && !codec && !direct) { fp.d_big.reserve((size_t)n_grp * 4); P.big = fp.d_big.as<uint32_t>(); P.n_big = cnt(MISC_N_BIG); }
    // duplex molecules of more than 64 records: k_family_wave<1> lists them for the kernels of duplex_deep.inc (without the list it defers them)
    if (dup_deep || codec_deep) { fp.d_big.reserve((size_t)n_grp * 4); P.big = fp.d_big.as<uint32_t>(); P.n_big = cnt(MISC_N_BIG); }   // (CODEC: k_family_wave<2>, codec_deep.inc)
    n_cur = meth_dev ? 0u : n_grp;       // (methylation-aware mode: no wavefront-per-family kernel runs)
  }

  // Wave-per-family launches over growing LDS slices: everything first, then only the groups whose records did not fit
  // (long-tail families: 6 KB holds ~18 records of 150 bp, 12 KB ~36, 22 KB all 64 a wavefront can take).
  // Fewer wavefronts per workgroup as the slices grow: the LDS a workgroup asks for is what limits the wavefronts a CU holds
  // (4 x 22 KB = one workgroup = 4 waves per CU; 1 x 22 KB = six workgroups = 6 waves)
  void wave_slices(std::vector<Slice>& st, uint32_t first_wpb) const {
    const uint32_t bytes[3] = {P.lds_wave_bytes, 12288u, 22016u};
    for (int i = 0; i < 3; i++) if (i == 0 || bytes[i] > bytes[i - 1]) st.push_back({bytes[i], i == 0 ? first_wpb : i == 1 ? 2u : 1u, 1});
  }
  // One launch per slice over the current list: a family that does not fit the slice goes on the launch's retry list, which the next launch
  // takes (`keep_last`: the last one leaves such a list too, for the stage behind the chain; else its families are deferred).  The host
  // learns the length of the next list from a 4-byte copy behind each launch.
  template <class Launch> void run_slices(const std::vector<Slice>& st, bool keep_last, Launch launch) {
    for (size_t i = 0; i < st.size() && n_cur; i++) {
      FastParams PS = stage_params(st[i].bytes, i + 1 < st.size() || keep_last);
      launch(st[i], PS);
      uint32_t n_next = 0;
      if (dup_deep || codec_deep) {   // the count of listed deep molecules travels with the copy the chain waits for anyway (the split stages' window: retry .. big)
        unsigned long long h_cnt[MISC_SPLIT_WINDOW] = {};
        hip_check(hipMemcpyAsync(h_cnt, misc + MISC_N_RETRY, sizeof(h_cnt), hipMemcpyDeviceToHost, s), "D2H");
        sync();
        n_next = (uint32_t)h_cnt[0]; n_dup_deep = (uint32_t)h_cnt[MISC_N_BIG - MISC_N_RETRY];
      } else {
        hip_check(hipMemcpyAsync(&n_next, cnt(MISC_N_RETRY), 4, hipMemcpyDeviceToHost, s), "D2H");
        sync();
      }
      next_list(PS.retry ? n_next : 0);
    }
  }

  // ---- split pipeline: k_split_parse, chunk by chunk on the second stream, under k_split_cols of the chunk before; k_split_finish ----
  void split_pipeline() {
    // k_split_cols over growing LDS slices (4 / 2 / 1 / 1 wavefronts per workgroup); what it does not take is collected in
    // `route` and starts the k_simplex_wave2 chain
    if (!fp.s2_attr_set) {
      FGX_LDS_ATTR(65536, k_split_cols<0, 0, 0, 0>);
      FGX_LDS_ATTR(65536, k_split_cols<160, 80, 0, 0>);
      FGX_LDS_ATTR(65536, k_split_cols<0, 0, 0, 1>);
      FGX_LDS_ATTR(65536, k_split_cols<160, 80, 0, 1>);
      FGX_LDS_ATTR(65536, k_split_cols<0, 0, 0, 2>);
      FGX_LDS_ATTR(65536, k_split_cols<160, 80, 0, 2>);
      FGX_LDS_ATTR(65536, k_split_cols<0, 0, 1, 0>);
      FGX_LDS_ATTR(65536, k_split_cols<160, 80, 1, 0>);
      fp.s2_attr_set = true;
    }
    P.s2_image = table_image<S2Image>(fp.d_s2img, build_s2_image, "H2D s2 image");
    fp.d_route.reserve((size_t)n_grp * 4);
    fp.d_split_out.reserve((size_t)n_grp * sizeof(SplitOut));
    if (!early_parse) prepare_parse();
    P.fam_desc = fp.d_famdesc.as<uint4>();
    P.split_rec = fp.d_split_rec.as<SplitRec>(); P.split_fam = fp.d_split_fam.as<SplitFam>(); P.split_out = fp.d_split_out.as<SplitOut>();
    P.route = fp.d_route.as<uint32_t>(); P.n_route = cnt(MISC_N_ROUTE);
    if (direct) { PK.dir_size = P.dir_size; PK.min_input_bq = o.min_input_base_quality; PK.per_base_tags = o.produce_per_base_tags; PK.rg_len = (uint32_t)c->rg.size(); }
    fp.last_split_chunks = n_chunks;
    fp.dir_chunks_run = (n_grp + chunk_fam_raw - 1) / chunk_fam_raw;     // chunks that hold families (the rounding of chunk_fam can leave the last ones empty)
    fork_s2();
    size_t dir_scan_bytes = 0;
    if (direct) {
      const DirSizeIn in(fp.d_dir_size.as<uint32_t>(), DirCast());
      (void)hipcub::DeviceScan::ExclusiveSum(nullptr, dir_scan_bytes, in, fp.d_dir_off.as<uint64_t>(), (int)std::min<uint64_t>(chunk_fam, n_grp), fp.s2);
      fp.d_scan_tmp2.reserve(dir_scan_bytes + 64);
    }
    if (!early_parse) launch_parse(0, dir_scan_bytes);
    // the sample that picks the builds: one strided copy of at most one row per family of the first chunk (the rows past it are not
    // parsed yet and hold what the previous batch left)
    SplitFam fam_sample[64];
    const uint32_t sample_span = (uint32_t)std::min<uint64_t>(chunk_fam, n_grp), sample_stride = std::max<uint32_t>(1u, sample_span / 64u);
    const uint32_t n_sample = sample_span < 64u ? sample_span : 64u;
    hip_check(hipMemcpy2DAsync(fam_sample, sizeof(SplitFam), fp.d_split_fam.p, (size_t)sample_stride * sizeof(SplitFam), sizeof(SplitFam), n_sample, hipMemcpyDeviceToHost, fp.s2), "D2H sample");
    hip_check(hipEventRecord(fp.ev_sample, fp.s2), "event");
    // (round 5) the record kernel is bound by HBM bandwidth (it reads the whole blob: 4.2 TB/s alone on the chip), and a column kernel
    // beside it gets what is left — with every chunk's record kernel queued up front, the first column kernel took 6.9 ms instead of
    // 1.7 and the two streams added up like one (profiles/r05_timeline_*.txt).  Paced: chunk k + 2 is parsed
    // when the column kernel of chunk k has finished, i.e. under the column kernel of chunk k + 1.
    const bool paced = ps.pace != 0 && n_chunks > 2;
    for (uint32_t ci = 1; ci < (paced ? 2u : n_chunks); ci++) launch_parse(ci, dir_scan_bytes);
    fp.last_host_syncs++;
    hip_check(hipEventSynchronize(fp.ev_sample), "sync");
    const bool packed_ok = !direct && P.s2_packed != 0 && P.s2_nsafe != FGX_NEVER_CAP && P.min_reads <= P.s2_nsafe && ((uint32_t)P.min_input_bq & 0xFFu) <= 128u;   // (what run_cols_packed asks of the caller's options)
    const SplitBuild B = choose_split_build(fam_sample, n_sample, mean_recs, packed_ok, P.s2_nsafe, ps);
    fp.last_split_build = B.packed ? (B.partner ? 2u : 1u) : 0u;
    cur_list = nullptr; n_cur = n_grp; out_list = 0;
    for (size_t ci = 0; ci < B.stages.size() && n_cur; ci++) {
      const Slice& S = B.stages[ci];
      FastParams PS = stage_params(S.bytes, ci + 1 < B.stages.size());
      PS.s2_partner = (B.partner || (ci > 0 && ps.later_packed && B.packed)) ? 1u : 0u;
      const bool pair_build = B.packed && (ci == 0 || ps.later_packed);
      if (ci == 0) {   // the first stage takes the families in file order, chunk by chunk behind the record kernel
        for (uint32_t k = 0; k < n_chunks; k++) {
          const uint32_t ga = k * chunk_fam, gb = (uint32_t)std::min<uint64_t>((uint64_t)ga + chunk_fam, n_grp);
          if (ga >= gb) break;
          hip_check(hipStreamWaitEvent(s, fp.ev_chunk[k], 0), "wait");
          if (S.build) launch_split_cols<160, 80>(S, pair_build, PS, ga, gb - ga); else launch_split_cols<0, 0>(S, pair_build, PS, ga, gb - ga);
          // the chunk's EndDescs / record sizes / counters (a thread per family: waits on memory, few instructions) on the second
          // stream, under the next chunk's column kernel
          hip_check(hipEventRecord(fp.ev_cols[k], s), "event");
          hip_check(hipStreamWaitEvent(fp.s2, fp.ev_cols[k], 0), "wait");
          FastParams PF = P;
          PF.group_list = nullptr; PF.g0 = ga;
          FGX_LAUNCH(k_split_finish, dim3((gb - ga + 255) / 256), dim3(256), 0, fp.s2, PF, gb - ga);
          if (paced && k + 2 < n_chunks) launch_parse(k + 2, dir_scan_bytes);
        }
      } else {
        if (S.build) launch_split_cols<160, 80>(S, pair_build, PS, 0u, n_cur); else launch_split_cols<0, 0>(S, pair_build, PS, 0u, n_cur);
        FastParams PF = P;                       // the families this (larger-slice) launch finished: the list it was given
        PF.group_list = cur_list; PF.g0 = 0;
        FGX_LAUNCH(k_split_finish, dim3((n_cur + 255) / 256), dim3(256), 0, s, PF, n_cur);
      }
      // (round 6: the route / big counters come along — after the LAST stage they are final, and two host synchronisations of their own go away)
      unsigned long long h_cnt[MISC_SPLIT_WINDOW] = {};
      hip_check(hipMemcpyAsync(h_cnt, misc + MISC_N_RETRY, sizeof(h_cnt), hipMemcpyDeviceToHost, s), "D2H");
      split_counts_seen = true;
      sync();
      const uint32_t n_next = PS.retry ? (uint32_t)h_cnt[0] : 0u;
      h_route_seen = (uint32_t)h_cnt[MISC_N_ROUTE - MISC_N_RETRY]; h_big_seen = (uint32_t)h_cnt[MISC_N_BIG - MISC_N_RETRY];
      if (ci == 0) fp.last_first_stage_retries = n_next;
      next_list(n_next);
    }
    hip_check(hipEventRecord(fp.ev_fin, fp.s2), "event");          // the per-chunk k_split_finish launches
    join_s2(fp.ev_fin);
    uint32_t n_route = h_route_seen;
    if (!split_counts_seen) {
      hip_check(hipMemcpyAsync(&n_route, cnt(MISC_N_ROUTE), 4, hipMemcpyDeviceToHost, s), "D2H");
      sync();
    }
    cur_list = fp.d_route.as<uint32_t>(); n_cur = n_route; out_list = 0;
    fp.last_routed = n_route;
    if (ps.verbose) fprintf(stderr, "[fgx] split pipeline: %u families, %u routed to k_simplex_wave2\n", n_grp, n_route);
  }
  // QS, SS: the build with rows of 160 + 80 bytes as immediates, or 0, 0.  (round 5) `pair_build`: the packed pass for the families of its shape and, when
  // PS.s2_partner announces it, run_cols for the rest as a second launch over the same families; (round 6) the later stages — the families that
  // need larger LDS slices: ends of 9 .. 31 rows — always as the pair (their lists are mixed)
  template <int QS, int SS> void launch_split_cols(const Slice& S, bool pair_build, FastParams& PS, uint32_t g_first, uint32_t count) {
    PS.g0 = g_first;
    const uint32_t wpb = std::min<uint32_t>(S.wpb, 65536u / S.bytes);   // wpb x slice within the 64 KiB requested for k_split_cols
    const size_t lds = (size_t)wpb * S.bytes;
    const dim3 grid((count + wpb - 1) / wpb), block(64 * wpb);
    if (direct) FGX_LAUNCH(HIP_KERNEL_NAME(k_split_cols<QS, SS, 1, 0>), grid, block, lds, s, PS, count);
    else if (!pair_build) FGX_LAUNCH(HIP_KERNEL_NAME(k_split_cols<QS, SS, 0, 0>), grid, block, lds, s, PS, count);
    else {
      FGX_LAUNCH(HIP_KERNEL_NAME(k_split_cols<QS, SS, 0, 1>), grid, block, lds, s, PS, count);
      if (PS.s2_partner) FGX_LAUNCH(HIP_KERNEL_NAME(k_split_cols<QS, SS, 0, 2>), grid, block, lds, s, PS, count);
    }
  }

  // ---- split pipeline: the record kernel (k_split_parse) on the second stream ----
  void prepare_parse() {   // its buffers, streams and parameters
    fp.d_split_rec.reserve((size_t)n_rec * sizeof(SplitRec) + 64);
    fp.d_split_fam.reserve((size_t)n_grp * sizeof(SplitFam) + 64);
    if (!fp.s2) {
      create_compute_stream(&fp.s2);
      for (int i = 0; i < FastPath::MAX_CHUNKS; i++) { hip_check(hipEventCreateWithFlags(&fp.ev_chunk[i], hipEventDisableTiming), "hipEventCreate"); hip_check(hipEventCreateWithFlags(&fp.ev_cols[i], hipEventDisableTiming), "hipEventCreate"); }
      hip_check(hipEventCreateWithFlags(&fp.ev_fin, hipEventDisableTiming), "hipEventCreate");
      hip_check(hipEventCreateWithFlags(&fp.ev_sample, hipEventDisableTiming), "hipEventCreate");
    }
    memset(&PK, 0, sizeof(PK));
    PK.blob = d_blob; PK.rec_off = d_rec_off; PK.rec_len = d_rec_len; PK.grp_first = d_grp_first; PK.blob_len = blob_len;
    PK.min_reads = o.min_reads; PK.max_reads = o.max_reads; PK.overlap = o.overlapping_consensus;
    PK.tag0 = o.tag[0]; PK.tag1 = o.tag[1]; PK.cell0 = o.cell_tag[0]; PK.cell1 = o.cell_tag[1];
    PK.prefix_len = (uint32_t)c->prefix.size();
    PK.split_rec = fp.d_split_rec.as<SplitRec>(); PK.split_fam = fp.d_split_fam.as<SplitFam>();
  }
  void fork_s2() {   // the second stream starts where this one is: the batch's buffers, the memsets
    hip_check(hipEventRecord(fp.ev_chunk[FastPath::MAX_CHUNKS - 1], s), "event");
    hip_check(hipStreamWaitEvent(fp.s2, fp.ev_chunk[FastPath::MAX_CHUNKS - 1], 0), "wait");
  }
  void launch_parse(uint32_t ci, size_t dir_scan_bytes = 0) {
    const uint32_t ga = ci * chunk_fam, gb = std::min<uint64_t>((uint64_t)ga + chunk_fam, n_grp);
    if (ga >= gb) return;
    const uint64_t waves = ((uint64_t)(gb - ga) + fpw - 1) / fpw;
    s2_busy = true;
    FGX_LAUNCH(k_split_parse, dim3((uint32_t)((waves + 1) / 2)), dim3(128), 0, fp.s2, PK, ga, gb, fpw, (uint64_t*)nullptr, 3u, (uint4*)nullptr);
    if (direct) {   // the chunk's record offsets: exclusive scan of the predicted family sizes, carried on from the chunk before
      const DirSizeIn in(fp.d_dir_size.as<uint32_t>() + ga, DirCast());
      hip_check(hipcub::DeviceScan::ExclusiveSum(fp.d_scan_tmp2.p, dir_scan_bytes, in, fp.d_dir_off.as<uint64_t>() + ga, (int)(gb - ga), fp.s2), "scan of the record sizes");
      FGX_LAUNCH(k_dir_carry, dim3((gb - ga + 255) / 256), dim3(256), 0, fp.s2, fp.d_dir_off.as<uint64_t>() + ga, fp.d_dir_size.as<uint32_t>() + ga, gb - ga, fp.d_dir_base.as<uint64_t>() + ci);
    }
    hip_check(hipEventRecord(fp.ev_chunk[ci], fp.s2), "event");
  }
  // (round 6) The record kernel of the FIRST chunk starts before the column bounds are counted and scanned: it needs nothing of them, and the host
  // waits for its first families anyway (their tile strides pick the column kernel's build).  Before, the second stream started behind
  // k_col_bound + scan + a host synchronisation: 0.37 ms into the step.  Launched when the batch can take the split pipeline at all; should the count of
  // small families then say otherwise, its descriptors are simply not used.
  void parse_first_chunk_early() {
    if (!(simplex_v2 && sw.split && !seg4 && !sw.direct && ps.early)) return;
    prepare_parse();
    fork_s2();
    launch_parse(0);
    early_parse = true;
  }

  // ---- k_simplex_seg<4> / <2> (4 / 2 families per wavefront, while the mean family fits a quarter / half of the wave's LDS) → k_simplex_wave2
  //      (two-accumulator column loop, the families of the common record shape) over the growing slices.  What is outside their shape is
  //      collected in `retry_old` and goes through the k_family_wave<0> launches ----
  void wave2_chain() {
    if (!fp.v2_attr_set) {
      FGX_LDS_ATTR(WAVES_PER_BLOCK * 22016, k_simplex_wave2);
      FGX_LDS_ATTR(WAVES_PER_BLOCK * 32768, k_simplex_seg<2>);
      FGX_LDS_ATTR(WAVES_PER_BLOCK * 32768, k_simplex_seg<4>);
      fp.v2_attr_set = true;
    }
    P.w2_image = table_image<W2Lds>(fp.d_w2img, build_w2_image, "H2D w2 image");
    P.fam_desc = fp.d_famdesc.as<uint4>();
    std::vector<Slice> chain;   // (Slice.build: families per wavefront)
    if (ps.seg && mean_span + (16 * 8 + 64) <= sw.seg_bytes / 4) chain.push_back({sw.seg_bytes, ps.seg_wpb, 4});
    if (ps.seg && ps.seg2 && mean_span + (32 * 8 + 64) <= sw.seg_bytes / 2) chain.push_back({sw.seg_bytes, (uint32_t)WAVES_PER_BLOCK, 2});
    // (workgroup-cooperative variants — four families' record phases on one wavefront, 11.9 ms; a producer / consumer pipeline in persistent workgroups,
    // 19.3 ms — against 10.2 ms per 1 M depth-8 families here: the CU is fed by the number of independent wavefronts, not by lane utilisation.  HISTORY.md §4)
    wave_slices(chain, ps.w2_wpb);
    fp.d_retry_old.reserve((size_t)n_grp * 4);
    const bool ran = n_cur != 0;
    run_slices(chain, false, [&](const Slice& S, FastParams& PS) {
      PS.retry_old = fp.d_retry_old.as<uint32_t>(); PS.n_retry_old = cnt(MISC_N_RETRY_OLD);
      const uint32_t fpb = S.wpb * (uint32_t)S.build;      // families per workgroup
      const dim3 grid((n_cur + fpb - 1) / fpb), block(64 * S.wpb);
      const size_t lds = (size_t)S.wpb * S.bytes;
      if (S.build == 4) FGX_LAUNCH(HIP_KERNEL_NAME(k_simplex_seg<4>), grid, block, lds, s, PS, n_cur);
      else if (S.build == 2) FGX_LAUNCH(HIP_KERNEL_NAME(k_simplex_seg<2>), grid, block, lds, s, PS, n_cur);
      else FGX_LAUNCH(k_simplex_wave2, grid, block, lds, s, PS, n_cur);
    });
    uint32_t n_old = 0;
    if (ran) {   // (no kernel of the chain has run — the split pipeline kept every family —: nothing to read, no synchronisation)
      hip_check(hipMemcpyAsync(&n_old, cnt(MISC_N_RETRY_OLD), 4, hipMemcpyDeviceToHost, s), "D2H");
      sync();
    }
    cur_list = fp.d_retry_old.as<uint32_t>(); n_cur = n_old; out_list = 0;
  }

  // ---- k_family_wave: duplex, CODEC, simplex with --trim, and what k_simplex_wave2 left ----
  void family_wave_stages() {
    std::vector<Slice> st;
    wave_slices(st, ps.fw_wpb);
    run_slices(st, !(duplex || codec), [&](const Slice& S, FastParams& PS) {
      const dim3 grid((n_cur + S.wpb - 1) / S.wpb), block(64 * S.wpb);
      const size_t lds = (size_t)S.wpb * S.bytes;
      if (codec && o.codec_max_reads_per_strand > 0) FGX_LAUNCH(HIP_KERNEL_NAME(k_family_wave<2, 0, 1>), grid, block, lds, s, PS, n_cur);
      else if (codec) FGX_LAUNCH(HIP_KERNEL_NAME(k_family_wave<2>), grid, block, lds, s, PS, n_cur);
      else if (meth_dup && dup_cap) FGX_LAUNCH(HIP_KERNEL_NAME(k_family_wave<1, 1, 1>), grid, block, lds, s, PS, n_cur);
      else if (meth_dup) FGX_LAUNCH(HIP_KERNEL_NAME(k_family_wave<1, 1>), grid, block, lds, s, PS, n_cur);
      else if (dup_cap) FGX_LAUNCH(HIP_KERNEL_NAME(k_family_wave<1, 0, 1>), grid, block, lds, s, PS, n_cur);
      else if (duplex) FGX_LAUNCH(HIP_KERNEL_NAME(k_family_wave<1>), grid, block, lds, s, PS, n_cur);
      else FGX_LAUNCH(HIP_KERNEL_NAME(k_family_wave<0>), grid, block, lds, s, PS, n_cur);
    });
    if (meth_dup) fp.last_meth_device = n_grp;
  }

  // ---- deep duplex molecules (duplex_deep.inc): the list k_family_wave<1> filled — sizes, scan, the record kernel in its two builds, the column kernel.
  //      What they do not take is on the deferred list when they are done.  A batch without such a molecule launches nothing and waits for nothing here ----
  uint32_t n_dup_deep = 0;   // listed molecules (run_slices reads the count); not counted into last_big_families / last_deep_families: those are the simplex path's
  bool dup_deep_ran = false;
  void duplex_deep_molecules() {
    if (!dup_deep || !n_dup_deep) return;
    const uint32_t* const list = fp.d_big.as<uint32_t>();
    const uint32_t n_list = n_dup_deep;
    fp.d_deep_sizes.reserve((size_t)n_list * 8 + 64); fp.d_deep_row0.reserve((size_t)n_list * 8 + 64);
    FGX_LAUNCH(k_deep_sizes, dim3((n_list + 255) / 256), dim3(256), 0, s, list, n_list, d_grp_first, fp.d_deep_sizes.as<uint64_t>());
    scan_u64(fp.d_deep_sizes.as<uint64_t>(), fp.d_deep_row0.as<uint64_t>(), n_list, "scan of the deep molecules' records");
    uint64_t lastr[2] = {0, 0};
    hip_check(hipMemcpyAsync(&lastr[0], fp.d_deep_row0.as<uint64_t>() + (n_list - 1), 8, hipMemcpyDeviceToHost, s), "D2H");
    hip_check(hipMemcpyAsync(&lastr[1], fp.d_deep_sizes.as<uint64_t>() + (n_list - 1), 8, hipMemcpyDeviceToHost, s), "D2H");
    sync();
    const uint64_t n_rows = lastr[0] + lastr[1];
    if (n_rows > (uint64_t)n_rec) throw std::runtime_error("device pipeline: " + std::to_string(n_rows) + " rows for the deep duplex kernels, more than the batch has records");
    fp.d_deep_rows.reserve((size_t)n_rows * sizeof(DeepRow) + 64); fp.d_deep_fams.reserve((size_t)n_list * sizeof(DuplexDeepMol) + 64);
    hip_check(hipMemsetAsync(cnt(MISC_N_DEEP), 0, 8, s), "memset");   // (both halves of the word: decided molecules, of which capped)
    DuplexDeepParams DP;
    DP.list = list; DP.n_list = n_list; DP.row0 = fp.d_deep_row0.as<uint64_t>();
    DP.rows = fp.d_deep_rows.as<DeepRow>(); DP.mols = fp.d_deep_fams.as<DuplexDeepMol>(); DP.n_done = cnt(MISC_N_DEEP);
    DP.rows_walk = nullptr;
    if (dup_deep_cap) {   // the scoring rows of capped sets in walk order: a set's copies lie where its rows lie, so the array is as long as `rows` — only a caller with a cap pays for it
      fp.d_deep_walk.reserve((size_t)n_rows * sizeof(DeepRow) + 64);
      DP.rows_walk = fp.d_deep_walk.as<DeepRow>();
    }
    FastParams PD = P;
    PD.group_list = nullptr;
    // (both builds over the whole list: a workgroup whose molecule is the other build's returns at once)
    // (FGX_DEEP_CLIPS=1: the clip-taking builds of the record kernel in place of the others; the column kernels are the same)
    if (dup_deep_cap) {
      if (sw.deep_clips) {
        FGX_LAUNCH(HIP_KERNEL_NAME(k_duplex_deep_parse<128, 128, 1, 1>), dim3(n_list), dim3(128), 0, s, PD, DP);
        FGX_LAUNCH(HIP_KERNEL_NAME(k_duplex_deep_parse<256, DEEP_MAX, 1, 1>), dim3(n_list), dim3(256), 0, s, PD, DP);
      } else {
        FGX_LAUNCH(HIP_KERNEL_NAME(k_duplex_deep_parse<128, 128, 1>), dim3(n_list), dim3(128), 0, s, PD, DP);
        FGX_LAUNCH(HIP_KERNEL_NAME(k_duplex_deep_parse<256, DEEP_MAX, 1>), dim3(n_list), dim3(256), 0, s, PD, DP);
      }
      FGX_LAUNCH(HIP_KERNEL_NAME(k_duplex_deep_cols<1>), dim3((n_list + 3) / 4), dim3(256), 0, s, PD, DP);
    } else {
      if (sw.deep_clips) {
        FGX_LAUNCH(HIP_KERNEL_NAME(k_duplex_deep_parse<128, 128, 0, 1>), dim3(n_list), dim3(128), 0, s, PD, DP);
        FGX_LAUNCH(HIP_KERNEL_NAME(k_duplex_deep_parse<256, DEEP_MAX, 0, 1>), dim3(n_list), dim3(256), 0, s, PD, DP);
      } else {
        FGX_LAUNCH(HIP_KERNEL_NAME(k_duplex_deep_parse<128, 128>), dim3(n_list), dim3(128), 0, s, PD, DP);
        FGX_LAUNCH(HIP_KERNEL_NAME(k_duplex_deep_parse<256, DEEP_MAX>), dim3(n_list), dim3(256), 0, s, PD, DP);
      }
      FGX_LAUNCH(HIP_KERNEL_NAME(k_duplex_deep_cols<0>), dim3((n_list + 3) / 4), dim3(256), 0, s, PD, DP);
    }
    dup_deep_ran = true;   // (the count of decided molecules comes back with the batch's counters)
  }

  // ---- deep CODEC molecules (codec_deep.inc): the list k_family_wave<2> filled (run_slices read its count into n_dup_deep, the one counter of listed deep
  //      molecules) — sizes, scan, the record kernel in its two builds, the column kernel.  What they do not take is on the deferred list when they are done:
  //      from there the canonical second pass or the general path, as before.  A batch without such a molecule launches nothing and waits for nothing here ----
  bool codec_deep_ran = false;
  void codec_deep_molecules() {
    if (!codec_deep || !n_dup_deep) return;
    const uint32_t* const list = fp.d_big.as<uint32_t>();
    const uint32_t n_list = n_dup_deep;
    fp.d_deep_sizes.reserve((size_t)n_list * 8 + 64); fp.d_deep_row0.reserve((size_t)n_list * 8 + 64);
    FGX_LAUNCH(k_deep_sizes, dim3((n_list + 255) / 256), dim3(256), 0, s, list, n_list, d_grp_first, fp.d_deep_sizes.as<uint64_t>());
    scan_u64(fp.d_deep_sizes.as<uint64_t>(), fp.d_deep_row0.as<uint64_t>(), n_list, "scan of the deep molecules' records");
    uint64_t lastr[2] = {0, 0};
    hip_check(hipMemcpyAsync(&lastr[0], fp.d_deep_row0.as<uint64_t>() + (n_list - 1), 8, hipMemcpyDeviceToHost, s), "D2H");
    hip_check(hipMemcpyAsync(&lastr[1], fp.d_deep_sizes.as<uint64_t>() + (n_list - 1), 8, hipMemcpyDeviceToHost, s), "D2H");
    sync();
    const uint64_t n_rows = lastr[0] + lastr[1];
    if (n_rows > (uint64_t)n_rec) throw std::runtime_error("device pipeline: " + std::to_string(n_rows) + " rows for the deep CODEC kernels, more than the batch has records");
    // a molecule of n records holds at most n rows and at most n RX values (d_deep_walk: the RX list, 8 bytes an entry)
    fp.d_deep_rows.reserve((size_t)n_rows * sizeof(DeepRow) + 64); fp.d_deep_fams.reserve((size_t)n_list * sizeof(CodecDeepMol) + 64);
    fp.d_deep_walk.reserve((size_t)n_rows * 8 + 64);
    hip_check(hipMemsetAsync(cnt(MISC_N_DEEP), 0, 8, s), "memset");   // (both halves of the word: decided molecules, of which capped)
    CodecDeepParams DP;
    DP.list = list; DP.n_list = n_list; DP.row0 = fp.d_deep_row0.as<uint64_t>();
    DP.rows = fp.d_deep_rows.as<DeepRow>(); DP.mols = fp.d_deep_fams.as<CodecDeepMol>(); DP.umi = fp.d_deep_walk.as<unsigned long long>(); DP.n_done = cnt(MISC_N_DEEP);
    FastParams PD = P;
    PD.group_list = nullptr;
    // (both builds over the whole list: a workgroup whose molecule is the other build's returns at once; the CAP builds for a caller with a cap, as k_family_wave<2, 0, 1>)
    if (o.codec_max_reads_per_strand > 0) {
      FGX_LAUNCH(HIP_KERNEL_NAME(k_codec_deep_parse<128, 128, 1>), dim3(n_list), dim3(128), 0, s, PD, DP);
      FGX_LAUNCH(HIP_KERNEL_NAME(k_codec_deep_parse<256, 256, 1>), dim3(n_list), dim3(256), 0, s, PD, DP);
    } else {
      FGX_LAUNCH(HIP_KERNEL_NAME(k_codec_deep_parse<128, 128>), dim3(n_list), dim3(128), 0, s, PD, DP);
      FGX_LAUNCH(HIP_KERNEL_NAME(k_codec_deep_parse<256, 256>), dim3(n_list), dim3(256), 0, s, PD, DP);
    }
    FGX_LAUNCH(k_codec_deep_cols, dim3((n_list + 3) / 4), dim3(256), 0, s, PD, DP);
    codec_deep_ran = true;   // (the counts of decided molecules come back with the batch's counters)
  }

  // ---- deep families: k_deep_parse + k_deep_cols (simplex_deep.inc) take the big list; what is outside their shape goes on to k_family ----
  // One pass of the streaming kernels over a family list; returns how many families it handed on (to `out`).
  // `size_class`: 0 = the wavefront-sized build of the record kernel (families of up to 64 records), 1 = two wavefronts (up to 128), 2 = four (up to DEEP_MAX),
  // 3 = four, up to DEEP_CAP_MAX records (--max-reads: what the cap leaves of such a family fits an end's 255 reads)
  uint32_t deep_pass(const uint32_t* list, uint32_t n_list, int size_class, uint32_t* out) {
    fp.d_deep_sizes.reserve((size_t)n_list * 8 + 64); fp.d_deep_row0.reserve((size_t)n_list * 8 + 64);
    FGX_LAUNCH(k_deep_sizes, dim3((n_list + 255) / 256), dim3(256), 0, s, list, n_list, d_grp_first, fp.d_deep_sizes.as<uint64_t>());
    scan_u64(fp.d_deep_sizes.as<uint64_t>(), fp.d_deep_row0.as<uint64_t>(), n_list, "scan of the deep families' records");
    uint64_t lastr[2] = {0, 0};
    hip_check(hipMemcpyAsync(&lastr[0], fp.d_deep_row0.as<uint64_t>() + (n_list - 1), 8, hipMemcpyDeviceToHost, s), "D2H");
    hip_check(hipMemcpyAsync(&lastr[1], fp.d_deep_sizes.as<uint64_t>() + (n_list - 1), 8, hipMemcpyDeviceToHost, s), "D2H");
    sync();
    const uint64_t n_rows = lastr[0] + lastr[1];
    if (n_rows > (uint64_t)n_rec) throw std::runtime_error("device pipeline: " + std::to_string(n_rows) + " rows for the streaming kernels, more than the batch has records");
    fp.d_deep_rows.reserve((size_t)n_rows * sizeof(DeepRow) + 64); fp.d_deep_fams.reserve((size_t)n_list * sizeof(DeepFam) + 64);
    hip_check(hipMemsetAsync(cnt(MISC_N_DEEP), 0, 4, s), "memset");
    DeepParams DP;
    DP.list = list; DP.n_list = n_list; DP.row0 = fp.d_deep_row0.as<uint64_t>();
    DP.rows = fp.d_deep_rows.as<DeepRow>(); DP.fams = fp.d_deep_fams.as<DeepFam>(); DP.out_list = out; DP.n_out = cnt(MISC_N_DEEP);
    FastParams PD = P;
    PD.group_list = nullptr;
    // (methylation-aware mode: the clip-taking build of the record kernel, in every size class it runs; FGX_DEEP_CLIPS=1: the same builds in the plain mode's classes)
    const bool clips = !meth_dev && sw.deep_clips;
    if (clips && size_class == 1) FGX_LAUNCH(HIP_KERNEL_NAME(k_deep_parse<128, 128, 1>), dim3(n_list), dim3(128), 0, s, PD, DP);
    else if (clips && size_class == 2) FGX_LAUNCH(HIP_KERNEL_NAME(k_deep_parse<256, DEEP_MAX, 1>), dim3(n_list), dim3(256), 0, s, PD, DP);
    else if (clips && size_class == 3) FGX_LAUNCH(HIP_KERNEL_NAME(k_deep_parse<256, DEEP_CAP_MAX, 1>), dim3(n_list), dim3(256), 0, s, PD, DP);
    else if (meth_dev && size_class == 0) FGX_LAUNCH(HIP_KERNEL_NAME(k_deep_parse<64, 64, 1>), dim3(n_list), dim3(64), 0, s, PD, DP);
    else if (meth_dev && size_class == 2) FGX_LAUNCH(HIP_KERNEL_NAME(k_deep_parse<256, DEEP_MAX, 1>), dim3(n_list), dim3(256), 0, s, PD, DP);
    else if (meth_dev && size_class == 3) FGX_LAUNCH(HIP_KERNEL_NAME(k_deep_parse<256, DEEP_CAP_MAX, 1>), dim3(n_list), dim3(256), 0, s, PD, DP);
    else if (size_class == 0) FGX_LAUNCH(HIP_KERNEL_NAME(k_deep_parse<64, 64>), dim3(n_list), dim3(64), 0, s, PD, DP);
    else if (size_class == 1) FGX_LAUNCH(HIP_KERNEL_NAME(k_deep_parse<128, 128>), dim3(n_list), dim3(128), 0, s, PD, DP);
    else if (size_class == 2) FGX_LAUNCH(HIP_KERNEL_NAME(k_deep_parse<256, DEEP_MAX>), dim3(n_list), dim3(256), 0, s, PD, DP);
    else FGX_LAUNCH(HIP_KERNEL_NAME(k_deep_parse<256, DEEP_CAP_MAX>), dim3(n_list), dim3(256), 0, s, PD, DP);
    if (meth_dev) FGX_LAUNCH(HIP_KERNEL_NAME(k_deep_cols<1>), dim3((n_list + 3) / 4), dim3(256), 0, s, PD, DP);
    else FGX_LAUNCH(HIP_KERNEL_NAME(k_deep_cols<0>), dim3((n_list + 3) / 4), dim3(256), 0, s, PD, DP);
    uint32_t n_left = 0;
    hip_check(hipMemcpyAsync(&n_left, cnt(MISC_N_DEEP), 4, hipMemcpyDeviceToHost, s), "D2H");
    sync();
    return n_left;
  }
  // One pass of the wide kernels (simplex_wide.inc) over what the streaming kernels left; returns how many families it handed on (to `out`).
  uint32_t wide_pass(const uint32_t* list, uint32_t n_list, uint32_t* out) {
    fp.d_deep_sizes.reserve((size_t)n_list * 8 + 64); fp.d_deep_row0.reserve((size_t)n_list * 8 + 64);
    hip_check(hipMemsetAsync(cnt(MISC_N_DEEP), 0, 4, s), "memset");   // (first: the largest family; then, cleared again, the families handed on)
    FGX_LAUNCH(k_wide_sizes, dim3((n_list + 255) / 256), dim3(256), 0, s, list, n_list, d_grp_first, fp.d_deep_sizes.as<uint64_t>(), cnt(MISC_N_DEEP));
    scan_u64(fp.d_deep_sizes.as<uint64_t>(), fp.d_deep_row0.as<uint64_t>(), n_list, "scan of the wide families' records");
    uint64_t lastr[2] = {0, 0};
    uint32_t n_max = 0;
    hip_check(hipMemcpyAsync(&n_max, cnt(MISC_N_DEEP), 4, hipMemcpyDeviceToHost, s), "D2H");
    hip_check(hipMemcpyAsync(&lastr[0], fp.d_deep_row0.as<uint64_t>() + (n_list - 1), 8, hipMemcpyDeviceToHost, s), "D2H");
    hip_check(hipMemcpyAsync(&lastr[1], fp.d_deep_sizes.as<uint64_t>() + (n_list - 1), 8, hipMemcpyDeviceToHost, s), "D2H");
    sync();
    const uint64_t n_rows = lastr[0] + lastr[1];
    if (n_rows > (uint64_t)n_rec) throw std::runtime_error("device pipeline: " + std::to_string(n_rows) + " rows for the wide kernels, more than the batch has records");
    WideParams W;
    memset(&W, 0, sizeof(W));
    W.n_rows = (n_rows + 7) & ~7ull;
    W.lds_recs = std::min<uint32_t>(WIDE_MAX, (n_max + 63u) & ~63u);
    if (W.lds_recs == 0) W.lds_recs = 64;
    fp.d_deep_rows.reserve((size_t)n_rows * sizeof(DeepRow) + 64); fp.d_deep_fams.reserve((size_t)n_list * sizeof(DeepFam) + 64);
    fp.d_wide_scratch.reserve((size_t)W.n_rows * WIDE_REC_BYTES + 64);
    fp.d_wide_pass.reserve((size_t)n_list * 8 + 64); fp.d_wide_pass0.reserve((size_t)n_list * 8 + 64);
    hip_check(hipMemsetAsync(cnt(MISC_N_DEEP), 0, 4, s), "memset");
    hip_check(hipMemsetAsync(fp.d_wide_pass.p, 0, (size_t)n_list * 8, s), "memset");
    W.list = list; W.n_list = n_list; W.row0 = fp.d_deep_row0.as<uint64_t>();
    W.scratch = fp.d_wide_scratch.as<uint8_t>();
    W.rows = fp.d_deep_rows.as<DeepRow>(); W.fams = fp.d_deep_fams.as<DeepFam>(); W.out_list = out; W.n_out = cnt(MISC_N_DEEP);
    W.passes = fp.d_wide_pass.as<uint64_t>(); W.pass0 = fp.d_wide_pass0.as<uint64_t>();
    FastParams PD = P;
    PD.group_list = nullptr;
    const uint32_t lds = W.lds_recs * WIDE_LDS_PER_REC;
    FGX_LDS_ATTR((int)WIDE_LDS_BYTES, k_wide_parse);
    FGX_LAUNCH(k_wide_parse, dim3(n_list), dim3(WIDE_NT), lds, s, PD, W);
    scan_u64(fp.d_wide_pass.as<uint64_t>(), fp.d_wide_pass0.as<uint64_t>(), n_list, "scan of the wide families' passes");
    uint64_t lastp[2] = {0, 0};
    uint32_t n_left = 0;
    hip_check(hipMemcpyAsync(&lastp[0], fp.d_wide_pass0.as<uint64_t>() + (n_list - 1), 8, hipMemcpyDeviceToHost, s), "D2H");
    hip_check(hipMemcpyAsync(&lastp[1], fp.d_wide_pass.as<uint64_t>() + (n_list - 1), 8, hipMemcpyDeviceToHost, s), "D2H");
    hip_check(hipMemcpyAsync(&n_left, cnt(MISC_N_DEEP), 4, hipMemcpyDeviceToHost, s), "D2H");
    sync();
    const uint64_t n_items = lastp[0] + lastp[1];
    // (a taken family has at most two ends of at most 65 535 columns: 2 048 passes)
    if (n_items > (uint64_t)n_list * 2048ull) throw std::runtime_error("device pipeline: " + std::to_string(n_items) + " column passes for " + std::to_string(n_list) + " wide families");
    W.n_items = (uint32_t)n_items;
    fp.d_wide_depth.reserve((size_t)n_items * sizeof(uint2) + 64);
    W.item_depth = fp.d_wide_depth.as<uint2>();
    if (n_items) FGX_LAUNCH(k_wide_cols, dim3((W.n_items + 3) / 4), dim3(256), 0, s, PD, W);
    FGX_LAUNCH(k_wide_finish, dim3((n_list + 3) / 4), dim3(256), 0, s, PD, W);
    return n_left;
  }
  void deep_families() {
    if (!duplex && !codec) {
      if (split_counts_seen && fp.last_routed == 0) n_big = h_big_seen;   // (no kernel after the split stages has run: what their last synchronisation read is final)
      else {
        hip_check(hipMemcpyAsync(&n_big, cnt(MISC_N_BIG), 4, hipMemcpyDeviceToHost, s), "D2H");
        sync();
      }
    }
    if (meth_dev) {
      fp.d_big.reserve((size_t)n_grp * 4);
      FGX_LAUNCH(k_iota, dim3((n_grp + 255) / 256), dim3(256), 0, s, fp.d_big.as<uint32_t>(), n_grp);
      n_big = n_grp;
    }
    fp.last_big_families = n_big;
    big_list = fp.d_big.as<uint32_t>();
    if (!(n_big && (sw.deep || meth_dev) && !o.trim)) return;
    P.s2_image = table_image<S2Image>(fp.d_s2img, build_s2_image, "H2D s2 image");   // (the column kernel's LDS tables: the split pipeline's image)
    fp.d_deep_out.reserve((size_t)n_big * 4 + 64);
    // Methylation-aware mode, every family: the wavefront-sized build of the record kernel first; what neither build takes is on the deferred list (the
    // general path knows the mode).  Else (round 6) two wavefronts per family first: a family of 65 .. 128 records — every deep family of a 2 .. 50-pair
    // long tail — kept a quarter to a half of the 256 threads of the large build busy in the record kernel.  What has more records goes on to the large build.
    const uint32_t n_more = deep_pass(fp.d_big.as<uint32_t>(), n_big, meth_dev ? 0 : 1, fp.d_deep_out.as<uint32_t>());
    uint32_t n_left = 0;
    big_list = fp.d_deep_out.as<uint32_t>();
    if (n_more) {
      fp.d_deep_out2.reserve((size_t)n_more * 4 + 64);
      n_left = deep_pass(fp.d_deep_out.as<uint32_t>(), n_more, 2, fp.d_deep_out2.as<uint32_t>());
      big_list = fp.d_deep_out2.as<uint32_t>();
      // --max-reads: a family of DEEP_MAX + 1 .. DEEP_CAP_MAX records fits the kernels once the cap has cut its ends; the large build handed those on
      // (with what is not the kernels' shape, which the next build passes through)
      if (n_left && P.max_reads >= 0) {
        n_left = deep_pass(fp.d_deep_out2.as<uint32_t>(), n_left, 3, fp.d_deep_out.as<uint32_t>());   // (the first pass's list has been read: its room again)
        big_list = fp.d_deep_out.as<uint32_t>();
      }
    }
    fp.last_deep_families = meth_dev ? n_big : n_big - n_left;
    // FGX_DEEP_WIDE=1: what those builds left — more records than they hold, an end of more than 255 reads — through the wide kernels; the rest goes on
    if (sw.deep_wide && n_left && !meth_dev && !duplex && !codec) {
      const bool in_out2 = big_list == fp.d_deep_out2.as<uint32_t>();
      DevBuf& ob = in_out2 ? fp.d_deep_out : fp.d_deep_out2;
      ob.reserve((size_t)n_left * 4 + 64);
      const uint32_t* const in_list = in_out2 ? fp.d_deep_out2.as<uint32_t>() : fp.d_deep_out.as<uint32_t>();   // (reserve may have moved the other buffer, not this one)
      const uint32_t n_after = wide_pass(in_list, n_left, ob.as<uint32_t>());
      fp.last_wide_families = n_left - n_after;
      n_left = n_after;
      big_list = ob.as<uint32_t>();
    }
    if (meth_dev) fp.last_meth_device = n_grp;
    n_big = meth_dev ? 0u : n_left;   // (what is not the kernels' shape: k_family)
  }

  // ---- k_family, one workgroup per family: more bytes than the largest slice (what the chain left), then more than 64 records (what the
  //      streaming kernels left of the list the first kernels filled) ----
  void workgroup_families() {
    for (int pass = 0; pass < 2 && !duplex && !codec; pass++) {
      const uint32_t n = pass == 0 ? n_cur : n_big;
      if (!n) continue;
      FastParams P2 = P;
      P2.group_list = pass == 0 ? cur_list : big_list; P2.retry = nullptr; P2.n_retry = nullptr;
      if (sw.lds_tile_large) { fp.lds_tile_bytes_large = sw.lds_tile_large; P2.lds_tile_bytes = fp.lds_tile_bytes_large; }
      FGX_LDS_ATTR((int)fp.lds_tile_bytes_large, k_family);
      FGX_LAUNCH(k_family, dim3(n), dim3(NT), fp.lds_tile_bytes_large, s, P2);
    }
  }

  // ---- k_call_full: the dense pass over the append lists.  RUN_AGAIN_LARGER_POOL: every list was full, the batch again with twice the room ----
  int call_full() {
    std::vector<uint32_t> counts(N_LISTS);
    hip_check(hipMemcpyAsync(counts.data(), fp.d_full_count.p, (size_t)N_LISTS * 4, hipMemcpyDeviceToHost, s), "D2H");
    sync();
    uint32_t mx = 0, mn = 0xFFFFFFFFu;
    for (uint32_t v : counts) { uint32_t vv = v < full_cap ? v : full_cap; mx = vv > mx ? vv : mx; mn = v < mn ? v : mn; n_full += vv; }
    if (mn >= full_cap && fp.pool_div > 1) {
      // every list is full: some family found no room (and was deferred).  Twice the room, if the device has it, and the batch again.
      size_t free_b = 0, total_b = 0;
      (void)hipMemGetInfo(&free_b, &total_b);
      const uint64_t want = (col_cap / (fp.pool_div / 2) + (uint64_t)N_LISTS * fp.pool_slack) * sizeof(FullItem);
      if (want < (uint64_t)free_b + (uint64_t)fp.d_full_items.cap) {
        fp.pool_div /= 2;
        if (ps.verbose) fprintf(stderr, "[fgx] call_full pool exhausted: the batch again with 1/%u of the column bound\n", fp.pool_div);
        return FastPath::RUN_AGAIN_LARGER_POOL;
      }
    }
    if (mx) {
      FullParams F;
      memset(&F, 0, sizeof(F));
      F.items = fp.d_full_items.as<FullItem>(); F.count = fp.d_full_count.as<uint32_t>(); F.cap = full_cap;
      F.T = P.T; F.TU = P.TU; F.min_reads = P.min_reads; F.min_cons_bq = P.min_cons_bq;
      F.col_code = P.col_code; F.col_qual = P.col_qual; F.col_err = P.col_err;
      F.col_depth = P.col_depth; F.min_input_bq = P.min_input_bq;
      F.out = P.out; F.slot_desc = P.slot_desc; F.slot_err = P.slot_err; F.rg_len = P.rg_len; F.per_base_tags = P.per_base_tags;
      F.rx_base = fp.d_ends.as<char>() + (duplex ? offsetof(DuplexDesc, rx) : codec ? offsetof(CodecDesc, rx) : offsetof(EndDesc, rx));
      F.rx_stride = duplex ? sizeof(DuplexDesc) : codec ? sizeof(CodecDesc) : sizeof(EndDesc);
      if (full_results) { F.res = full_res(); F.flag = P.full_flag; F.n_flag = n_grp; }
      F.stats = P.full_stats;
      FGX_LAUNCH(k_call_full, dim3((mx + 255) / 256, N_LISTS), dim3(256), 0, s, F);
    }
    // the methylation tags' share of the record sizes: the consensus bases are final now
    if (meth_dev) FGX_LAUNCH(k_meth_sizes, dim3((n_slots + 3) / 4), dim3(256), 0, s, P, n_slots, fp.d_mslot.as<MethSlot>());
    if (meth_dup) FGX_LAUNCH(k_duplex_meth_sizes, dim3((n_slots + 3) / 4), dim3(256), 0, s, P, n_slots, fp.d_mslot.as<DuplexMethSlot>());
    return 0;
  }

  // ---- direct records: cE of the records whose columns had errors; did every prediction hold; is there anything to merge? ----
  int check_direct() {
    FGX_LAUNCH(k_fix_ce, dim3((n_slots + 255) / 256), dim3(256), 0, s, fp.d_slot_desc.as<SlotDesc>(), fp.d_slot_err.as<uint32_t>(), n_slots, fp.d_out.as<uint8_t>(), P.rg_len);
    unsigned long long h_flags = 0, h_def = 0, h_route = 0;
    hip_check(hipMemcpyAsync(&h_flags, misc + MISC_DIR_FLAGS, 8, hipMemcpyDeviceToHost, s), "D2H");
    hip_check(hipMemcpyAsync(&h_def, misc + MISC_N_DEFERRED, 8, hipMemcpyDeviceToHost, s), "D2H");
    hip_check(hipMemcpyAsync(&h_route, misc + MISC_N_ROUTE, 8, hipMemcpyDeviceToHost, s), "D2H");
    hip_check(hipMemcpyAsync(&dir_total, fp.d_dir_base.as<uint64_t>() + fp.dir_chunks_run, 8, hipMemcpyDeviceToHost, s), "D2H");
    sync();
    if ((uint32_t)h_flags != 0) {          // a family's records are not what k_split_parse predicted: nothing of the batch can be trusted to be in place
      fprintf(stderr, "[fgx] direct records: %u families differ in size from the prediction; this caller goes back to the column scratch (please report)\n", (uint32_t)h_flags);
      fp.direct_off = true;
      return FastPath::RUN_AGAIN_LARGER_POOL;
    }
    if ((uint32_t)(h_flags >> 32) != 0) {  // more record bytes than the first estimate of the room: the exact amount is known now
      fp.dir_cap_min = dir_total + dir_total / 16 + 4096;
      if (ps.verbose) fprintf(stderr, "[fgx] direct records: the batch needs %llu bytes of output, %llu were at hand: again\n", (unsigned long long)dir_total, (unsigned long long)dir_cap);
      return FastPath::RUN_AGAIN_LARGER_POOL;
    }
    dir_routed = (uint32_t)h_route;
    dir_pure = dir_routed == 0 && (uint32_t)h_def == 0;
    fp.last_direct = dir_pure ? 1 : 2;
    if (ps.verbose) fprintf(stderr, "[fgx] direct records: %llu bytes in place, %u families left the split pipeline, %u deferred\n", (unsigned long long)dir_total, dir_routed, (uint32_t)h_def);
    return 0;
  }

  // ---- where the records go: the scan of their sizes (its last element is the total: d_sizes[n_slots] is 0), the output buffer ----
  void place_records() {
    hip_check(hipEventRecord(fp.ev[1], s), "event");
    out_len = dir_total;
    out_ptr = fp.d_out.as<uint8_t>();
    if (dir_pure) return;
    scan_u64(fp.d_sizes.as<uint64_t>(), fp.d_offsets.as<uint64_t>(), n_slots + 1, "scan");
    uint64_t out_total = 0;
    hip_check(hipMemcpyAsync(&out_total, fp.d_offsets.as<uint64_t>() + n_slots, 8, hipMemcpyDeviceToHost, s), "D2H");
    sync();
    out_len = out_total;
    if (out_len > (1ull << 40)) throw std::runtime_error("device pipeline: the scan of the record sizes gives " + std::to_string(out_len) + " bytes of output (a record size is corrupt)");
    if (direct) { fp.d_out2.reserve(out_len + 16); out_ptr = fp.d_out2.as<uint8_t>(); }   // the merged stream: d_out holds the directly written records
    else { fp.d_out.reserve(out_len + 16); out_ptr = fp.d_out.as<uint8_t>(); }
  }

  // what the three record writers' parameters share
  template <class EP, class Desc> void emit_params(EP& E, const Desc* ends, uint8_t* out) const {
    memset(&E, 0, sizeof(E));
    E.blob = d_blob; E.rec_off = d_rec_off; E.ends = ends; E.out_off = fp.d_offsets.as<uint64_t>(); E.out = out;
    E.slot_end = n_slots;
    E.col_code = P.col_code; E.col_qual = P.col_qual; E.col_err = P.col_err;
    E.prefix = fp.d_strings.as<char>(); E.prefix_len = P.prefix_len; E.rg = fp.d_strings.as<char>() + P.prefix_len; E.rg_len = P.rg_len;
    E.per_base_tags = P.per_base_tags; E.cell0 = P.cell0; E.cell1 = P.cell1;
  }
  // ---- the record writers, the counters, the result ----
  // (round 6) duplex / CODEC: the per-field record writer (k_emit_duplex / k_emit_codec: any length, any tag size) used to run over EVERY slot behind the fast
  // writer and find nothing to do (0.97 / 0.33 ms per step of wavefronts that load a descriptor and leave); a counting kernel (a thread per slot) now says
  // how many records the fast writer refuses, and the per-field kernel is launched — after the batch's last synchronisation — only when there are any
  void write_records() {
    hip_check(hipEventRecord(fp.ev[2], s), "event");
    const dim3 per_slot((n_slots + 255) / 256), wave_per_slot((n_slots + 3) / 4), wave_per_family((n_grp + 3) / 4);
    DuplexEmitParams DE;
    CodecEmitParams CE;
    if (codec) {
      emit_params(CE, fp.d_ends.as<CodecDesc>(), fp.d_out.as<uint8_t>());
      CE.col_depth = P.col_depth;
      CE.has_outer = o.codec_has_outer_bases_qual; CE.outer_qual = o.codec_outer_bases_qual; CE.outer_len = o.codec_outer_bases_length;
      CE.has_ss = o.codec_has_single_strand_qual; CE.ss_qual = o.codec_single_strand_qual;
      CE.stats = fp.d_statslots.as<unsigned long long>();
      CE.n_slow = cnt(MISC_N_SLOW);
      FGX_LAUNCH(HIP_KERNEL_NAME(k_count_slow<CodecDesc>), per_slot, dim3(256), 0, s, CE.ends, 0u, n_slots, CE.prefix_len, CE.rg_len, CE.n_slow);
      FGX_LAUNCH(k_emit_codec_fast, wave_per_slot, dim3(256), 0, s, CE);
    } else if (duplex) {
      emit_params(DE, fp.d_ends.as<DuplexDesc>(), fp.d_out.as<uint8_t>());
      DE.col_obs = P.col_obs;
      DE.n_slow = cnt(MISC_N_SLOW);
      DE.meth_flag = P.meth_flag;
      DE.col_obs_all = P.col_obs_all;
      FGX_LAUNCH(HIP_KERNEL_NAME(k_count_slow<DuplexDesc>), per_slot, dim3(256), 0, s, DE.ends, 0u, n_slots, DE.prefix_len, DE.rg_len, DE.n_slow);
      if (meth_dup && dup_cap) FGX_LAUNCH(HIP_KERNEL_NAME(k_emit_duplex_fast<1, 1>), wave_per_slot, dim3(256), 0, s, DE);
      else if (meth_dup) FGX_LAUNCH(HIP_KERNEL_NAME(k_emit_duplex_fast<1>), wave_per_slot, dim3(256), 0, s, DE);
      else if (dup_cap) FGX_LAUNCH(HIP_KERNEL_NAME(k_emit_duplex_fast<0, 1>), wave_per_slot, dim3(256), 0, s, DE);
      else FGX_LAUNCH(HIP_KERNEL_NAME(k_emit_duplex_fast<0>), wave_per_slot, dim3(256), 0, s, DE);
    } else if (!direct || !dir_pure) {
      EmitParams E;
      emit_params(E, fp.d_ends.as<EndDesc>(), out_ptr);
      E.col_depth = P.col_depth; E.tag0 = P.tag0; E.tag1 = P.tag1;
      if (full_results) { E.full_res = full_res(); E.full_flag = P.full_flag; }
      if (!direct) FGX_LAUNCH(k_emit, wave_per_family, dim3(256), 0, s, E);   // one wavefront per family (slots 3g .. 3g + 2)
      else {
        // the merge: the families that left the split pipeline are written by k_emit from their descriptors, the directly written ones move
        // to their place in the final stream
        if (dir_routed) {
          E.fam_list = fp.d_route.as<uint32_t>(); E.n_fam = dir_routed;
          FGX_LAUNCH(k_emit, dim3((dir_routed + 3) / 4), dim3(256), 0, s, E);
        }
        FGX_LAUNCH(k_dir_copy, wave_per_family, dim3(256), 0, s, fp.d_split_out.as<SplitOut>(), fp.d_dir_off.as<uint64_t>(), fp.d_offsets.as<uint64_t>(),
                   fp.d_sizes.as<uint64_t>(), fp.d_out.as<uint8_t>(), out_ptr, n_grp);
      }
    }
    if (meth_dev) FGX_LAUNCH(k_meth_tail, wave_per_slot, dim3(256), 0, s, P, n_slots, fp.d_mslot.as<MethSlot>(), fp.d_offsets.as<uint64_t>(), out_ptr);
    if (meth_dup) FGX_LAUNCH(k_duplex_meth_tail, wave_per_slot, dim3(256), 0, s, P, n_slots, fp.d_mslot.as<DuplexMethSlot>(), fp.d_offsets.as<uint64_t>(), out_ptr);
    hip_check(hipEventRecord(fp.ev[3], s), "event");
    hip_check(hipEventRecord(c->ev1, s), "event");
    unsigned long long h_misc[MISC_READ_BACK];
    auto read_counters = [&] {
      FGX_LAUNCH(k_reduce_stats, dim3(1), dim3(64), 0, s, fp.d_statslots.as<unsigned long long>(), misc, (const unsigned long long*)P.full_stats, (uint32_t)MISC_FULL_RESULTS);
      hip_check(hipMemcpyAsync(h_misc, misc, sizeof(h_misc), hipMemcpyDeviceToHost, s), "D2H");
      sync();
    };
    read_counters();
    if ((duplex || codec) && (uint32_t)h_misc[MISC_N_SLOW] != 0) {     // records the fast writer left: the per-field kernel, then the counters again (the CODEC writer counts bases)
      if (codec) FGX_LAUNCH(k_emit_codec, wave_per_slot, dim3(256), 0, s, CE);
      else if (meth_dup && dup_cap) FGX_LAUNCH(HIP_KERNEL_NAME(k_emit_duplex<1, 1>), wave_per_slot, dim3(256), 0, s, DE);
      else if (meth_dup) FGX_LAUNCH(HIP_KERNEL_NAME(k_emit_duplex<1>), wave_per_slot, dim3(256), 0, s, DE);
      else if (dup_cap) FGX_LAUNCH(HIP_KERNEL_NAME(k_emit_duplex<0, 1>), wave_per_slot, dim3(256), 0, s, DE);
      else FGX_LAUNCH(HIP_KERNEL_NAME(k_emit_duplex<0>), wave_per_slot, dim3(256), 0, s, DE);
      read_counters();
    }
    float ms = 0, msf = 0, mse = 0;
    hip_check(hipEventElapsedTime(&ms, c->ev0, c->ev1), "elapsed");
    hip_check(hipEventElapsedTime(&msf, fp.ev[0], fp.ev[1]), "elapsed");
    hip_check(hipEventElapsedTime(&mse, fp.ev[2], fp.ev[3]), "elapsed");
    res->d_out = out_ptr;
    res->out_len = out_len;
    res->count = h_misc[MISC_STATS + 1];   // every consensus read of a fast-path family is one record
    for (int i = 0; i < FGX_STATS_LEN; i++) res->stats[i] = h_misc[MISC_STATS + i];
    res->n_deferred = (uint32_t)(h_misc[MISC_N_DEFERRED] & 0xFFFFFFFFull);
    fp.last_meth_clipped = (uint32_t)(h_misc[MISC_N_METH_CLIPPED] & 0xFFFFFFFFull);
    if (!fp.canon_second_pass) fp.last_deep_clipped = (uint32_t)(h_misc[MISC_N_METH_CLIPPED] >> 32);   // (the second pass runs no clip build outside the mode)
    if (dup_deep_ran && fp.canon_second_pass) fp.last_deep_indels = (uint32_t)(h_misc[MISC_N_DEEP] & 0xFFFFFFFFull);   // (FGX_DEEP_INDELS=1; fgx_debug_last_duplex_deep stays the first pass's count)
    else if (dup_deep_ran) { fp.last_duplex_deep = (uint32_t)(h_misc[MISC_N_DEEP] & 0xFFFFFFFFull); fp.last_duplex_deep_capped = (uint32_t)(h_misc[MISC_N_DEEP] >> 32); }
    if (codec_deep_ran) { fp.last_codec_deep = (uint32_t)(h_misc[MISC_N_DEEP] & 0xFFFFFFFFull); fp.last_codec_deep_capped = (uint32_t)(h_misc[MISC_N_DEEP] >> 32); }
    res->d_deferred = fp.d_deferred.as<uint32_t>();
    res->d_out_off = fp.d_offsets.as<uint64_t>();
    res->d_slot_size = fp.d_sizes.as<uint64_t>();
    res->n_slots = n_slots;
    res->ms_kernels = ms; res->ms_k_family = msf; res->ms_k_emit = mse;
    fp.last_packed_families = h_misc[MISC_BUILD_FAMILIES]; fp.last_classic_families = h_misc[MISC_BUILD_FAMILIES + 1];
    fp.last_packed_clean = h_misc[MISC_BUILD_FAMILIES + 2]; fp.last_packed_general = h_misc[MISC_BUILD_FAMILIES + 3];
    for (int i = 0; i < FULL_STATS_N; i++) fp.last_full_results[i] = h_misc[MISC_FULL_RESULTS + i];
    for (int i = 0; i < OV_STATS_N; i++) fp.last_packed_overlap[i] = h_misc[MISC_PACKED_OVERLAP + i];
    res->cols_used = h_misc[MISC_COLS_USED];
    res->full_items = n_full;
  }
};

// One batch through the launch chain: the stages in the order they enqueue.  RUN_AGAIN_LARGER_POOL: FastPath::run calls again.
int run_once(FastPath& fp, fgx_caller* c, const uint8_t* d_blob, uint64_t blob_len, const uint64_t* d_rec_off, const uint32_t* d_rec_len, uint32_t n_rec,
             const uint32_t* d_grp_first, uint32_t n_grp, FastResult* res) {
  memset(res, 0, sizeof(*res));
  fp.last_launches = 0; fp.last_host_syncs = 0;
  if (n_grp == 0) return 0;
  static const ProcessSwitches ps{};
  Batch b{fp, c, d_blob, blob_len, d_rec_off, d_rec_len, n_rec, d_grp_first, n_grp, res, ps};
  b.set_up();
  b.parse_first_chunk_early();
  b.bound_columns();
  b.fill_params();
  if (b.use_split) b.split_pipeline();
  if (b.simplex_v2) b.wave2_chain();
  b.family_wave_stages();
  b.duplex_deep_molecules();
  b.codec_deep_molecules();
  b.deep_families();
  b.workgroup_families();
  if (const int rc = b.call_full()) return rc;
  if (b.direct) if (const int rc = b.check_direct()) return rc;
  b.place_records();
  b.write_records();
  return 0;
}

}  // namespace

// The columns whose call needs the log-sum-exp chain wait in append lists for k_call_full.  Their room is a fraction of the column
// bound (1/8: clean libraries need under 1 %); when a batch fills EVERY list — a noisy library: a few per cent of disagreeing bases
// at depth 8 — the batch is run again with twice the room (and the caller keeps the larger fraction for its next batches) instead
// of handing the families that found no room to the host path.
int FastPath::run(fgx_caller* c, const uint8_t* d_blob, uint64_t blob_len, const uint64_t* d_rec_off, const uint32_t* d_rec_len,
                  uint32_t n_rec, const uint32_t* d_grp_first, uint32_t n_grp, FastResult* res) {
  if (!pool_init) {   // (test knobs: a tiny pool makes a small batch exhaust it)
    if (const char* e = getenv("FGX_POOL_DIV")) { const long v = atol(e); if (v >= 1 && v <= (1 << 20)) pool_div = (uint32_t)v; }
    if (const char* e = getenv("FGX_POOL_SLACK")) { const long v = atol(e); if (v >= 1 && v <= 4096) pool_slack = (uint32_t)v; }
    pool_init = true;
  }
  for (;;) {
    const int rc = run_once(*this, c, d_blob, blob_len, d_rec_off, d_rec_len, n_rec, d_grp_first, n_grp, res);
    if (rc != RUN_AGAIN_LARGER_POOL) {
      if (const char* e = fgx_knob("FGX_S2_DEBUG")) if (atoi(e)) {   // (development: the packed pass's counters, cumulative over the process)
        uint32_t h[64];
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpyFromSymbol(h, HIP_SYMBOL(g_s2_dbg), sizeof(h)) == hipSuccess) {
          fprintf(stderr, "[s2 packed] runs tried %u finished %u (columns for k_call_full %u) no room %u shape refused %u", h[0], h[1], h[2], h[3], h[42]);
          fprintf(stderr, "\n");
        }
      }
      return rc;
    }
  }
}

}  // namespace fgx

#if FGX_PHASE_TIMING
extern "C" int fgx_debug_phase_cycles(unsigned long long* out16, int reset) {
  unsigned long long h[64 * 16];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(fgx::g_phase), sizeof(h)) != hipSuccess) return 1;
  for (int i = 0; i < 16; i++) { out16[i] = 0; for (int b = 0; b < 64; b++) out16[i] += h[b * 16 + i]; }
  if (reset) { memset(h, 0, sizeof(h)); if (hipMemcpyToSymbol(HIP_SYMBOL(fgx::g_phase), h, sizeof(h)) != hipSuccess) return 1; }
  return 0;
}
#endif
