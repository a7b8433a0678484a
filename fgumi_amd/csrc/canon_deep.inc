// canon_deep.inc — the canonical form (canon_core.h) of duplex molecules of 65 .. 512 records, a WORKGROUP per molecule (FGX_DEEP_INDELS=1).
//
// k_canon_duplex (canon_device.hip) gives a molecule to one lane: serial scalar code with an O(n^2) name search and a slab of 19 KB.  At 512 records that is tens of
// milliseconds a lane.  Here thread = record and wavefront = pair: k_canon_duplex_deep computes, for every molecule of more than 64 records on the deferred list, the very
// bytes `canon_duplex_molecule<DEEP_MAX_READS>` computes — status, delta, lengths, every byte of every kept record and its 4-byte prefix
// (tests/test_wavemu_deep_indels.py and tests/test_gpu_deep_indels.py compare the two) — in the order of that function:
//   1. record checks (thread = record) and the working copy (wavefront = record, 16-byte pieces); any refusal is a workgroup-uniform exit;
//   2. the strand-orientation collision, per record side, by ballots;
//   3. pairing: per name the LAST record with FIRST and the LAST without it — a name hash as the filter, names verified — then the overlap correction, a wavefront per
//      pair, lane = reference position of a stretch both mates align (the merge of the two CIGARs gives at most 32 such stretches; inside one both query offsets
//      advance with the lane).  SEQ packs two bases a byte: the lane of the EVEN query offset writes the byte with its neighbour's nibble (a shuffle), so no two
//      lanes read-modify-write one byte; the byte that straddles two stretches is written by one lane in each, a wave_sync() apart;
//   4. per record: mate clip (bam::mate_clip on the ops and MC), final length walked back over the corrected copy, the simplified CIGAR — reversed, truncated — built
//      IN PLACE in LDS over the raw ops, packed `len << 4 | kind` (512 x 16 x 4 B = 32 KB);
//   5. the alignment filter per record side: the stable longest-first order as a RANK (each thread counts the reads ahead of its own: <= 512 compares), then at most 16
//      rounds — the next representative is the first read in that order that is a prefix of no representative so far (an LDS minimum), every thread tests its read
//      against it, and joins when the representative precedes it (no early break, as in fgbio); a 17th group is out of scope; best group by size, then simp_cmp, the
//      later group winning ties; then the gates of canon_duplex_molecule (read counts of the survivors, a biting cap, the cell barcode of a dropped first record);
//   6. canon::rewrite_record per thread on its own record, and the prefixes.
// LDS: 41 KB a workgroup (CanonDeepLds), three workgroups of eight wavefronts per CU.  Per-thread state stays in registers; the parsed MC ops (17 dwords) are the
// kernel's only private array.  Only cross-lane operations that tests/wavemu/simt.h maps are used (ballot, shuffle, __syncthreads*, LDS atomics), all under
// workgroup- or wavefront-uniform control flow: the emulator faults otherwise.
//
// Included by fastpath.hip inside namespace fgx (so that the wave emulator compiles it under its lock-step shim).

namespace {

constexpr uint32_t CD_NT = canon::DEEP_MAX_READS;      // 512 threads: thread = record
constexpr uint32_t CD_NONE = 0xFFFFFFFFu;
enum : uint32_t { CD_STRAND = 1u, CD_R2 = 2u, CD_REV = 4u, CD_MEMBER = 8u, CD_NSIMP_SHIFT = 8u };

struct CanonDeepLds {
  uint32_t simp[canon::DEEP_MAX_READS][canon::MAX_OPS];   // raw CIGAR ops, then the simplified CIGAR: len << 4 | kind
  uint32_t key[canon::DEEP_MAX_READS];                    // name hash
  uint32_t final_len[canon::DEEP_MAX_READS];
  uint32_t clip[canon::DEEP_MAX_READS];
  uint16_t info[canon::DEEP_MAX_READS];                   // CD_* bits | n_simp << 8
  uint16_t pair_a[canon::DEEP_MAX_READS / 2], pair_b[canon::DEEP_MAX_READS / 2];   // the FIRST record / the other record of every pair
  uint32_t g_rep[canon::MAX_GROUPS], g_size[canon::MAX_GROUPS];
  uint32_t bad, n_pairs, next, has[2], side_rev[2], first_of, first_kept;
  uint32_t ov[4];
};
static_assert(sizeof(CanonDeepLds) <= 48 * 1024, "k_canon_duplex_deep: three workgroups per CU");

__device__ __forceinline__ bool cd_is_prefix(const uint32_t* a, uint32_t na, const uint32_t* b, uint32_t nb) {   // canon::simp_is_prefix on packed ops
  if (na > nb) return false;
  for (uint32_t i = 0; i < na; i++) {
    if (i + 1 == na) { if ((a[i] & 15u) != (b[i] & 15u) || (a[i] >> 4) > (b[i] >> 4)) return false; }
    else if (a[i] != b[i]) return false;
  }
  return true;
}
__device__ __forceinline__ int cd_cmp(const uint32_t* a, uint32_t na, const uint32_t* b, uint32_t nb) {   // canon::simp_cmp: length, then kind — the packed word's own order
  const uint32_t n = na < nb ? na : nb;
  for (uint32_t i = 0; i < n; i++) if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return na == nb ? 0 : (na < nb ? -1 : 1);
}

// The new nibbles of 64 consecutive query offsets (`x` of lane l = x of lane 0 + l; nc = the lane's new code, 0xFF = none): the lane of an even offset writes the byte
// with the next lane's nibble; lane 0 of an odd offset writes its own low nibble (the high one is not this step's).
__device__ __forceinline__ void cd_put_nibbles(uint8_t* seq, uint32_t x, uint32_t nc, uint32_t lane) {
  const uint32_t up = (uint32_t)__shfl_down((int)nc, 1);
  uint32_t hi = 0xFFu, lo = 0xFFu;
  if (!(x & 1u)) { hi = nc; if (lane < 63u) lo = up; }
  else if (lane == 0) lo = nc;
  if (hi != 0xFFu || lo != 0xFFu) {
    uint32_t b = seq[x >> 1];
    if (hi != 0xFFu) b = (hi << 4) | (b & 0x0Fu);
    if (lo != 0xFFu) b = (b & 0xF0u) | lo;
    seq[x >> 1] = (uint8_t)b;
  }
}

// canon::overlap_pair by one wavefront: every lane walks the two CIGARs (the same scalar work in each), the lanes share the positions of a stretch.
__device__ __forceinline__ void cd_overlap_pair(uint8_t* a, uint32_t an, uint8_t* b, uint32_t bn, uint32_t lane, uint32_t* st) {
  const bam::Rec v1{a, an}, v2{b, bn};
  if ((v1.flags() | v2.flags()) & bam::F_UNMAPPED) return;
  if (v1.ref_id() != v2.ref_id()) return;
  if (v1.pos() < 0 || v2.pos() < 0) return;
  const uint32_t n1 = v1.n_cigar(), n2 = v2.n_cigar();
  auto ref_len = [](const bam::Rec& v, uint32_t n) -> int64_t {      // bam::ref_len_checked0
    int64_t r = 0;
    for (uint32_t i = 0; i < n; i++) { const uint32_t op = v.cigar_op(i); if (bam::op_consumes_ref(op & 0xFu)) { r += (int32_t)(op >> 4); if (r > 2147483647LL) return 0; } }
    return r;
  };
  const int64_t rl1 = ref_len(v1, n1), rl2 = ref_len(v2, n2);
  if (rl1 == 0 || rl2 == 0) return;
  const int64_t s1 = (int64_t)v1.pos() + 1, e1 = (int64_t)v1.pos() + rl1, s2 = (int64_t)v2.pos() + 1, e2 = (int64_t)v2.pos() + rl2;
  const int64_t lo = s1 > s2 ? s1 : s2, hi = e1 < e2 ? e1 : e2;
  uint8_t* const seq1 = a + v1.seq_off();
  uint8_t* const seq2 = b + v2.seq_off();
  uint8_t* const q1 = a + v1.qual_off();
  uint8_t* const q2 = b + v2.qual_off();
  uint32_t i1 = 0, i2 = 0;
  int64_t r1 = s1, r2 = s2, x1 = 0, x2 = 0;        // reference position and query offset at the start of op i1 / i2
  while (i1 < n1 && i2 < n2 && r1 <= hi && r2 <= hi) {
    const uint32_t op1 = v1.cigar_op(i1), t1 = op1 & 0xFu, op2 = v2.cigar_op(i2), t2 = op2 & 0xFu;
    const int64_t l1 = op1 >> 4, l2 = op2 >> 4;
    if (!(t1 == 0 || t1 == 7 || t1 == 8)) { if (t1 == 1 || t1 == 4) x1 += l1; else if (t1 == 2 || t1 == 3) r1 += l1; i1++; continue; }
    if (!(t2 == 0 || t2 == 7 || t2 == 8)) { if (t2 == 1 || t2 == 4) x2 += l2; else if (t2 == 2 || t2 == 3) r2 += l2; i2++; continue; }
    const int64_t end1 = r1 + l1 - 1, end2 = r2 + l2 - 1;
    int64_t s = r1 > r2 ? r1 : r2, e = end1 < end2 ? end1 : end2;
    if (s < lo) s = lo;
    if (e > hi) e = hi;
    for (int64_t base = s; base <= e; base += 64) {
      const int64_t p = base + lane;
      const bool act = p <= e;
      const uint32_t x = (uint32_t)(x1 + (p - r1)), y = (uint32_t)(x2 + (p - r2));
      uint32_t nc = 0xFFu;
      if (act) {
        const uint32_t k1 = ((uint32_t)seq1[x >> 1] >> ((~x & 1u) << 2)) & 15u, k2 = ((uint32_t)seq2[y >> 1] >> ((~y & 1u) << 2)) & 15u;
        if (k1 != 15u && k2 != 15u) {
          st[0]++;
          const uint32_t qa = q1[x], qb = q2[y];
          if (k1 == k2) {
            st[1]++;
            const uint32_t sm = qa + qb, nq = sm < 93u ? sm : 93u;
            q1[x] = (uint8_t)nq; q2[y] = (uint8_t)nq;
            if (nq != qa || nq != qb) st[3]++;
          } else {
            st[2]++;
            uint32_t cq;
            if (qa == qb) { nc = 15u; cq = 2u; }
            else if (qa > qb) { nc = k1; cq = qa - qb > 2u ? qa - qb : 2u; }
            else { nc = k2; cq = qb - qa > 2u ? qb - qa : 2u; }
            q1[x] = (uint8_t)cq; q2[y] = (uint8_t)cq;
            st[3] += 2;
          }
        }
      }
      cd_put_nibbles(seq1, x, nc, lane);
      cd_put_nibbles(seq2, y, nc, lane);
      wave_sync();           // (the byte two stretches share: the next step's lane reads what this step's lane wrote)
    }
    if (end1 <= end2) { r1 += l1; x1 += l1; i1++; } else { r2 += l2; x2 += l2; i2++; }
  }
}

__global__ void __launch_bounds__(CD_NT)
k_canon_duplex_deep(canon::Params P, const uint8_t* __restrict__ blob, const uint64_t* __restrict__ rec_off, const uint32_t* __restrict__ rec_len,
                    const uint32_t* __restrict__ grp_first, const uint32_t* __restrict__ def, uint32_t nd, const uint64_t* __restrict__ first,
                    uint8_t* out, const uint64_t* __restrict__ out_off, uint32_t* out_len, int* status, canon::Delta* delta) {
  __shared__ CanonDeepLds S;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t k = blockIdx.x;
  if (k >= nd) return;
  const uint32_t r0 = grp_first[def[k]], n = grp_first[def[k] + 1] - r0;
  if (n <= 64u) return;                                   // the lane kernel's (uniform; ahead of every barrier)
  rec_off += r0; rec_len += r0; out_off += first[k]; out_len += first[k];
  auto refuse = [&]() {
    if (tid == 0) { status[k] = canon::CANON_OUT_OF_SCOPE; canon::Delta D; D.minority = 0; D.ov[0] = D.ov[1] = D.ov[2] = D.ov[3] = 0; delta[k] = D; }
  };
  if (n > canon::DEEP_MAX_READS || P.trim || P.min_xy > P.min_total || P.min_yx > P.min_xy) { refuse(); return; }
  if (tid == 0) {
    S.bad = 0; S.n_pairs = 0; S.has[0] = S.has[1] = 0; S.side_rev[0] = S.side_rev[1] = 0; S.first_of = S.first_kept = CD_NONE;
    S.ov[0] = S.ov[1] = S.ov[2] = S.ov[3] = 0;
  }
  __syncthreads();

  // ---- 1. record checks (canon_duplex_molecule's first loop), thread = record ----
  const bool mine = tid < n;
  uint32_t info = 0, len = 0;
  if (mine) {
    len = rec_len[tid];
    bool ok = len >= 32;
    if (ok) {
      const bam::Rec v{blob + rec_off[tid], len};
      const uint16_t f = v.flags();
      const uint32_t nc = v.n_cigar(), l = v.l_seq();
      ok = !(v.l_read_name() == 0 || (uint64_t)v.aux_off() > len);
      if (ok && (!(f & bam::F_PAIRED) || (f & (bam::F_UNMAPPED | bam::F_SECONDARY | bam::F_SUPPLEMENTARY)))) ok = false;
      if (ok && ((f & bam::F_FIRST) != 0) == ((f & bam::F_LAST) != 0)) ok = false;
      if (ok && (nc == 0 || nc > canon::MAX_OPS)) ok = false;
      if (ok) {
        uint64_t ql = 0;
        for (uint32_t i = 0; i < nc; i++) { const uint32_t op = v.cigar_op(i); if ((op & 0xFu) > 8u) ok = false; if (bam::op_consumes_query(op & 0xFu)) ql += op >> 4; }
        if (ql != l) ok = false;
      }
      if (ok) {
        const int st = canon::mi_strand(v);
        if (st < 0) ok = false;
        else {
          info = (st ? CD_STRAND : 0u) | ((f & bam::F_LAST) ? CD_R2 : 0u) | ((f & bam::F_REVERSE) ? CD_REV : 0u);
          atomicOr(&S.has[st], 1u);
        }
      }
    }
    if (!ok) atomicOr(&S.bad, 1u);
    S.info[tid] = (uint16_t)info;
  }
  __syncthreads();
  if (S.bad) { refuse(); return; }
  // the working copy, a wavefront per record in 16-byte pieces; a read whose qualities are all 0xFF is refused
  for (uint32_t r = wv; r < n; r += CD_NT / 64u) {
    const uint32_t rl = rec_len[r];
    const uint8_t* const s = blob + rec_off[r];
    uint8_t* const d = out + out_off[r];
    const bam::Rec v{s, rl};
    const uint32_t l = v.l_seq(), qa = v.qual_off(), qe = qa + l;
    bool not_ff = false;
    for (uint32_t o = lane * 16u; o < rl; o += 64u * 16u) {
      if (o + 16u <= rl) {
        uint8_t w[16];
        __builtin_memcpy(w, s + o, 16);
        __builtin_memcpy(d + o, w, 16);
#pragma unroll
        for (uint32_t i = 0; i < 16u; i++) if (o + i >= qa && o + i < qe && w[i] != 0xFFu) not_ff = true;
      } else {
        for (uint32_t i = o; i < rl; i++) { const uint8_t c = s[i]; d[i] = c; if (i >= qa && i < qe && c != 0xFFu) not_ff = true; }
      }
    }
    const bool any = __any(not_ff);
    if (l != 0 && !any && lane == 0) atomicOr(&S.bad, 1u);
  }
  __syncthreads();
  if (S.bad) { refuse(); return; }
  const bool has_a = S.has[0] != 0, has_b = S.has[1] != 0;
  const uint32_t strand = info & CD_STRAND, r2 = (info & CD_R2) ? 1u : 0u;
  const bool rev = (info & CD_REV) != 0;

  // ---- 2. strand-orientation collision: a record side (AB-R1 ++ BA-R2 / AB-R2 ++ BA-R1) holds reads of both orientations ----
#pragma unroll
  for (uint32_t set = 0; set < 2; set++) {
    const bool in_set = mine && (strand == 0 ? r2 == set : r2 != set);
    const unsigned long long bf = __ballot(in_set && rev), bn = __ballot(in_set && !rev);
    if (lane == 0) { if (bf) atomicOr(&S.side_rev[set], 2u); if (bn) atomicOr(&S.side_rev[set], 1u); }
  }
  __syncthreads();
  if (has_a && has_b && (S.side_rev[0] == 3u || S.side_rev[1] == 3u)) { refuse(); return; }

  // ---- 3. the overlap pre-step: the LAST R1 and the LAST R2 of a name, a wavefront per pair ----
  if (P.overlapping && (P.min_yx == 0 || (has_a && has_b))) {
    uint32_t h = 2166136261u, nl = 0;
    const uint8_t* const nm = blob + (mine ? rec_off[tid] : rec_off[0]) + 32;
    if (mine) {
      nl = bam::Rec{nm - 32, len}.name_len();
      for (uint32_t i = 0; i < nl; i++) h = (h ^ nm[i]) * 16777619u;
      S.key[tid] = h;
    }
    __syncthreads();
    if (mine && !r2) {                                     // a FIRST record: the pair's, unless a later one carries the name
      bool later = false;
      uint32_t other = CD_NONE;
      for (uint32_t j = 0; j < n; j++) {
        if (j == tid || S.key[j] != h) continue;
        const bam::Rec vj{blob + rec_off[j], rec_len[j]};
        if (vj.name_len() != nl) continue;
        bool same = true;
        for (uint32_t i = 0; i < nl && same; i++) same = vj.name()[i] == nm[i];
        if (!same) continue;
        if (S.info[j] & CD_R2) other = j; else if (j > tid) later = true;
      }
      if (!later && other != CD_NONE) { const uint32_t p = atomicAdd(&S.n_pairs, 1u); S.pair_a[p] = (uint16_t)tid; S.pair_b[p] = (uint16_t)other; }
    }
    __syncthreads();
    const uint32_t np = S.n_pairs;
    uint32_t st[4] = {0, 0, 0, 0};
    for (uint32_t p = wv; p < np; p += CD_NT / 64u) {
      const uint32_t a = S.pair_a[p], b = S.pair_b[p];
      cd_overlap_pair(out + out_off[a], rec_len[a], out + out_off[b], rec_len[b], lane, st);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) if (st[i]) atomicAdd(&S.ov[i], st[i]);
    __syncthreads();
  }

  // ---- 4. per record: mate clip, final length, simplified CIGAR (in place over the raw ops) ----
  uint32_t clip = 0, fl = 0;
  if (mine) {
    const bam::Rec v{out + out_off[tid], len};
    uint32_t* const sp = S.simp[tid];
    const uint32_t nc = v.n_cigar(), l = v.l_seq();
    for (uint32_t i = 0; i < nc; i++) sp[i] = v.cigar_op(i);
    const uint32_t an = v.len > v.aux_off() ? v.len - v.aux_off() : 0;
    uint32_t mcl = 0, mc_ops[canon::MAX_OPS + 1];
    const int64_t mco = bam::find_z_tag(v.b + v.aux_off(), an, 'M', 'C', &mcl);
    bool overflow = false;
    const uint64_t c = bam::mate_clip(v, sp, nc, mco >= 0 ? v.b + v.aux_off() + mco : nullptr, mcl, mc_ops, canon::MAX_OPS + 1, &overflow);
    if (overflow) atomicOr(&S.bad, 1u);
    else {
      clip = c > l ? l : (uint32_t)c;
      fl = l - clip;
      const uint8_t* const q = v.b + v.qual_off();
      while (fl > 0) {
        const uint32_t s = rev ? l - fl : fl - 1;
        if (v.base_code(s) == 15 || q[s] < P.min_bq) fl--; else break;
      }
      uint32_t nt = 0;                                     // S, H, =, X -> M; adjacent ops merged
      for (uint32_t i = 0; i < nc; i++) {
        const uint32_t t = sp[i] & 0xFu, kk = (t == 4 || t == 5 || t == 7 || t == 8) ? 0u : t, ln = sp[i] >> 4;
        if (nt && (sp[nt - 1] & 0xFu) == kk) { const uint32_t sum = (sp[nt - 1] >> 4) + ln; if (sum >= (1u << 28)) atomicOr(&S.bad, 1u); sp[nt - 1] = (sum << 4) | kk; }
        else { sp[nt] = (ln << 4) | kk; nt++; }
      }
      if (rev) for (uint32_t i = 0; i < nt / 2; i++) { const uint32_t t = sp[i]; sp[i] = sp[nt - 1 - i]; sp[nt - 1 - i] = t; }
      uint32_t remaining = fl, ns = 0;
      for (uint32_t i = 0; i < nt && remaining > 0; i++) {
        const uint32_t kd = sp[i] & 0xFu, ln = sp[i] >> 4;
        if (kd == 0 || kd == 1) { const uint32_t take = ln < remaining ? ln : remaining; sp[ns++] = (take << 4) | kd; remaining -= take; }
        else sp[ns++] = sp[i];
      }
      info |= ns << CD_NSIMP_SHIFT;
      S.final_len[tid] = fl; S.clip[tid] = clip;
    }
  }
  __syncthreads();
  if (S.bad) { refuse(); return; }

  // ---- 5. the read-count gate, the alignment filter per record side, the gates behind it ----
  const uint32_t na = (uint32_t)__syncthreads_count(mine && !r2 && strand == 0), nb = (uint32_t)__syncthreads_count(mine && !r2 && strand != 0);
  const uint64_t xy = na > nb ? na : nb, yx = na > nb ? nb : na;
  const bool gate = P.min_total <= xy + yx && P.min_xy <= xy && P.min_yx <= yx;
  uint64_t minority = 0;
  bool keep = true;
  if (gate) {
    for (uint32_t set = 0; set < 2; set++) {
      const bool member = mine && (strand == 0 ? r2 == set : r2 != set) && fl > 0;
      if (mine) S.info[tid] = (uint16_t)(member ? info | CD_MEMBER : info);
      const uint32_t m = (uint32_t)__syncthreads_count(member);
      if (m < 2) continue;
      // stable order, longest first, AB reads ahead of BA reads: the rank = reads ahead of this one
      uint32_t rank = 0;
      const uint32_t ns = info >> CD_NSIMP_SHIFT;
      if (member) {
        const uint32_t my_pos = (strand ? 512u : 0u) | tid;
        for (uint32_t j = 0; j < n; j++) {
          const uint32_t ij = S.info[j];
          if (!(ij & CD_MEMBER)) continue;
          const uint32_t lj = S.final_len[j], pj = ((ij & CD_STRAND) ? 512u : 0u) | j;
          rank += (lj > fl || (lj == fl && pj < my_pos)) ? 1u : 0u;
        }
      }
      uint32_t mask = 0, ng = 0;
      bool too_many = false;
      for (;;) {
        if (tid == 0) S.next = CD_NONE;
        __syncthreads();
        if (member && mask == 0) atomicMin(&S.next, (rank << 16) | tid);
        __syncthreads();
        const uint32_t nxt = S.next;
        if (nxt == CD_NONE) break;
        if (ng == canon::MAX_GROUPS) { too_many = true; break; }
        const uint32_t rep = nxt & 0xFFFFu, rep_rank = nxt >> 16;
        const bool joins = member && (rank == rep_rank || (rank > rep_rank && cd_is_prefix(S.simp[tid], ns, S.simp[rep], (uint32_t)S.info[rep] >> CD_NSIMP_SHIFT)));
        if (joins) mask |= 1u << ng;
        const uint32_t size = (uint32_t)__syncthreads_count(joins);
        if (tid == 0) { S.g_rep[ng] = rep; S.g_size[ng] = size; }
        ng++;
      }
      if (too_many) { refuse(); return; }
      uint32_t best = 0;                                   // larger group, then smaller CIGAR; the later group wins exact ties
      for (uint32_t g = 1; g < ng; g++) {
        int c;
        if (S.g_size[best] != S.g_size[g]) c = S.g_size[best] < S.g_size[g] ? -1 : 1;
        else { const uint32_t ra = S.g_rep[g], rb = S.g_rep[best]; c = cd_cmp(S.simp[ra], (uint32_t)S.info[ra] >> CD_NSIMP_SHIFT, S.simp[rb], (uint32_t)S.info[rb] >> CD_NSIMP_SHIFT); }
        if (c <= 0) best = g;
      }
      const bool dropped = member && !((mask >> best) & 1u);
      if (dropped) keep = false;
      minority += (uint32_t)__syncthreads_count(dropped);
    }
    if (minority) {
      const uint64_t ka = (uint32_t)__syncthreads_count(mine && keep && !r2 && strand == 0), kb = (uint32_t)__syncthreads_count(mine && keep && !r2 && strand != 0);
      const uint64_t kxy = ka > kb ? ka : kb, kyx = ka > kb ? kb : ka;
      if (!(P.min_total <= kxy + kyx && P.min_xy <= kxy && P.min_yx <= kyx)) { refuse(); return; }
    }
    if (P.max_reads_per_strand >= 0) {
      bool bites = false;
      for (uint32_t a = 0; a < 2; a++) for (uint32_t b = 0; b < 2; b++) {
        const uint64_t cnt = (uint32_t)__syncthreads_count(mine && keep && fl > 0 && (strand ? 1u : 0u) == a && r2 == b);
        if (cnt > (uint64_t)P.max_reads_per_strand) bites = true;
      }
      if (bites) { refuse(); return; }
    }
  }
  // the cell barcode is read from the molecule's first /A (else /B) record: when the filter drops it, its successor must carry the same value
  if (P.cell_tag[0] && minority) {
    const uint32_t want = has_a ? 0u : CD_STRAND;
    if (mine && strand == want) { atomicMin(&S.first_of, tid); if (keep) atomicMin(&S.first_kept, tid); }
    __syncthreads();
    if (tid == 0) {
      const uint32_t f0 = S.first_of, fk = S.first_kept;
      if (f0 != CD_NONE && f0 != fk) {
        if (fk == CD_NONE) S.bad = 1;
        else {
          const bam::Rec a{out + out_off[f0], rec_len[f0]}, b{out + out_off[fk], rec_len[fk]};
          uint32_t la = 0, lb = 0;
          const int64_t oa = bam::find_z_tag(a.b + a.aux_off(), a.len - a.aux_off(), (uint8_t)P.cell_tag[0], (uint8_t)P.cell_tag[1], &la);
          const int64_t ob = bam::find_z_tag(b.b + b.aux_off(), b.len - b.aux_off(), (uint8_t)P.cell_tag[0], (uint8_t)P.cell_tag[1], &lb);
          if ((oa < 0) != (ob < 0) || (oa >= 0 && la != lb)) S.bad = 1;
          else if (oa >= 0) for (uint32_t i = 0; i < la; i++) if (a.b[a.aux_off() + oa + i] != b.b[b.aux_off() + ob + i]) S.bad = 1;
        }
      }
    }
    __syncthreads();
    if (S.bad) { refuse(); return; }
  }

  // ---- 6. the canonical records and their prefixes ----
  if (mine) {
    uint32_t L = 0;
    if (keep) {
      L = canon::rewrite_record(out + out_off[tid], len, clip, r2 != 0);
      canon::wr32(out + out_off[tid] - 4, L);
    }
    out_len[tid] = L;
  }
  if (tid == 0) {
    canon::Delta D;
    D.minority = minority;
    for (int i = 0; i < 4; i++) D.ov[i] = S.ov[i];
    status[k] = canon::CANON_OK; delta[k] = D;
  }
}

}  // namespace

// The molecules of more than 64 records among the `nd` deferred ones (the interface of launch_canon_molecules, canon_device.hip, which calls this behind its lane
// kernel when FGX_DEEP_INDELS=1): one grid over the deferred list, a workgroup whose molecule is the lane kernel's returns at once.
void launch_canon_duplex_deep(hipStream_t s, const canon::Params& P, const uint8_t* d_blob, const uint64_t* d_rec_off, const uint32_t* d_rec_len, const uint32_t* d_grp_first,
                              const uint32_t* d_def, uint32_t nd, const uint64_t* d_first, uint8_t* d_out, const uint64_t* d_out_off, uint32_t* d_out_len, int* d_status,
                              canon::Delta* d_delta) {
  if (nd == 0) return;
  hipLaunchKernelGGL(k_canon_duplex_deep, dim3(nd), dim3(CD_NT), 0, s, P, d_blob, d_rec_off, d_rec_len, d_grp_first, d_def, nd, d_first, d_out, d_out_off, d_out_len, d_status,
                     d_delta);
  hip_check(hipGetLastError(), "k_canon_duplex_deep launch");
}

// Debug / test entry: ONE molecule (host arrays, the contract of fgx_canon_duplex_deep_host) through k_canon_duplex_deep.  `out` (records_len + 16 bytes) receives
// the canonical records at rec_off — which must leave room for the 4-byte prefix the kernel writes ahead of every kept record.  0, or 2 for bad arguments, 3 for a
// runtime error; *status = CANON_OK / CANON_OUT_OF_SCOPE.
extern "C" int fgx_debug_canon_duplex_deep_device(const fgx_options* o, const uint8_t* blob, uint64_t records_len, const uint64_t* rec_off, const uint32_t* rec_len, uint32_t n,
                                                  uint8_t* out, uint32_t* out_len, uint64_t* delta5, int* status) {
  if (!o || o->struct_size != sizeof(fgx_options) || !blob || !rec_off || !rec_len || !out || !out_len || !delta5 || !status || n <= 64) return 2;      // (a molecule of up to 64 records is the lane kernel's)
  for (uint32_t i = 0; i < n; i++) if (rec_off[i] < 4 || rec_len[i] > records_len || rec_off[i] > records_len - rec_len[i]) return 2;
  DevBuf d_blob, d_off, d_len, d_misc, d_out, d_olen;
  int rc = 0;
  try {
    if (o->device >= 0) hip_check(hipSetDevice(o->device), "hipSetDevice");      // (-1: the current device, as in fgx_create)
    d_blob.reserve(records_len + 64); d_off.reserve((size_t)n * 8); d_len.reserve((size_t)n * 4); d_out.reserve(records_len + 64); d_olen.reserve((size_t)n * 4);
    d_misc.reserve(256);      // grp_first[2] | def[1] | first[1] (u64, at 16) | status (at 24) | delta (at 32)
    uint8_t* const m = d_misc.as<uint8_t>();
    const uint32_t grp[3] = {0, n, 0};
    const uint64_t first0 = 0;
    hip_check(hipMemset(d_blob.p, 0, records_len + 64), "memset"); hip_check(hipMemset(d_out.p, 0, records_len + 64), "memset");
    hip_check(hipMemset(d_olen.p, 0, (size_t)n * 4), "memset"); hip_check(hipMemset(d_misc.p, 0, 256), "memset");
    hip_check(hipMemcpy(d_blob.p, blob, records_len, hipMemcpyHostToDevice), "H2D"); hip_check(hipMemcpy(d_off.p, rec_off, (size_t)n * 8, hipMemcpyHostToDevice), "H2D");
    hip_check(hipMemcpy(d_len.p, rec_len, (size_t)n * 4, hipMemcpyHostToDevice), "H2D"); hip_check(hipMemcpy(m, grp, 12, hipMemcpyHostToDevice), "H2D");
    hip_check(hipMemcpy(m + 16, &first0, 8, hipMemcpyHostToDevice), "H2D");
    const int unset = -1;
    hip_check(hipMemcpy(m + 24, &unset, 4, hipMemcpyHostToDevice), "H2D");
    launch_canon_duplex_deep(nullptr, canon_params_of(o), d_blob.as<uint8_t>(), d_off.as<uint64_t>(), d_len.as<uint32_t>(), (const uint32_t*)m, (const uint32_t*)(m + 8), 1,
                             (const uint64_t*)(m + 16), d_out.as<uint8_t>(), d_off.as<uint64_t>(), d_olen.as<uint32_t>(), (int*)(m + 24), (canon::Delta*)(m + 32));
    hip_check(hipDeviceSynchronize(), "k_canon_duplex_deep");
    canon::Delta D;
    int st = -1;
    hip_check(hipMemcpy(out, d_out.p, records_len, hipMemcpyDeviceToHost), "D2H"); hip_check(hipMemcpy(out_len, d_olen.p, (size_t)n * 4, hipMemcpyDeviceToHost), "D2H");
    hip_check(hipMemcpy(&st, m + 24, 4, hipMemcpyDeviceToHost), "D2H"); hip_check(hipMemcpy(&D, m + 32, sizeof(D), hipMemcpyDeviceToHost), "D2H");
    if (st < 0) { st = canon::CANON_OUT_OF_SCOPE; D.minority = 0; D.ov[0] = D.ov[1] = D.ov[2] = D.ov[3] = 0; for (uint32_t i = 0; i < n; i++) out_len[i] = 0; }
    *status = st;
    delta5[0] = D.minority; for (int i = 0; i < 4; i++) delta5[1 + i] = D.ov[i];
  } catch (const std::exception& ex) { fprintf(stderr, "fgx_debug_canon_duplex_deep_device: %s\n", ex.what()); rc = 3; }
  for (DevBuf* b : {&d_blob, &d_off, &d_len, &d_misc, &d_out, &d_olen}) b->free_();
  return rc;
}
