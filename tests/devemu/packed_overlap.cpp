// TEST INFRASTRUCTURE: the overlap correction of k_split_cols's packed build on packed words (fgumi_amd/csrc/packed_core.h: ov_step and the
// gather / scatter functions around it) compiled for the host, against the rule stated position by position (overlapping.rs:236-336 as
// simplex_split.inc's shared_base applies it).  Bound by tests/test_packed_overlap_core.py.
#include <cstdint>
#include <cstring>
#include "../../fgumi_amd/csrc/packed_core.h"

using namespace fgx;

namespace {

// ---- the rule, one shared position -----------------------------------------------------------------------------------------------------
struct Cnt { uint32_t agree, dis, corr; };
void rule(uint32_t& c1, uint32_t& c2, uint32_t& qa, uint32_t& qb, uint32_t floor_, Cnt& n) {
  if (c1 == 15u || c2 == 15u) return;
  uint32_t newq, newc;
  if (c1 == c2) {
    const uint32_t sm = qa + qb;
    newq = sm < 93u ? sm : 93u;
    newc = c1;
    n.agree++;
    if (newq != qa || newq != qb) n.corr++;
  } else {
    const int d = (int)qa - (int)qb;
    const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
    newq = ad < 2u ? 2u : ad;
    newc = d == 0 ? 15u : d > 0 ? c1 : c2;
    n.dis++;
    n.corr += 2;
  }
  if (newq < floor_) newc = 0;
  c1 = c2 = newc; qa = qb = newq;
}

uint32_t code_at(const uint8_t* seq, uint32_t p) { return (seq[p >> 1] >> ((~p & 1u) << 2)) & 15u; }
void set_code(uint8_t* seq, uint32_t p, uint32_t c) { const uint32_t sh = (~p & 1u) << 2; seq[p >> 1] = (uint8_t)((seq[p >> 1] & ~(15u << sh)) | (c << sh)); }
uint32_t ld32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
void st32(uint8_t* p, uint32_t v) { memcpy(p, &v, 4); }
uint64_t splitmix(uint64_t& s) { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

}  // namespace

extern "C" {

// Exhaustive at ONE position `pos` of a group and one floor: all 16 x 16 code pairs x all quality pairs 0 .. 127; the seven other positions hold
// codes and qualities drawn from `seed` (codes 15 and equal codes among them).  Every output of ov_step is compared at all eight positions
// with the rule: A's stored words, B's words after its deltas, the three counts.  Returns the number of inputs that differ (first[8]: c1, c2,
// qa, qb of the first one and what differed).
uint64_t pov_exhaustive(uint32_t floor_, uint32_t pos, uint64_t seed, uint32_t* first) {
  const uint32_t mb4 = floor_ * 0x01010101u;
  uint8_t qA[8], qB[8], sA[4], sB[4];
  uint64_t s = seed, bad = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t r = splitmix(s);
    qA[i] = (uint8_t)(r % 128u); qB[i] = (uint8_t)((r >> 8) % 128u);
    static const uint8_t pool[8] = {1, 2, 4, 8, 15, 0, 3, 1};
    const uint32_t ca = pool[(r >> 16) & 7u], cb = ((r >> 24) & 3u) ? ca : pool[(r >> 32) & 7u];
    set_code(sA, (uint32_t)i, ca); set_code(sB, (uint32_t)i, cb);
  }
  // the seven other positions: their results once
  uint32_t wc1[8], wc2[8], wq1[8], wq2[8];
  Cnt base = {0, 0, 0};
  for (uint32_t i = 0; i < 8; i++) {
    wc1[i] = code_at(sA, i); wc2[i] = code_at(sB, i); wq1[i] = qA[i]; wq2[i] = qB[i];
    if (i != pos) rule(wc1[i], wc2[i], wq1[i], wq2[i], floor_, base);
  }
  for (uint32_t c1 = 0; c1 < 16; c1++)
    for (uint32_t c2 = 0; c2 < 16; c2++) {
      set_code(sA, pos, c1); set_code(sB, pos, c2);
      const uint32_t caw = ld32(sA), cbp = pk::swap_nibbles(ld32(sB));
      for (uint32_t qa = 0; qa < 128; qa++) {
        qA[pos] = (uint8_t)qa;
        for (uint32_t qb = 0; qb < 128; qb++) {
          qB[pos] = (uint8_t)qb;
          pk::OvStep R;
          pk::ov_step(ld32(qA), ld32(qA + 4), caw, ld32(qB), ld32(qB + 4), cbp, 0xFFFFFFFFu, 0xFFFFFFFFu, mb4, R);
          uint32_t e1 = c1, e2 = c2, ea = qa, eb = qb;
          Cnt n = base;
          rule(e1, e2, ea, eb, floor_, n);
          // A as stored, B after its deltas
          uint8_t gqa[8], gqb[8], gsa[4], gsb[4];
          st32(gqa, R.qa[0]); st32(gqa + 4, R.qa[1]); st32(gsa, R.ca);
          st32(gqb, ld32(qB) ^ R.dq[0]); st32(gqb + 4, ld32(qB + 4) ^ R.dq[1]); st32(gsb, pk::swap_nibbles(cbp ^ R.dc));
          bool ok = (R.n_ad & 0xFFFFu) == n.agree && (R.n_ad >> 16) == n.dis && R.n_chg + 2u * n.dis == n.corr;
          for (uint32_t i = 0; i < 8 && ok; i++) {
            const uint32_t x1 = i == pos ? e1 : wc1[i], x2 = i == pos ? e2 : wc2[i], y1 = i == pos ? ea : wq1[i], y2 = i == pos ? eb : wq2[i];
            ok = code_at(gsa, i) == x1 && code_at(gsb, i) == x2 && gqa[i] == y1 && gqb[i] == y2;
          }
          if (!ok) { if (!bad && first) { first[0] = c1; first[1] = c2; first[2] = qa; first[3] = qb; first[4] = R.n_ad; first[5] = R.n_chg; first[6] = n.agree | (n.dis << 16); first[7] = n.corr; } bad++; }
        }
      }
    }
  return bad;
}

// One pair the way the kernel walks it: rows of qs quality / ss sequence bytes; A's shared bases start at its base 0, B's at `off`; cn shared
// bases; a "lane" per group of eight, in the order order[] gives (any order must do: the deltas compose).  The rows are corrected IN PLACE;
// counts3 = agree, dis, corr.  Returns 1 when the guard fires (a byte of 128 or more at a shared position: nothing is written), else 0.
int pov_pair(uint8_t* qA, uint8_t* sA, uint8_t* qB, uint8_t* sB, uint32_t qs, uint32_t ss, uint32_t off, uint32_t cn, uint32_t floor_, const uint32_t* order, uint32_t* counts3) {
  const uint32_t mb4 = floor_ * 0x01010101u, ng = (cn + 7u) >> 3, sq = off & 3u, sn = off & 7u;
  counts3[0] = counts3[1] = counts3[2] = 0;
  struct Lane { uint32_t bq0, bq1, bq2, bs0, bs1, ml, mh, qax, qay, caw, qbx, qby, cbp; };
  auto load = [&](uint32_t k, Lane& L) {
    const uint32_t bqe = qs - 4u, bse = ss - 4u;
    L.bq0 = 4u * ((off >> 2) + 2u * k); L.bq1 = L.bq0 + 4u < bqe ? L.bq0 + 4u : bqe; L.bq2 = L.bq0 + 8u < bqe ? L.bq0 + 8u : bqe;
    L.bs0 = 4u * ((off >> 3) + k); L.bs1 = L.bs0 + 4u < bse ? L.bs0 + 4u : bse;
    pk::ov_in_masks(cn, k, &L.ml, &L.mh);
    L.qax = ld32(qA + 8u * k); L.qay = ld32(qA + 8u * k + 4u); L.caw = ld32(sA + 4u * k);
    pk::ov_gather_q(ld32(qB + L.bq0), ld32(qB + L.bq1), ld32(qB + L.bq2), sq, &L.qbx, &L.qby);
    L.cbp = pk::ov_gather_c(ld32(sB + L.bs0), ld32(sB + L.bs1), sn);
  };
  for (uint32_t k = 0; k < ng; k++) { Lane L; load(k, L); if (pk::ov_high(L.qax, L.qay, L.qbx, L.qby, L.ml, L.mh)) return 1; }
  uint32_t n_ad = 0, n_chg = 0;
  for (uint32_t i = 0; i < ng; i++) {
    const uint32_t k = order[i];
    Lane L;
    load(k, L);
    pk::OvStep R;
    pk::ov_step(L.qax, L.qay, L.caw, L.qbx, L.qby, L.cbp, L.ml, L.mh, mb4, R);
    uint32_t e[3], f[2];
    pk::ov_scatter_q(R.dq[0], R.dq[1], sq, e); pk::ov_scatter_c(R.dc, sn, f);
    st32(qA + 8u * k, R.qa[0]); st32(qA + 8u * k + 4u, R.qa[1]); st32(sA + 4u * k, R.ca);
    st32(qB + L.bq0, ld32(qB + L.bq0) ^ e[0]); st32(qB + L.bq1, ld32(qB + L.bq1) ^ e[1]); st32(qB + L.bq2, ld32(qB + L.bq2) ^ e[2]);
    st32(sB + L.bs0, ld32(sB + L.bs0) ^ f[0]); st32(sB + L.bs1, ld32(sB + L.bs1) ^ f[1]);
    n_ad += R.n_ad; n_chg += R.n_chg;
  }
  counts3[0] = n_ad & 0xFFFFu; counts3[1] = n_ad >> 16; counts3[2] = n_chg + 2u * counts3[1];
  return 0;
}

// the same pair by the rule, position by position
void pov_pair_rule(uint8_t* qA, uint8_t* sA, uint8_t* qB, uint8_t* sB, uint32_t off, uint32_t cn, uint32_t floor_, uint32_t* counts3) {
  Cnt n = {0, 0, 0};
  for (uint32_t w = 0; w < cn; w++) {
    uint32_t c1 = code_at(sA, w), c2 = code_at(sB, off + w), qa = qA[w], qb = qB[off + w];
    rule(c1, c2, qa, qb, floor_, n);
    set_code(sA, w, c1); set_code(sB, off + w, c2); qA[w] = (uint8_t)qa; qB[off + w] = (uint8_t)qb;
  }
  counts3[0] = n.agree; counts3[1] = n.dis; counts3[2] = n.corr;
}

// the host twins of the builtins, for a check against their definitions in Python
uint32_t pov_alignbyte(uint32_t hi, uint32_t lo, uint32_t n) { return pk::alignbyte(hi, lo, n); }
uint32_t pov_alignbit(uint32_t hi, uint32_t lo, uint32_t n) { return pk::alignbit(hi, lo, n); }
uint32_t pov_popc(uint32_t x) { return pk::popc(x); }

}  // extern "C"
