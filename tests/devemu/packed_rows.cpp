// TEST INFRASTRUCTURE: the row-loop arithmetic of k_split_cols's packed column pass (fgumi_amd/csrc/packed_core.h: keep_mask, acc_row, acc_row_seq and
// the clean test below_*) compiled for the host and walked the way the kernel walks it (simplex_split.inc phases 1b and 6: a "lane" per group of
// eight positions).  Bound by tests/test_packed_rows_core.py.
#include <cstdint>
#include <cstring>
#include "../../fgumi_amd/csrc/packed_core.h"

using namespace fgx;

extern "C" {

// q = 0 .. 255 at position `pos` of a group whose other seven qualities are `bg`: the keep words of both formulations
void prow_keep_masks(uint32_t floor_, uint32_t pos, uint32_t bg, uint32_t* branch_free, uint32_t* bitwise) {
  const uint32_t mb4 = floor_ * 0x01010101u;
  for (uint32_t q = 0; q < 256; q++) {
    uint8_t b[8];
    memset(b, (int)bg, 8);
    b[pos] = (uint8_t)q;
    uint32_t qx, qy;
    memcpy(&qx, b, 4); memcpy(&qy, b + 4, 4);
    branch_free[q] = pk::keep_mask(qx, qy, mb4); bitwise[q] = pk::keep_mask_bitwise(qx, qy, mb4);
  }
}

// rows of `qs` quality and `ss` sequence bytes, m rows, groups of eight positions: per group {f_or, A8, B8} of acc_row (with_q = 1) or acc_row_seq
void prow_acc(const uint8_t* seq, const uint8_t* qual, uint32_t qs, uint32_t ss, uint32_t m, uint32_t groups, uint32_t floor_, int with_q, uint32_t* out3) {
  const uint32_t mb4 = floor_ * 0x01010101u;
  for (uint32_t k = 0; k < groups; k++) {
    pk::Acc A;
    pk::acc_reset(A);
    for (uint32_t j = 0; j < m; j++) {
      uint32_t qx, qy, b;
      memcpy(&qx, qual + (size_t)j * qs + 8u * k, 4); memcpy(&qy, qual + (size_t)j * qs + 8u * k + 4, 4); memcpy(&b, seq + (size_t)j * ss + 4u * k, 4);
      if (with_q) pk::acc_row(A, qx, qy, b, mb4); else pk::acc_row_seq(A, b);
    }
    out3[3 * k] = A.f_or; out3[3 * k + 1] = A.A8; out3[3 * k + 2] = A.B8;
  }
}

// the clean test of one end: m rows of `qs` quality bytes, row j a read of lens[j] bases (the rows are as wide as the longest).  per_row = 0: the
// kernel's choice (one length: masks once behind the last row; several: each row with its own), 1: the per-row form whatever the lengths.
// Returns 1 = some quality below the floor at a position below its read's length ("not clean"), 0 = clean.
int prow_dirty(const uint8_t* qual, uint32_t qs, uint32_t m, const uint32_t* lens, uint32_t floor_, int per_row) {
  if (floor_ > 128u) return 1;
  uint32_t lenE = 0;
  bool one_len = true;
  for (uint32_t j = 0; j < m; j++) { if (lens[j] > lenE) lenE = lens[j]; if (lens[j] != lens[0]) one_len = false; }
  const uint32_t mb4 = floor_ * 0x01010101u, groups = (lenE + 7u) >> 3;
  bool dirty = false;
  for (uint32_t k = 0; k < groups; k++) {
    pk::Below Z;
    pk::below_reset(Z);
    for (uint32_t j = 0; j < m; j++) {
      uint32_t qx, qy;
      memcpy(&qx, qual + (size_t)j * qs + 8u * k, 4); memcpy(&qy, qual + (size_t)j * qs + 8u * k + 4, 4);
      if (one_len && !per_row) pk::below_row(Z, qx, qy, mb4); else pk::below_row_len(Z, qx, qy, mb4, lens[j], k);
    }
    if (one_len && !per_row) { uint32_t nfl, nfh; pk::count_masks(lenE, k, &nfl, &nfh); dirty |= pk::below_any(Z, nfl, nfh); }
    else dirty |= pk::below_any(Z, pk::H, pk::H);
  }
  return dirty ? 1 : 0;
}

}  // extern "C"
