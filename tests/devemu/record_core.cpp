// TEST INFRASTRUCTURE: the per-record rules of the simplex parsers (fgumi_amd/csrc/record_core.h: the very functions the kernels inline) compiled for the
// host.  The clip grids run here, record by record, against bam::mate_clip (bamrec.h: the op-by-op rule) and against the oracle's orc_mate_clip, which the
// test hands in as a function pointer.  Bound by tests/test_record_core.py.
#include <cstdint>
#include <cstring>
#include <cstdio>
#include "../../fgumi_amd/csrc/record_core.h"

using namespace fgx;

namespace {

void put32(uint8_t* p, uint32_t v) { memcpy(p, &v, 4); }

// a record of one M op: name "q", l_seq bases, MC:Z:<ML>M — returns its length
uint32_t build_record(uint8_t* b, int32_t ref_id, int32_t pos, uint32_t flags, uint32_t l_seq, int32_t mref, int32_t mpos, uint32_t ML, uint32_t* mc_off, uint32_t* mc_len) {
  const uint32_t l_name = 2;
  put32(b, (uint32_t)ref_id); put32(b + 4, (uint32_t)pos); put32(b + 8, l_name | (60u << 8) | (4680u << 16)); put32(b + 12, 1u | (flags << 16));
  put32(b + 16, l_seq); put32(b + 20, (uint32_t)mref); put32(b + 24, (uint32_t)mpos); put32(b + 28, 0);
  uint32_t o = 32;
  b[o++] = 'q'; b[o++] = 0;
  put32(b + o, l_seq << 4); o += 4;
  for (uint32_t i = 0; i < (l_seq + 1) / 2; i++) b[o++] = 0x11;
  for (uint32_t i = 0; i < l_seq; i++) b[o++] = 30;
  b[o++] = 'M'; b[o++] = 'C'; b[o++] = 'Z';
  *mc_off = o;
  const int n = snprintf((char*)b + o, 16, "%uM", ML);
  *mc_len = (uint32_t)n;
  o += (uint32_t)n + 1;
  return o;
}

}  // namespace

extern "C" {

typedef uint64_t (*OracleClip)(const uint8_t*, uint32_t);

// Every combination of the listed pos / mpos / l_seq / ML values x both strands of read and mate x {paired on one reference, unpaired, mate unmapped,
// mate on another reference}: record::single_m_mate_clip behind the guards the kernels apply, bam::mate_clip and the oracle.  Returns the number of
// records checked; *n_bad = records where the three do not agree, bad[0..7] = the first such case (pos, mpos, l_seq, ML, flags, closed form, bamrec, oracle)
uint64_t rcore_clip_grid(const int32_t* pos_v, uint32_t n_pos, const int32_t* mpos_v, uint32_t n_mpos, const uint32_t* lseq_v, uint32_t n_lseq, const uint32_t* ml_v, uint32_t n_ml,
                         OracleClip oracle, uint64_t* n_bad, int64_t* bad) {
  static uint8_t b[32 + 2 + 4 + 32768 + 65536 + 32];
  uint64_t checked = 0;
  *n_bad = 0;
  for (uint32_t a = 0; a < n_pos; a++) for (uint32_t c = 0; c < n_mpos; c++) for (uint32_t d = 0; d < n_lseq; d++) for (uint32_t e = 0; e < n_ml; e++)
    for (uint32_t strands = 0; strands < 4; strands++) for (uint32_t kind = 0; kind < 4; kind++) {
      uint32_t flags = (strands & 1 ? bam::F_REVERSE : 0) | (strands & 2 ? bam::F_MATE_REVERSE : 0);
      if (kind != 1) flags |= bam::F_PAIRED | bam::F_FIRST;
      if (kind == 2) flags |= bam::F_MATE_UNMAPPED;
      const int32_t mref = kind == 3 ? 4 : 3;
      uint32_t mc_off, mc_len;
      const uint32_t len = build_record(b, 3, pos_v[a], flags, lseq_v[d], mref, mpos_v[c], ml_v[e], &mc_off, &mc_len);
      // the closed form, as the parsers reach it
      const record::FixedHeader H = record::decode_header(bam::rd32(b), bam::rd32(b + 4), bam::rd32(b + 8), bam::rd32(b + 12), bam::rd32(b + 16));
      const record::MateFields M = record::decode_mate(bam::rd32(b + 20), bam::rd32(b + 24));
      const uint32_t ML = record::mc_single_m(mc_len, [&]() { unsigned long long v; memcpy(&v, b + mc_off, 8); return v; });
      int64_t got = -1;
      // (k_family_wave calls it with the mate-unmapped flag set and relies on the function's own term; the streaming parsers test the flag before)
      if (ML != 0 && record::mate_in_range(M)) got = record::single_m_mate_clip(H, H.ref_id, M, (int32_t)ML);
      // the op-by-op rule
      uint32_t ops[1] = {lseq_v[d] << 4}, mops[8];
      bool overflow = false;
      const bam::Rec v{b, len};
      const int64_t want = (int64_t)bam::mate_clip(v, ops, 1, b + mc_off, mc_len, mops, 8, &overflow);
      const int64_t orc = (int64_t)oracle(b, len);
      checked++;
      if (got != want || got != orc || overflow) {
        if (!*n_bad) { bad[0] = pos_v[a]; bad[1] = mpos_v[c]; bad[2] = lseq_v[d]; bad[3] = ml_v[e]; bad[4] = flags; bad[5] = got; bad[6] = want; bad[7] = orc; }
        ++*n_bad;
      }
      // the overlap alone (the CODEC caller's use: a pair known to be FR, the mate's length in hand) where the whole rule found an FR pair
      if (got > 0 && (int64_t)record::single_m_overlap_clip((flags & bam::F_REVERSE) != 0, H.pos, (int32_t)H.l_seq, M.pos, (int32_t)ML) != got) ++*n_bad;
    }
  return checked;
}

// `<n>M` of an MC value (its bytes, no NUL needed): n, 0 = not of that form.  The eight bytes come from a buffer whose bytes past the value are `pad`
uint32_t rcore_mc(const uint8_t* s, uint32_t n, uint32_t pad) {
  uint8_t buf[16];
  memset(buf, (int)pad, sizeof(buf));
  memcpy(buf, s, n < 16 ? n : 16);
  return record::mc_single_m(n, [&]() { unsigned long long v; memcpy(&v, buf, 8); return v; });
}

// The pairing hash of the name at buf[off, off + name_len) through the three fetch styles of the kernels: 0 = an LDS slice (base + record offset + 32 + o, one
// unaligned read), 1 = the global record (pointer + 32 + o), 2 = the split kernel's head window (the window starts at the name: offset o).  `steps`, if given, takes
// the 8-byte input of every step in order (up to 64); returns the hash
uint32_t rcore_name_hash(int style, const uint8_t* buf, uint32_t off, uint32_t name_len, uint64_t* steps, uint32_t* n_steps) {
  uint32_t k = 0;
  auto log32 = [&](uint32_t w) { if (steps && k < 128) { if (k & 1) steps[k >> 1] |= (uint64_t)w << 32; else steps[k >> 1] = w; } k++; return w; };
  auto log64 = [&](unsigned long long v) { const unsigned long long m = v & ((1ULL << (8 * name_len)) - 1ULL); if (steps && k < 128) steps[k >> 1] = m; k += 2; return v; };
  uint32_t h;
  if (style == 0) {
    const uint8_t* W = buf; const uint32_t lo = off - 32;      // (the record would start 32 bytes before its name)
    h = record::name_hash30(name_len, [&](uint32_t o) { uint32_t v; memcpy(&v, W + (lo + 32 + o), 4); return log32(v); },
                            [&](uint32_t o) { unsigned long long v; memcpy(&v, W + (lo + 32 + o), 8); return log64(v); });
  } else if (style == 1) {
    const uint8_t* rec = buf + off - 32;
    h = record::name_hash30(name_len, [&](uint32_t o) { return log32(bam::rd32(rec + 32 + o)); },
                            [&](uint32_t o) { return log64((unsigned long long)bam::rd32(rec + 32 + o) | ((unsigned long long)bam::rd32(rec + 36 + o) << 32)); });
  } else {
    uint8_t Wh[48 + 8];
    memset(Wh, 0xEE, sizeof(Wh));
    memcpy(Wh, buf + off, name_len < 48 ? name_len : 48);
    if (name_len < 48) memcpy(Wh + name_len, buf + off + name_len, 48 - name_len);   // what follows the name in the record follows it in the window
    h = record::name_hash30(name_len, [&](uint32_t o) { uint32_t v; memcpy(&v, Wh + o, 4); return log32(v); }, [&](uint32_t o) { unsigned long long v; memcpy(&v, Wh + o, 8); return log64(v); });
  }
  if (n_steps) *n_steps = k >> 1;
  return h;
}

// header dwords d[0..7) and the record length -> out[0..3) = seq / qual / aux offsets, returns bit 0 layout odd, bit 1 streaming_header_odd, bit 2 streaming_flags_odd
uint32_t rcore_shape(const uint32_t* d, uint32_t len, uint32_t max_cig, int take_unmapped, uint32_t head_window, int frag_with_mate_flags_odd, uint32_t* out) {
  const record::FixedHeader H = record::decode_header(d[0], d[1], d[2], d[3], d[4]);
  const record::Layout L = record::layout(H, len);
  out[0] = L.seq_off; out[1] = L.qual_off; out[2] = L.aux_off;
  return (L.odd ? 1u : 0u) | (record::streaming_header_odd(H, max_cig, take_unmapped != 0, head_window) ? 2u : 0u) | (record::streaming_flags_odd(H, frag_with_mate_flags_odd != 0) ? 4u : 0u);
}
int rcore_single_block_op(uint32_t op, uint32_t l_seq) { return record::single_block_op(op, l_seq) ? 1 : 0; }

// the one-aligned-block walk over n ops: out = lead, aln, trail, tot; returns bit 0 fits l_seq, bit 1 complex (I / D / N / P)
uint32_t rcore_cigar_block(const uint32_t* ops, uint32_t n, uint32_t l_seq, uint32_t* out) {
  record::CigarBlock B = record::cigar_block_start();
  for (uint32_t i = 0; i < n; i++) record::cigar_block_op(B, ops[i]);
  out[0] = B.lead; out[1] = B.aln; out[2] = B.trail; out[3] = B.tot;
  return (record::cigar_block_fits(B, l_seq) ? 1u : 0u) | (B.cplx ? 2u : 0u);
}

int rcore_first_record_odd(int has_mi, uint32_t mi_len, uint32_t prefix_len) { return record::first_record_odd(has_mi != 0, mi_len, prefix_len) ? 1 : 0; }

}  // extern "C"
