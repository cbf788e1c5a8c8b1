// seq_bits.h -- what the sequence stages share, host and device: how a byte is read as a base, the limits of a read window
// and an oligo, and THE bit-vector edit-distance recurrence.  bc_search / bc_search_multi (bc_kernels.hip), ls_edit
// (ls_kernels.hip) and mp_verify (mp_kernels.hip) all step through bv_step_word; ep_kernels.hip, mp_kernels.hip and the
// index builder in lva_stages.cpp read bytes through base_code.  tests/test_seq_bits_host.py holds both to a plain DP.
#pragma once
#include <cstdint>

#ifdef __HIP__
#define SEQ_HD __host__ __device__
#else
#define SEQ_HD
#endif

namespace lva {

constexpr int kMaxRef = 1024;              // oligo positions (the simulator's strand limit)
constexpr int kMaxRead = 4096;             // bases of a read window
constexpr uint32_t kBaseN = 4;

// basecall characters and lva_encode's codes -> 0..3, anything else N
SEQ_HD inline uint32_t base_code(uint8_t b) {
  switch (b) {
    case 'A': case 0: return 0;
    case 'C': case 1: return 1;
    case 'G': case 2: return 2;
    case 'T': case 3: return 3;
    default: return kBaseN;
  }
}

// the base on the other strand; N stays N
SEQ_HD inline uint32_t complement_code(uint32_t c) { return c < kBaseN ? 3u - c : kBaseN; }

// One column of the unit-cost matrix over 64 rows (Myers' bit-vector recurrence in its block form): pv / mv are the
// vertical +1 / -1 deltas of the column, eq the rows whose pattern symbol equals the column's text symbol, hin the
// horizontal delta entering the word's first row (-1, 0, +1; +1 throughout: D[0][j] = j, the whole-string distance; 0:
// D[0][j] = 0, the text's ends are free).  Leaves the next column in pv / mv and the horizontal deltas of the 64 rows in
// ph / mh; returns the delta leaving the last row, which enters the next word.
SEQ_HD inline int bv_step_word(uint64_t& pv, uint64_t& mv, uint64_t eq, int hin, uint64_t& ph, uint64_t& mh) {
  const uint64_t neg = hin < 0 ? 1ull : 0ull, pos = hin > 0 ? 1ull : 0ull;
  const uint64_t xv = eq | mv;
  eq |= neg;
  const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;
  ph = mv | ~(xh | pv);
  mh = pv & xh;
  const int hout = (int)(ph >> 63) - (int)(mh >> 63);
  const uint64_t phs = (ph << 1) | pos, mhs = (mh << 1) | neg;
  pv = mhs | ~(xv | phs);
  mv = phs & xv;
  return hout;
}

// what a column adds to the score D[m][j]: the horizontal delta of row m, bit (m - 1) & 63 of word (m - 1) >> 6
SEQ_HD inline int bv_row_delta(uint64_t ph, uint64_t mh, int bit) { return (int)((ph >> bit) & 1ull) - (int)((mh >> bit) & 1ull); }

}  // namespace lva
