// st_kernels.hip -- DESIGN.md section 1 row N7, the traceback: the best path of a given base sequence on a read.
//
// The definition is trellis_score.reference_trace; the device is held to it byte for byte (tests/test_gpu_trellis_trace.py).
// The forward pass is the frame that sc_score runs (sc_frame.h) under a cell rule that adds the one thing a traceback
// needs -- which predecessor won.  The tie rule is the one sc_score's hi_of chain implies: a later candidate replaces an
// earlier one only if it is strictly greater, the candidates in the frame's order (stay first, then the states of the
// position below, ascending; for a flop the stay, then the step).
//
//   st_fill   sc_frame under StRule: same LDS, same additions, the maxima as compare and select, so the two end scores are
//             sc_score's bits.  For every cell it writes it stores one back-pointer byte (st_kernels.h) to the pair's
//             scratch in HBM, [nblk][w] indexed by p - lo(t): consecutive lanes store consecutive bytes.
//   st_walk   the traceback, one wavefront per pair, in runs of kStRun blocks: the 64 lanes stage the kStRun bytes of each
//             row that the walk can reach (it moves down at most one position per block) and the band words of the run
//             into LDS -- one byte per lane and row, consecutive lanes consecutive bytes, the loads of a run in flight
//             together -- and the run is then walked out of LDS by the whole wavefront in step (every value it decides on
//             goes through readfirstlane, so the walk is scalar control flow and lane 0 stores what it finds).  A position
//             outside a block's band holds what it held two blocks earlier: the walk goes there and counts a stale hop.
//
// Two kernels, not a tail: the walk wants other LDS (staged rows, not parity buffers) and other registers than the fill,
// whose register figure is what keeps eight wavefronts on a SIMD; launched on one stream the second sees the first's stores.
//
// LDS ordering in st_fill is the frame's (sc_frame.h); StRule stores to HBM only.  In st_walk a barrier separates a run's
// staging stores from its walk and the walk's loads from the next run's staging; control flow around both is uniform.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sc_frame.h"
#include "st_kernels.h"

namespace lva {

namespace {

// ScRule's maxima with the winner kept, and the byte of every cell stored after it
struct StRule : ScRule {
  uint8_t* back;          // the pair's back-pointers, [nblk][w]
  uint32_t w;
  uint8_t* brow;          // brow[p - lo]: the byte of position p of this block
  uint32_t won, in;       // of the cell at hand: the flip's choice, the flop's bit

  __device__ StRule(uint8_t* back, uint32_t w) : back(back), w(w), brow(back), won(0), in(0) {}
  __device__ float flip_first(float stay, const float (&x)[8], uint32_t b) {
    float flip = stay;
    won = 0;
#pragma unroll
    for (uint32_t s = 0; s < 8; ++s)
      if (s != b && flip < x[s]) { flip = x[s]; won = 1 + s; }
    return flip;
  }
  __device__ float flip_of(float stay, float from_flip, float from_flop, uint32_t b2) {
    float flip = stay;
    won = 0;
    if (flip < from_flip) { flip = from_flip; won = 1 + b2; }
    if (flip < from_flop) { flip = from_flop; won = 5 + b2; }
    return flip;
  }
  __device__ float flop_of(float stay, float step) {
    in = stay < step ? kStFlopBit : 0u;
    return in ? step : stay;
  }
  __device__ void block_begins(int t) { brow = back + (size_t)t * w; }
  __device__ void stored(int p, int lo) const { brow[p - lo] = (uint8_t)(p == 0 ? 0u : won | in); }   // position 0 only stays
};

// grid = pairs, block = one wavefront; dynamic LDS: sc_lds_bytes(max_len), cap = sc_lds_positions(max_len)
__global__ __launch_bounds__(64) void st_fill(const float* __restrict__ post, const uint8_t* __restrict__ bases,
                                              const ScPair* __restrict__ pairs, const StBp* __restrict__ bp,
                                              const uint32_t* __restrict__ band, int cap, uint8_t* __restrict__ scratch,
                                              float* __restrict__ out) {
  const StBp where = bp[blockIdx.x];
  sc_frame(post, bases, pairs, band, cap, out, StRule(scratch + where.at, where.w));
}

__device__ inline uint32_t first_lane(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// grid = pairs, block = one wavefront; dynamic LDS: st_walk_lds_bytes()
__global__ __launch_bounds__(64) void st_walk(const uint8_t* __restrict__ bases, const ScPair* __restrict__ pairs,
                                              const StBp* __restrict__ bp, const uint32_t* __restrict__ band,
                                              const uint8_t* __restrict__ scratch, const float* __restrict__ score, int end,
                                              int stride, int32_t* __restrict__ out_enter, uint8_t* __restrict__ out_kind,
                                              int32_t* __restrict__ out_info) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint8_t* stage = reinterpret_cast<uint8_t*>(smem);                            // [kStRun][kStRun]: row u = block t - u
  uint32_t* sband = reinterpret_cast<uint32_t*>(smem + kStRun * kStRun);        // [kStRun]: its band word

  const int lane = threadIdx.x;
  const ScPair pr = pairs[blockIdx.x];
  const StBp where = bp[blockIdx.x];
  const int len = (int)pr.len, nblk = (int)pr.nblk;
  int32_t* enter = out_enter + (size_t)blockIdx.x * stride;
  uint8_t* kind = out_kind + (size_t)blockIdx.x * stride;
  int32_t* info = out_info + (size_t)blockIdx.x * 4;

  const float flip = score[(size_t)blockIdx.x * 2], flop = score[(size_t)blockIdx.x * 2 + 1];
  int k = (int)first_lane(end < 0 ? (flip < flop ? 1u : 0u) : (uint32_t)end);   // the state the walk is in: 0 flip, 1 flop
  const bool path = first_lane((k ? flop : flip) != kNegInf ? 1u : 0u) != 0u;
  // a path enters every position once, so the walk fills [0, len) itself; the rest of the row, or all of it, is filled here
  for (int j = (path ? len : 0) + lane; j < stride; j += kStRun) { enter[j] = -1; kind[j] = 255; }
  if (!path) {
    if (lane == 0) { info[0] = -1; info[1] = -1; info[2] = 0; info[3] = 0; }
    return;
  }
  const int end_state = k;
  const uint8_t* rows = scratch + where.at;
  int t = nblk - 1, p = len, n_stale = 0, start_state = -1;
  while (t >= 0) {
    const int nrows = min(kStRun, t + 1);
    const int low = p - (kStRun - 1), col = low + lane;                 // the run can reach positions low .. p
    const uint32_t my_band = lane < nrows ? band[pr.band_at + t - lane] : 0u;
    sband[lane] = my_band;
    for (int u0 = 0; u0 < nrows; u0 += 8) {                             // eight rows' loads in flight, then their LDS stores
      uint8_t v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {                                     // (a row past nrows has the band word 0: no lane loads)
        const uint32_t bw = __builtin_amdgcn_readlane(my_band, u0 + i);
        const int lo = (int)(bw & 0xFFFFu), hi = (int)(bw >> 16);
        v[i] = col >= lo && col < hi ? rows[(size_t)(t - u0 - i) * where.w + (col - lo)] : (uint8_t)0;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) stage[(u0 + i) * kStRun + lane] = v[i];
    }
    __syncthreads();
    int u = 0;
    while (u < nrows) {
      const uint32_t bw = first_lane(sband[u]);
      const int lo = (int)(bw & 0xFFFFu), hi = (int)(bw >> 16);
      if (p < lo || p >= hi) {                                          // stale: the cell holds what it held two blocks earlier
        ++n_stale;
        u += 2;
        continue;
      }
      const uint32_t byte = first_lane(stage[u * kStRun + (p - low)]);
      const uint32_t won = k ? (byte >> 4) & 1u : byte & 15u;
      if (won == 0 || p == 0) { ++u; continue; }                        // a stay
      if (lane == 0) { enter[p - 1] = t - u; kind[p - 1] = (uint8_t)k; }
      if (p == 1) {                                                     // into position 0: a flop is entered from flip b
        start_state = k ? (int)first_lane(base_code(bases[pr.seq_off]) & 3u) : (int)won - 1;
        k = 0;
      } else {
        k = k ? 0 : (won >= 5u ? 1 : 0);
      }
      --p;
      ++u;
    }
    __syncthreads();
    t -= u;
  }
  if (lane == 0) { info[0] = end_state; info[1] = start_state; info[2] = n_stale; info[3] = 0; }
}

}  // namespace

int launch_st_fill(const float* post, const uint8_t* bases, const ScPair* pairs, const StBp* bp, const uint32_t* band,
                   int32_t n_pairs, int32_t max_len, uint8_t* scratch, float* out_score, void* stream) {
  if (n_pairs <= 0) return 0;
  hipLaunchKernelGGL(st_fill, dim3(n_pairs), dim3(64), sc_lds_bytes(max_len), (hipStream_t)stream, post, bases, pairs, bp, band,
                     (int)sc_lds_positions(max_len), scratch, out_score);
  return (int)hipGetLastError();
}

int launch_st_walk(const uint8_t* bases, const ScPair* pairs, const StBp* bp, const uint32_t* band, int32_t n_pairs,
                   const uint8_t* scratch, const float* score, int32_t end, int32_t stride, int32_t* out_enter, uint8_t* out_kind,
                   int32_t* out_info, void* stream) {
  if (n_pairs <= 0) return 0;
  hipLaunchKernelGGL(st_walk, dim3(n_pairs), dim3(kStRun), st_walk_lds_bytes(), (hipStream_t)stream, bases, pairs, bp, band, scratch,
                     score, (int)end, (int)stride, out_enter, out_kind, out_info);
  return (int)hipGetLastError();
}

}  // namespace lva
