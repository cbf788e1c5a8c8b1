// sc_frame.h -- device only: the one-message trellis of DESIGN.md section 1 row N7, everything that sc_score (sc_kernels.hip),
// st_fill (st_kernels.hip) and fw_forward (fw_kernels.hip) share, as one function over a cell rule.
//
// A path of the reference trellis (decode_post_conv_parallel_LVA, :589-858) that carries one message walks that message's
// convolutional states, so per time step a band of positions x the flip-flop states is left, and of a position's eight
// states only flip b and flop b + 4 of its base b are ever finite.
//
//   sc_frame   one wavefront per (read, sequence) pair, lanes over the positions of the block's band, in passes of 64 where
//              the band is wider (the unbanded default).  Both parity buffers of the pair live in LDS and, as in the
//              reference, are never cleared: a position outside a block's band keeps what it held.  Posterior rows go
//              through LDS kScStage at a time, loaded by consecutive lanes from consecutive floats; the band words of
//              those rows are loaded with them, one per lane, and handed out by readlane.
//              The frame forms every term prev + row[...] itself, one float32 addition each, and hands the terms of a cell
//              to the rule in the definition's order; the rule says how they combine (ScRule below: what a rule may change).
//
// LDS ordering.  In a step a lane reads the buffer of parity t & 1 (its own position and the one below) and the staged row,
// and writes the other parity at its own position: within a step nothing that is written is read, passes included.  Two
// things need an order and get a workgroup barrier (the workgroup is the wavefront, so the compiler drops the barrier
// instruction and keeps its fences: the wait for the LDS counter, and the rule that a step's loads are not moved above
// the stores of the step before, which it may otherwise do -- another address of the same lane): (1) a step's stores
// before the next step's loads of that buffer -- the barrier that ends every step, which also keeps the last reads of the
// staged rows ahead of the next chunk's staging stores; (2) the staging stores (and the initial state) before the first
// step that reads them.  Control flow around every barrier is uniform: the band, the block count and the chunk are the
// wavefront's.  No hook of a rule touches LDS: what a rule reads of the buffers is handed to it, so the argument holds for
// every rule.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sc_kernels.h"

namespace lva {

constexpr float kNegInf = -__builtin_huge_valf();

// the larger of two scores, neither of them NaN (the definition excludes NaN): one compare and select, no canonicalisation
__device__ __forceinline__ float hi_of(float a, float b) { return a < b ? b : a; }

// The cell rule of sc_score, and the base of the others: maxima, nothing masked, nothing beside the scores.
struct ScRule {
  // what a value read from `prev` counts as: a state of position 0, (flip, flop) of position p >= 1
  __device__ float zero_of(float v) const { return v; }
  __device__ float2 cell_of(float2 v, int /*p*/) const { return v; }
  // flip b at p == 1: the stay, and x[s] from state s of position 0 -- x[b] is no term (flip b never enters flip b)
  __device__ float flip_first(float stay, const float (&x)[8], uint32_t b) const {
    float flip = stay;
#pragma unroll
    for (uint32_t s = 0; s < 8; ++s)
      if (s != b) flip = hi_of(flip, x[s]);
    return flip;
  }
  // flip b at p >= 2: the stay, from flip b2 (-inf if b2 == b) and from flop b2 + 4 of the position below
  __device__ float flip_of(float stay, float from_flip, float from_flop, uint32_t /*b2*/) const { return hi_of(hi_of(stay, from_flip), from_flop); }
  // flop b + 4: the stay, and the step from flip b below
  __device__ float flop_of(float stay, float step) const { return hi_of(stay, step); }
  // uniform, around the passes of block t with band [lo, hi); per cell, after the store of position p
  __device__ void block_begins(int /*t*/) {}
  __device__ void block_ends(int /*lo*/, int /*hi*/) {}
  __device__ void stored(int /*p*/, int /*lo*/) const {}
};

// grid = pairs, block = one wavefront; dynamic LDS: sc_lds_bytes(max_len), cap = sc_lds_positions(max_len)
template <class Rule>
__device__ __forceinline__ void sc_frame(const float* __restrict__ post, const uint8_t* __restrict__ bases,
                                         const ScPair* __restrict__ pairs, const uint32_t* __restrict__ band, int cap,
                                         float* __restrict__ out, Rule rule) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* stage = reinterpret_cast<float*>(smem);                        // [kScStage][40]
  float* zero = stage + kScStage * 40;                                  // [2][8]: position 0, every state
  float2* st = reinterpret_cast<float2*>(zero + 16);                    // [2][cap]: (flip b, flop b + 4) of position p >= 1
  uint8_t* bb = reinterpret_cast<uint8_t*>(st + 2 * (size_t)cap);       // [cap]: base of p | base of p - 1 << 2

  const int lane = threadIdx.x;
  const ScPair pr = pairs[blockIdx.x];
  const int npos = (int)pr.len + 1, nblk = (int)pr.nblk;

  for (int p = lane; p < npos; p += 64) {
    st[p] = make_float2(kNegInf, kNegInf);
    st[cap + p] = make_float2(kNegInf, kNegInf);
    const uint32_t b = p >= 1 ? base_code(bases[pr.seq_off + p - 1]) & 3u : 0u;
    const uint32_t b2 = p >= 2 ? base_code(bases[pr.seq_off + p - 2]) & 3u : 0u;
    bb[p] = (uint8_t)(b | b2 << 2);
  }
  if (lane < 8) { zero[lane] = 0.0f; zero[8 + lane] = kNegInf; }       // :657-663 on the buffer that the first swap makes `prev`

  const float* rows = post + (size_t)pr.row0 * 40;
  for (int t0 = 0; t0 < nblk; t0 += kScStage) {
    const int nrows = min(kScStage, nblk - t0);
    for (int i = lane; i < nrows * 40; i += 64) stage[i] = rows[(size_t)t0 * 40 + i];
    const uint32_t my_band = lane < nrows ? band[pr.band_at + t0 + lane] : 0u;
    __syncthreads();                                                    // (2)
    for (int u = 0; u < nrows; ++u) {
      const uint32_t bw = __builtin_amdgcn_readlane(my_band, u);
      const int lo = (int)(bw & 0xFFFFu), hi = (int)(bw >> 16);
      const int from = ((t0 + u) & 1), to = from ^ 1;                   // prev = buffer t & 1, cur the other (:669-670)
      const float* row = stage + u * 40;
      const float2* prev = st + (size_t)from * cap;
      float2* cur = st + (size_t)to * cap;
      const float* zprev = zero + from * 8;
      rule.block_begins(t0 + u);
      for (int p = lo + lane; p < hi; p += 64) {
        if (p == 0) {                                                   // stays only, a plain addition (:706-713)
          float* zcur = zero + to * 8;
#pragma unroll
          for (int k = 0; k < 8; ++k) zcur[k] = rule.zero_of(zprev[k]) + row[k < 4 ? k * 8 + k : 32 + k];
          rule.stored(0, lo);
          continue;
        }
        const uint32_t c = bb[p], b = c & 3u, b2 = (c >> 2) & 3u;
        const float2 me = rule.cell_of(prev[p], p);
        const float stay = me.x + row[b * 8 + b];
        float flip, step;
        if (p == 1) {                                                   // from every state of position 0 but flip b
          float x[8];                                                   // (unrolled: registers)
#pragma unroll
          for (uint32_t s = 0; s < 8; ++s) x[s] = rule.zero_of(zprev[s]) + row[b * 8 + s];
          flip = rule.flip_first(stay, x, b);
          step = rule.zero_of(zprev[b]);
        } else {                                                        // the position below holds flip b2 and flop b2 + 4 alone
          const float2 below = rule.cell_of(prev[p - 1], p - 1);        // (no branch: flip b never enters flip b, -inf says so)
          flip = rule.flip_of(stay, (b2 != b ? below.x : kNegInf) + row[b * 8 + b2], below.y + row[b * 8 + b2 + 4], b2);
          step = b2 == b ? below.x : kNegInf;                           // flop b + 4 is entered from flip b only (:879-881)
        }
        const float flop = rule.flop_of(me.y + row[32 + b + 4], step + row[32 + b]);
        cur[p] = make_float2(flip, flop);
        rule.stored(p, lo);
      }
      rule.block_ends(lo, hi);
      __syncthreads();                                                  // (1)
    }
  }
  if (lane == 0) {                                                      // `cur` after the last block (:806-824), read as the
    const float2 r = rule.cell_of(st[(size_t)(nblk & 1) * cap + npos - 1], npos - 1);   // `prev` of a block after it would be
    out[(size_t)blockIdx.x * 2] = r.x;
    out[(size_t)blockIdx.x * 2 + 1] = r.y;
  }
}

}  // namespace lva
