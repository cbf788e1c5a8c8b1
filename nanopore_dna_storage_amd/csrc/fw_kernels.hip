// fw_kernels.hip -- DESIGN.md section 1 row N7, the forward score: what ALL alignments of a base sequence weigh on a read.
//
// The one-message trellis that sc_score runs (sc_frame.h) -- a band of positions x (flip b, flop b + 4) per block -- under
// a cell rule with two differences, both of the definition trellis_score.reference_forward:
//   sum for max    every maximum of terms prev + post becomes m + log(sum exp(term - m)), m the largest term, the terms in the
//                  definition's order, which is the frame's: a flip -- the stay, from flip b2 (if b2 != b), from flop b2 + 4
//                  (at p = 1: the stay, then the seven other states of position 0 ascending); a flop -- the stay, the step
//                  from flip b.  The largest term's exp is 1 and is not evaluated: a flip costs two expf and one logf, a
//                  flop one of each.  A single finite term comes back exactly (m + logf(1 + 0)); all -inf gives -inf, not
//                  NaN (the subtractions take 0 for m then).  expf / logf are the library's accurate ones: this is a float32
//                  stage, held to twice the error of the definition's float32 restatement
//                  (tests/test_gpu_trellis_forward.py), and the additions stay single float32 additions (no FMA contraction).
//   cleared band   a cell outside its block's band is -inf.  The frame's parity buffers are never cleared: what the frame
//                  reads of `prev` the rule tests against the band of the block BEFORE (carried from step to step in a
//                  scalar; before block 0 every position holds its initial state) and takes -inf outside it -- the result,
//                  read after the last block, included.  Nothing is written for a position that leaves the band.
//
//   fw_forward  sc_frame under FwRule.
//
// LDS ordering: the frame's (sc_frame.h), unchanged by the band test, which is lane-local and reads nothing.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fw_kernels.h"
#include "sc_frame.h"

namespace lva {

namespace {

// log(exp(x1) + exp(x2)): 1 + e is e_1 + e_2 in either order
__device__ inline float lse2(float x1, float x2) {
  const float m = hi_of(x1, x2), l = x1 < x2 ? x1 : x2;
  const float e = expf(l - (m == kNegInf ? 0.0f : m));
  return m + logf(1.0f + e);
}

// log(exp(x1) + exp(x2) + exp(x3)), summed (e_1 + e_2) + e_3; the first largest term's e is 1, the two others are evaluated
__device__ inline float lse3(float x1, float x2, float x3) {
  const float m = hi_of(hi_of(x1, x2), x3), mm = m == kNegInf ? 0.0f : m;
  const bool a1 = x1 == m, a12 = a1 || x2 == m;
  const float d1 = x1 - mm, d2 = x2 - mm, d3 = x3 - mm;
  const float u = expf(a1 ? d2 : d1), v = expf(a12 ? d3 : d2);
  const float e1 = a1 ? 1.0f : u, e2 = a1 ? u : (a12 ? 1.0f : v), e3 = a12 ? v : 1.0f;
  return m + logf((e1 + e2) + e3);
}

// log-sum-exp for ScRule's maxima, and the cleared band on read
struct FwRule : ScRule {
  int plo = 0, phi = 1 << 16;      // the band of the block before: all of the initial state (no band word's hi reaches 1 << 16)
  bool zlive = true;               // position 0 was inside it

  __device__ float zero_of(float v) const { return zlive ? v : kNegInf; }
  __device__ float2 cell_of(float2 v, int p) const { return p < plo || p >= phi ? make_float2(kNegInf, kNegInf) : v; }
  __device__ float flip_first(float stay, const float (&x)[8], uint32_t b) const {
    float m = stay;
#pragma unroll
    for (uint32_t s = 0; s < 8; ++s)
      if (s != b) m = hi_of(m, x[s]);
    const float mm = m == kNegInf ? 0.0f : m;
    float sum = expf(stay - mm);
#pragma unroll
    for (uint32_t s = 0; s < 8; ++s)
      if (s != b) sum += expf(x[s] - mm);
    return m == kNegInf ? kNegInf : m + logf(sum);
  }
  __device__ float flip_of(float stay, float from_flip, float from_flop, uint32_t) const { return lse3(stay, from_flip, from_flop); }
  __device__ float flop_of(float stay, float step) const { return lse2(stay, step); }
  __device__ void block_begins(int) { zlive = plo == 0 && phi > 0; }
  __device__ void block_ends(int lo, int hi) { plo = lo; phi = hi; }
};

// grid = pairs, block = one wavefront; dynamic LDS: fw_lds_bytes(max_len), cap = sc_lds_positions(max_len)
__global__ __launch_bounds__(64) void fw_forward(const float* __restrict__ post, const uint8_t* __restrict__ bases,
                                                 const ScPair* __restrict__ pairs, const uint32_t* __restrict__ band, int cap,
                                                 float* __restrict__ out) {
  sc_frame(post, bases, pairs, band, cap, out, FwRule{});
}

}  // namespace

int launch_fw_forward(const float* post, const uint8_t* bases, const ScPair* pairs, const uint32_t* band, int32_t n_pairs,
                      int32_t max_len, float* out, void* stream) {
  if (n_pairs <= 0) return 0;
  hipLaunchKernelGGL(fw_forward, dim3(n_pairs), dim3(64), fw_lds_bytes(max_len), (hipStream_t)stream, post, bases, pairs, band,
                     (int)sc_lds_positions(max_len), out);
  return (int)hipGetLastError();
}

}  // namespace lva
