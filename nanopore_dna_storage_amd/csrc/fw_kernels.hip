// fw_kernels.hip -- DESIGN.md section 1 row N7, the forward score: what ALL alignments of a base sequence weigh on a read.
//
// sc_score's trellis (sc_kernels.hip) -- one message, so a band of positions x (flip b, flop b + 4) per block -- with two
// differences, both of the definition trellis_score.reference_forward:
//   sum for max    every maximum of terms prev + post becomes m + log(sum exp(term - m)), m the largest term, the terms in the
//                  definition's order: a flip -- the stay, from flip b2 (if b2 != b), from flop b2 + 4 (at p = 1: the stay,
//                  then the seven other states of position 0 ascending); a flop -- the stay, the step from flip b.  The
//                  largest term's exp is 1 and is not evaluated: a flip costs two expf and one logf, a flop one of each.
//                  A single finite term comes back exactly (m + logf(1 + 0)); all -inf gives -inf, not NaN (the
//                  subtractions take 0 for m then).  expf / logf are the library's accurate ones: this is a float32 stage,
//                  held to twice the error of the definition's float32 restatement (tests/test_gpu_trellis_forward.py), and
//                  the additions stay single float32 additions in the definition's order (no FMA contraction).
//   cleared band   a cell outside its block's band is -inf.  The parity buffers are sc_score's and are not cleared either:
//                  a lane that reads prev[p] or prev[p - 1] tests that position against the band of the block BEFORE
//                  (carried from step to step in a scalar; before block 0 every position holds its initial state) and takes
//                  -inf outside it.  Nothing is written for a position that leaves the band.
//
//   fw_forward  one wavefront per (read, sequence) pair, lanes over the positions of the block's band in passes of 64, both
//               parity buffers in LDS, posterior rows and band words staged kScStage at a time: sc_score's frame.
//
// LDS ordering: sc_score's argument, unchanged by the band test, which is lane-local and reads no more than sc_score does.
// In a step a lane reads the buffer of parity t & 1 (its own position and the one below) and the staged row, and writes
// the other parity at its own position: within a step nothing that is written is read, passes included.  Two things need
// an order and get a workgroup barrier (the workgroup is the wavefront: the compiler drops the barrier instruction and
// keeps its fences): (1) a step's stores before the next step's loads of that buffer -- the barrier that ends every step,
// which also keeps the last reads of the staged rows ahead of the next chunk's staging stores; (2) the staging stores (and
// the initial state) before the first step that reads them.  Control flow around every barrier is uniform: the band, the
// block count and the chunk are the wavefront's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fw_kernels.h"

namespace lva {

namespace {

constexpr float kNegInf = -__builtin_huge_valf();

// the larger of two scores, neither of them NaN: one compare and select
__device__ inline float hi_of(float a, float b) { return a < b ? b : a; }

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

// grid = pairs, block = one wavefront; dynamic LDS: fw_lds_bytes(max_len), cap = sc_lds_positions(max_len)
__global__ __launch_bounds__(64) void fw_forward(const float* __restrict__ post, const uint8_t* __restrict__ bases,
                                                 const ScPair* __restrict__ pairs, const uint32_t* __restrict__ band, int cap,
                                                 float* __restrict__ out) {
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
  if (lane < 8) { zero[lane] = 0.0f; zero[8 + lane] = kNegInf; }       // the buffer that the first swap makes `prev`

  const float* rows = post + (size_t)pr.row0 * 40;
  int plo = 0, phi = npos;                                              // the band of the block before: all of the initial state
  for (int t0 = 0; t0 < nblk; t0 += kScStage) {
    const int nrows = min(kScStage, nblk - t0);
    for (int i = lane; i < nrows * 40; i += 64) stage[i] = rows[(size_t)t0 * 40 + i];
    const uint32_t my_band = lane < nrows ? band[pr.band_at + t0 + lane] : 0u;
    __syncthreads();                                                    // (2)
    for (int u = 0; u < nrows; ++u) {
      const uint32_t bw = __builtin_amdgcn_readlane(my_band, u);
      const int lo = (int)(bw & 0xFFFFu), hi = (int)(bw >> 16);
      const int from = ((t0 + u) & 1), to = from ^ 1;                   // prev = buffer t & 1, cur the other
      const float* row = stage + u * 40;
      const float2* prev = st + (size_t)from * cap;
      float2* cur = st + (size_t)to * cap;
      const float* zprev = zero + from * 8;
      const bool zlive = plo == 0 && phi > 0;                           // position 0 was inside the band of the block before
      for (int p = lo + lane; p < hi; p += 64) {
        if (p == 0) {                                                   // stays only: a plain addition
          float* zcur = zero + to * 8;
#pragma unroll
          for (int k = 0; k < 8; ++k) zcur[k] = (zlive ? zprev[k] : kNegInf) + row[k < 4 ? k * 8 + k : 32 + k];
          continue;
        }
        const uint32_t c = bb[p], b = c & 3u, b2 = (c >> 2) & 3u;
        float2 me = prev[p];
        if (p < plo || p >= phi) me = make_float2(kNegInf, kNegInf);    // the cleared band, on read
        const float stay = me.x + row[b * 8 + b];
        float flip, step;
        if (p == 1) {                                                   // the stay, then every state of position 0 but flip b
          float x[8], m = stay;                                         // (x[b] is no term; unrolled: registers)
#pragma unroll
          for (uint32_t s = 0; s < 8; ++s) {
            x[s] = (zlive ? zprev[s] : kNegInf) + row[b * 8 + s];
            if (s != b) m = hi_of(m, x[s]);
          }
          const float mm = m == kNegInf ? 0.0f : m;
          float sum = expf(stay - mm);
#pragma unroll
          for (uint32_t s = 0; s < 8; ++s)
            if (s != b) sum += expf(x[s] - mm);
          flip = m == kNegInf ? kNegInf : m + logf(sum);
          step = zlive ? zprev[b] : kNegInf;
        } else {                                                        // the position below holds flip b2 and flop b2 + 4 alone
          float2 below = prev[p - 1];
          if (p - 1 < plo || p - 1 >= phi) below = make_float2(kNegInf, kNegInf);
          flip = lse3(stay, (b2 != b ? below.x : kNegInf) + row[b * 8 + b2], below.y + row[b * 8 + b2 + 4]);
          step = b2 == b ? below.x : kNegInf;                           // flop b + 4 is entered from flip b only
        }
        const float flop = lse2(me.y + row[32 + b + 4], step + row[32 + b]);
        cur[p] = make_float2(flip, flop);
      }
      plo = lo;
      phi = hi;
      __syncthreads();                                                  // (1)
    }
  }
  if (lane == 0) {
    const bool live = npos - 1 >= plo && npos - 1 < phi;                // the last position inside the last block's band
    const float2 r = st[(size_t)(nblk & 1) * cap + npos - 1];           // `cur` after the last block
    out[(size_t)blockIdx.x * 2] = live ? r.x : kNegInf;
    out[(size_t)blockIdx.x * 2 + 1] = live ? r.y : kNegInf;
  }
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
