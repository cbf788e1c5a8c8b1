// sc_kernels.hip -- DESIGN.md section 1 row N7: what a given base sequence scores on a read.
//
// A path of the reference trellis (decode_post_conv_parallel_LVA, :589-858) that carries one message walks that message's
// convolutional states, so per time step a band of positions x the flip-flop states is left, and of a position's eight
// states only flip b and flop b + 4 of its base b are ever finite.  The definition is trellis_score.reference_score; the
// device is held to it bit for bit (tests/test_gpu_trellis_score.py): single float32 additions, exact maxima, no FMA.
//
//   sc_score   one wavefront per (read, sequence) pair, lanes over the positions of the block's band, in passes of 64 where
//              the band is wider (the unbanded default).  Both parity buffers of the pair live in LDS and, as in the
//              reference, are never cleared: a position outside a block's band keeps what it held.  Posterior rows go
//              through LDS kScStage at a time, loaded by consecutive lanes from consecutive floats; the band words of
//              those rows are loaded with them, one per lane, and handed out by readlane.
//
// LDS ordering.  In a step a lane reads the buffer of parity t & 1 (its own position and the one below) and the staged row,
// and writes the other parity at its own position: within a step nothing that is written is read, passes included.  Two
// things need an order and get a workgroup barrier (the workgroup is the wavefront, so the compiler drops the barrier
// instruction and keeps its fences: the wait for the LDS counter, and the rule that a step's loads are not moved above
// the stores of the step before, which it may otherwise do -- another address of the same lane): (1) a step's stores
// before the next step's loads of that buffer -- the barrier that ends every step, which also keeps the last reads of the
// staged rows ahead of the next chunk's staging stores; (2) the staging stores (and the initial state) before the first
// step that reads them.  Control flow around every barrier is uniform: the band, the block count and the chunk are the
// wavefront's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sc_kernels.h"

namespace lva {

namespace {

constexpr float kNegInf = -__builtin_huge_valf();

// the larger of two scores, neither of them NaN (the definition excludes NaN): one compare and select, no canonicalisation
__device__ inline float hi_of(float a, float b) { return a < b ? b : a; }

// grid = pairs, block = one wavefront; dynamic LDS: sc_lds_bytes(max_len), cap = sc_lds_positions(max_len)
__global__ __launch_bounds__(64) void sc_score(const float* __restrict__ post, const uint8_t* __restrict__ bases,
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
      for (int p = lo + lane; p < hi; p += 64) {
        if (p == 0) {                                                   // stays only (:706-713)
          float* zcur = zero + to * 8;
#pragma unroll
          for (int k = 0; k < 8; ++k) zcur[k] = zprev[k] + row[k < 4 ? k * 8 + k : 32 + k];
          continue;
        }
        const uint32_t c = bb[p], b = c & 3u, b2 = (c >> 2) & 3u;
        const float2 me = prev[p];
        float flip = me.x + row[b * 8 + b], step;
        if (p == 1) {                                                   // from every state of position 0 but flip b
#pragma unroll
          for (uint32_t s = 0; s < 8; ++s)
            if (s != b) flip = hi_of(flip, zprev[s] + row[b * 8 + s]);
          step = zprev[b];
        } else {                                                        // the position below holds flip b2 and flop b2 + 4 alone
          const float2 below = prev[p - 1];                             // (no branch: flip b never enters flip b, -inf says so)
          flip = hi_of(flip, (b2 != b ? below.x : kNegInf) + row[b * 8 + b2]);
          flip = hi_of(flip, below.y + row[b * 8 + b2 + 4]);
          step = b2 == b ? below.x : kNegInf;                           // flop b + 4 is entered from flip b only (:879-881)
        }
        const float flop = hi_of(me.y + row[32 + b + 4], step + row[32 + b]);
        cur[p] = make_float2(flip, flop);
      }
      __syncthreads();                                                  // (1)
    }
  }
  if (lane == 0) {
    const float2 r = st[(size_t)(nblk & 1) * cap + npos - 1];           // `cur` after the last block (:806-824)
    out[(size_t)blockIdx.x * 2] = r.x;
    out[(size_t)blockIdx.x * 2 + 1] = r.y;
  }
}

}  // namespace

int launch_sc_score(const float* post, const uint8_t* bases, const ScPair* pairs, const uint32_t* band, int32_t n_pairs,
                    int32_t max_len, float* out, void* stream) {
  if (n_pairs <= 0) return 0;
  hipLaunchKernelGGL(sc_score, dim3(n_pairs), dim3(64), sc_lds_bytes(max_len), (hipStream_t)stream, post, bases, pairs, band,
                     (int)sc_lds_positions(max_len), out);
  return (int)hipGetLastError();
}

}  // namespace lva
