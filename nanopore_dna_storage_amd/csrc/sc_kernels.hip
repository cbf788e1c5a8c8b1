// sc_kernels.hip -- DESIGN.md section 1 row N7: what a given base sequence scores on a read.
//
// The definition is trellis_score.reference_score; the device is held to it bit for bit (tests/test_gpu_trellis_score.py):
// single float32 additions, exact maxima, no FMA.
//
//   sc_score   the one-message trellis of sc_frame.h (one wavefront per pair, the LDS, the staging, the barriers and the
//              argument for them: there) under its plain cell rule ScRule: every cell the maximum of its terms.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sc_frame.h"

namespace lva {

namespace {

// grid = pairs, block = one wavefront; dynamic LDS: sc_lds_bytes(max_len), cap = sc_lds_positions(max_len)
__global__ __launch_bounds__(64) void sc_score(const float* __restrict__ post, const uint8_t* __restrict__ bases,
                                               const ScPair* __restrict__ pairs, const uint32_t* __restrict__ band, int cap,
                                               float* __restrict__ out) {
  sc_frame(post, bases, pairs, band, cap, out, ScRule{});
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
