// philox.h -- Philox4x32-10 on the device, for every kernel that draws: counter (item, sub, number, stream) under the
// 64-bit seed as key (low word, high word).  nanopore_dna_storage_amd/philox.py is the same function in numpy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lva {

// the streams: 0..4 and 6 the read simulator (simulate.py), 5 the trial order (trials.py)
constexpr uint32_t kStreamMessage = 0, kStreamChannel = 1, kStreamDwell = 2, kStreamNoise = 3, kStreamLead = 4, kStreamTrial = 5,
                   kStreamSource = 6;

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(kPhiloxM0, c0), l0 = kPhiloxM0 * c0, h1 = __umulhi(kPhiloxM1, c2), l1 = kPhiloxM1 * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += kPhiloxW0; k1 += kPhiloxW1;
  }
  return {c0, c1, c2, c3};
}

}  // namespace lva
