// sim_pool_kernels.hip -- the read simulator's pool source: sim_strand with the message of a
// read taken from a pool of given messages, the entry and the orientation drawn by stream 6 (simulate.py).  The kernel is
// sim_strand.h's body with kPool set; sim_scores (sim_kernels.hip) serves both.
#include <hip/hip_runtime.h>

#include "sim_strand.h"

namespace lva {

namespace {

__global__ __launch_bounds__(64) void sim_strand_pool(SimParams p, SimPool pl, const uint16_t* __restrict__ posinfo,
                                                      const uint32_t* __restrict__ cdf, const uint8_t* __restrict__ bc,
                                                      const int64_t* __restrict__ row_off, const int64_t* __restrict__ base_off,
                                                      int32_t* __restrict__ lens, uint8_t* __restrict__ msgs,
                                                      uint8_t* __restrict__ bases, uint8_t* __restrict__ true_idx,
                                                      int32_t* __restrict__ bad) {
  sim_strand_body<true>(p, pl, posinfo, cdf, bc, row_off, base_off, lens, msgs, bases, true_idx, bad);
}

}  // namespace

int launch_sim_strand_pool(const SimParams& p, const SimPool& pool, int32_t n_reads, const uint16_t* posinfo, const uint32_t* cdf,
                           const uint8_t* bc, const int64_t* row_off, const int64_t* base_off, int32_t* lens, uint8_t* msgs,
                           uint8_t* bases, uint8_t* true_idx, int32_t* bad, void* stream) {
  if (n_reads <= 0) return 0;
  hipLaunchKernelGGL(sim_strand_pool, dim3((uint32_t)n_reads), dim3(64), 0, (hipStream_t)stream, p, pool, posinfo, cdf, bc, row_off,
                     base_off, lens, msgs, bases, true_idx, bad);
  return (int)hipGetLastError();
}

}  // namespace lva
