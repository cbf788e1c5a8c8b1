// ls_bucket.h -- the listing step the per-index kernels share: ls_consensus (ls_kernels.hip) lists and votes in one
// launch, tr_bucket_list (tr_kernels.hip) lists once for the many trials that vote afterwards.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lva {

// One wavefront lists the t reads of index x in read order into mem [t]: a ballot over 64 reads at a time, each hit
// placed behind the hits of lower lanes.
__device__ __forceinline__ void list_bucket(const int32_t* __restrict__ index, int n_reads, int x, int t, int32_t* __restrict__ mem,
                                            int lane) {
  int pos = 0;
  for (int i0 = 0; i0 < n_reads && pos < t; i0 += 64) {
    const int i = i0 + lane;
    const bool m = i < n_reads && index[i] == x;
    const unsigned long long mask = __ballot(m);
    const int at = pos + __popcll(mask & ((1ull << lane) - 1ull));
    if (m && at < t) mem[at] = i;
    pos += __popcll(mask);
  }
}

}  // namespace lva
