// ls_bucket.h -- what the per-index kernels share: the listing step -- ls_consensus (ls_kernels.hip) lists and votes in
// one launch, tr_bucket_list (tr_kernels.hip) lists once for the many trials that vote afterwards -- and the comparison
// of two payloads that both votes count with.
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

// what a vote compares: the n payload bytes of two reads
__device__ __forceinline__ bool same_payload(const uint8_t* a, const uint8_t* b, int n) {
  for (int k = 0; k < n; ++k)
    if (a[k] != b[k]) return false;
  return true;
}

}  // namespace lva
