// mi_kernels.hip -- DESIGN.md section 1 row N6: the read-mapping index built on the device (mi_kernels.h lists the steps).
//
// The host builder sorts every (k-mer, oligo) pair and walks all 4^k table entries on one core; here the table is a
// histogram.  What makes it exact:
//   distinct   an oligo counts a k-mer once however often it repeats it.  mi_count and mi_fill hold the oligo's k-mers in
//              LDS, one per position (kMiNoKmer where the k bytes are not all bases), and a position speaks for its k-mer
//              only if no earlier position holds the same one: a wavefront per oligo, the lanes read the same earlier
//              position at the same time (a broadcast), at most 1019 of them;
//   scan       whole tiles of kMiScanTile counters (4^k is a multiple of it for every k): a sum per tile, one workgroup
//              that scans the sums, a pass that scans each tile again on top of its sum.  Three launches on one stream:
//              the order of the launches is the only synchronisation;
//   order      mi_fill takes a slot of the segment from an atomic, so a segment's order is the order the atomics ran in.
//              The oligos of a segment are distinct, so an oligo's place in the ascending order is the number of smaller
//              ones in the segment: mi_rank counts them, a thread per pair, and writes the pair there.  No two pairs get
//              the same place, every place is taken, and two builds of the same input give the same bytes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mi_kernels.h"

namespace lva {

namespace {

constexpr int kWaves = kMiThreads / 64;

// ---------------------------------------------------------------- masks

// a thread per (oligo, direction, word): the four base words of 64 rows
__global__ __launch_bounds__(kMiThreads) void mi_masks(const uint8_t* __restrict__ refs, const int64_t* __restrict__ ref_off, size_t n_words,
                                                       int W, uint64_t* __restrict__ masks) {
  for (size_t t = (size_t)blockIdx.x * kMiThreads + threadIdx.x; t < n_words; t += (size_t)gridDim.x * kMiThreads) {
    const int w = (int)(t % (size_t)W);
    const size_t od = t / (size_t)W;             // oligo * 2 + reversed
    const size_t o = od >> 1;
    const bool reversed = od & 1;
    const uint8_t* ref = refs + ref_off[o];
    const int m = (int)(ref_off[o + 1] - ref_off[o]);
    uint64_t word[4] = {0, 0, 0, 0};
    for (int i = 0; i < 64; ++i) {
      const int pos = 64 * w + i;
      if (pos >= m) break;
      const uint32_t c = base_code(ref[reversed ? m - 1 - pos : pos]);
#pragma unroll
      for (int b = 0; b < 4; ++b) word[b] |= (uint64_t)(c == (uint32_t)b) << i;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) masks[(od * 4 + b) * (size_t)W + w] = word[b];
  }
}

// ---------------------------------------------------------------- an oligo's distinct k-mers

// the oligo as codes, then the k-mer that starts at every position 0 .. m - k; ends with the workgroup in step
__device__ __forceinline__ void oligo_kmers(const uint8_t* __restrict__ ref, int m, int k, uint8_t* s_base, uint32_t* s_kmer) {
  for (int i = threadIdx.x; i < m; i += kMiOligoThreads) s_base[i] = (uint8_t)base_code(ref[i]);
  __syncthreads();
  for (int i = threadIdx.x; i + k <= m; i += kMiOligoThreads) {
    uint32_t kmer = 0, n = 0;
    for (int j = 0; j < k; ++j) {
      const uint32_t c = s_base[i + j];
      n |= c >> 2;
      kmer = (kmer << 2) | (c & 3u);
    }
    s_kmer[i] = n ? kMiNoKmer : kmer;
  }
  __syncthreads();
}

// position i speaks for its k-mer: it has one, and no earlier position has the same
__device__ __forceinline__ bool first_of_its_kmer(const uint32_t* s_kmer, int i) {
  const uint32_t kmer = s_kmer[i];
  if (kmer == kMiNoKmer) return false;
  for (int j = 0; j < i; ++j)
    if (s_kmer[j] == kmer) return false;
  return true;
}

__global__ __launch_bounds__(kMiOligoThreads) void mi_count(const uint8_t* __restrict__ refs, const int64_t* __restrict__ ref_off, int n_refs,
                                                            int k, uint32_t* __restrict__ counts) {
  __shared__ uint8_t s_base[kMaxRef];
  __shared__ uint32_t s_kmer[kMaxRef];
  for (int o = blockIdx.x; o < n_refs; o += gridDim.x) {
    const int m = (int)(ref_off[o + 1] - ref_off[o]);
    if (m >= k && m <= kMaxRef) {                // (uniform in the workgroup)
      oligo_kmers(refs + ref_off[o], m, k, s_base, s_kmer);
      for (int i = threadIdx.x; i + k <= m; i += kMiOligoThreads)
        if (first_of_its_kmer(s_kmer, i)) atomicAdd(&counts[s_kmer[i]], 1u);
    }
    __syncthreads();                             // the next oligo overwrites the LDS
  }
}

// counts is the cursor of its segment: it holds what is left to place and ends at 0
__global__ __launch_bounds__(kMiOligoThreads) void mi_fill(const uint8_t* __restrict__ refs, const int64_t* __restrict__ ref_off, int n_refs,
                                                           int k, const uint32_t* __restrict__ offsets, uint32_t* __restrict__ counts,
                                                           int32_t* __restrict__ slot_oligo, uint32_t* __restrict__ slot_kmer) {
  __shared__ uint8_t s_base[kMaxRef];
  __shared__ uint32_t s_kmer[kMaxRef];
  for (int o = blockIdx.x; o < n_refs; o += gridDim.x) {
    const int m = (int)(ref_off[o + 1] - ref_off[o]);
    if (m >= k && m <= kMaxRef) {
      oligo_kmers(refs + ref_off[o], m, k, s_base, s_kmer);
      for (int i = threadIdx.x; i + k <= m; i += kMiOligoThreads) {
        if (!first_of_its_kmer(s_kmer, i)) continue;
        const uint32_t kmer = s_kmer[i];
        const uint32_t lo = offsets[kmer], len = offsets[kmer + 1] - lo;
        if (len == 0) continue;                  // dropped by max_occ
        const uint32_t left = atomicSub(&counts[kmer], 1u);
        if (left - 1u < len) {                   // (always: the segment was sized by the same count)
          slot_oligo[lo + left - 1u] = o;
          slot_kmer[lo + left - 1u] = kmer;
        }
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- clip, scan

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
  return v;                                      // lane 0 holds the sum
}

__global__ __launch_bounds__(kMiThreads) void mi_clip(uint32_t* __restrict__ counts, size_t table, uint32_t max_occ, uint32_t* __restrict__ stats) {
  __shared__ uint32_t s_part[2][kWaves];
  uint32_t kept = 0, dropped = 0;
  for (size_t c = (size_t)blockIdx.x * kMiThreads + threadIdx.x; c < table; c += (size_t)gridDim.x * kMiThreads) {
    const uint32_t v = counts[c];
    if (v > max_occ) {
      counts[c] = 0;
      ++dropped;
    } else if (v > 0) {
      ++kept;
    }
  }
  kept = wave_sum(kept);
  dropped = wave_sum(dropped);
  if ((threadIdx.x & 63) == 0) {
    s_part[0][threadIdx.x >> 6] = kept;
    s_part[1][threadIdx.x >> 6] = dropped;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) sum += s_part[threadIdx.x][w];
    if (sum) atomicAdd(&stats[threadIdx.x], sum);
  }
}

// the exclusive prefix sum of one value per thread over the workgroup, and the workgroup's sum; s_part may be reused after it
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* s_part, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) s_part[wave] = x;
  __syncthreads();
  uint32_t before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const uint32_t p = s_part[w];
    before += w < wave ? p : 0u;
    total += p;
  }
  __syncthreads();
  return before + x - v;
}

// a thread's 16 consecutive counters of tile `tile`
__device__ __forceinline__ void load_items(const uint32_t* __restrict__ counts, size_t tile, uint4 (&v)[4]) {
  const uint4* p = reinterpret_cast<const uint4*>(counts + tile * kMiScanTile + (size_t)threadIdx.x * 16);
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = p[q];
}
__device__ __forceinline__ uint32_t sum_items(const uint4 (&v)[4]) {
  uint32_t s = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) s += v[q].x + v[q].y + v[q].z + v[q].w;
  return s;
}

__global__ __launch_bounds__(kMiThreads) void mi_scan_sums(const uint32_t* __restrict__ counts, uint32_t* __restrict__ sums) {
  __shared__ uint32_t s_part[kWaves];
  uint4 v[4];
  load_items(counts, blockIdx.x, v);
  const uint32_t s = wave_sum(sum_items(v));
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) sum += s_part[w];
    sums[blockIdx.x] = sum;
  }
}

// one workgroup: sums becomes its own exclusive prefix sum, kMiThreads entries at a time; the total closes the offsets
__global__ __launch_bounds__(kMiThreads) void mi_scan_top(uint32_t* __restrict__ sums, uint32_t n_tiles, uint32_t* __restrict__ last_offset,
                                                          uint32_t* __restrict__ stats) {
  __shared__ uint32_t s_part[kWaves];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n_tiles; base += kMiThreads) {
    const uint32_t at = base + threadIdx.x;
    uint32_t total;
    const uint32_t before = block_exclusive_scan(at < n_tiles ? sums[at] : 0u, s_part, total);
    if (at < n_tiles) sums[at] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) {
    *last_offset = carry;
    stats[2] = carry;
  }
}

__global__ __launch_bounds__(kMiThreads) void mi_scan_add(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ sums,
                                                          uint32_t* __restrict__ offsets) {
  __shared__ uint32_t s_part[kWaves];
  uint4 v[4];
  load_items(counts, blockIdx.x, v);
  uint32_t total;
  uint32_t run = sums[blockIdx.x] + block_exclusive_scan(sum_items(v), s_part, total);
  uint4* out = reinterpret_cast<uint4*>(offsets + (size_t)blockIdx.x * kMiScanTile + (size_t)threadIdx.x * 16);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint4 o;
    o.x = run; run += v[q].x;
    o.y = run; run += v[q].y;
    o.z = run; run += v[q].z;
    o.w = run; run += v[q].w;
    out[q] = o;
  }
}

// ---------------------------------------------------------------- rank

__global__ __launch_bounds__(kMiThreads) void mi_rank(const int32_t* __restrict__ slot_oligo, const uint32_t* __restrict__ slot_kmer,
                                                      uint32_t pairs, uint32_t table, const uint32_t* __restrict__ offsets,
                                                      int32_t* __restrict__ lists) {
  for (size_t p = (size_t)blockIdx.x * kMiThreads + threadIdx.x; p < pairs; p += (size_t)gridDim.x * kMiThreads) {
    const uint32_t kmer = slot_kmer[p];
    if (kmer >= table) continue;                 // (never: mi_fill wrote every slot)
    const uint32_t lo = offsets[kmer], hi = offsets[kmer + 1];
    if (p < lo || p >= hi || hi > pairs) continue;
    const int32_t me = slot_oligo[p];
    uint32_t smaller = 0;
    for (uint32_t q = lo; q < hi; ++q) smaller += slot_oligo[q] < me ? 1u : 0u;
    lists[lo + smaller] = me;                    // smaller <= hi - lo - 1: me is not smaller than itself
  }
}

int grid_for(size_t items, int threads) {        // a thread per item, grid-stride past 2^20 workgroups
  const size_t blocks = (items + (size_t)threads - 1) / (size_t)threads;
  return (int)(blocks < ((size_t)1 << 20) ? blocks : ((size_t)1 << 20));
}

}  // namespace

int launch_mi_masks(const uint8_t* refs, const int64_t* ref_off, int32_t n_refs, int32_t ref_len, uint64_t* masks, void* stream) {
  if (n_refs <= 0 || ref_len <= 0) return 0;
  const int W = (ref_len + 63) / 64;
  const size_t n_words = (size_t)n_refs * 2 * (size_t)W;
  hipLaunchKernelGGL(mi_masks, dim3(grid_for(n_words, kMiThreads)), dim3(kMiThreads), 0, (hipStream_t)stream, refs, ref_off, n_words, W, masks);
  return (int)hipGetLastError();
}

int launch_mi_count(const uint8_t* refs, const int64_t* ref_off, int32_t n_refs, int32_t k, uint32_t* counts, void* stream) {
  if (n_refs <= 0) return 0;
  if (k < kMpMinK || k > kMpMaxK) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(mi_count, dim3(grid_for((size_t)n_refs, 1)), dim3(kMiOligoThreads), 0, (hipStream_t)stream, refs, ref_off, n_refs, k, counts);
  return (int)hipGetLastError();
}

int launch_mi_clip(uint32_t* counts, int32_t k, int32_t max_occ, uint32_t* stats, void* stream) {
  if (k < kMpMinK || k > kMpMaxK || max_occ < 0) return (int)hipErrorInvalidValue;
  const int blocks = (int)(mi_table(k) / kMiScanTile < 2048 ? mi_table(k) / kMiScanTile : 2048);
  hipLaunchKernelGGL(mi_clip, dim3(blocks), dim3(kMiThreads), 0, (hipStream_t)stream, counts, mi_table(k), (uint32_t)max_occ, stats);
  return (int)hipGetLastError();
}

int launch_mi_scan(const uint32_t* counts, int32_t k, uint32_t* sums, uint32_t* offsets, uint32_t* stats, void* stream) {
  if (k < kMpMinK || k > kMpMaxK) return (int)hipErrorInvalidValue;
  const uint32_t n_tiles = (uint32_t)mi_scan_tiles(k);
  hipLaunchKernelGGL(mi_scan_sums, dim3(n_tiles), dim3(kMiThreads), 0, (hipStream_t)stream, counts, sums);
  hipLaunchKernelGGL(mi_scan_top, dim3(1), dim3(kMiThreads), 0, (hipStream_t)stream, sums, n_tiles, offsets + mi_table(k), stats);
  hipLaunchKernelGGL(mi_scan_add, dim3(n_tiles), dim3(kMiThreads), 0, (hipStream_t)stream, counts, (const uint32_t*)sums, offsets);
  return (int)hipGetLastError();
}

int launch_mi_fill(const uint8_t* refs, const int64_t* ref_off, int32_t n_refs, int32_t k, const uint32_t* offsets, uint32_t* counts,
                   int32_t* slot_oligo, uint32_t* slot_kmer, void* stream) {
  if (n_refs <= 0) return 0;
  if (k < kMpMinK || k > kMpMaxK) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(mi_fill, dim3(grid_for((size_t)n_refs, 1)), dim3(kMiOligoThreads), 0, (hipStream_t)stream, refs, ref_off, n_refs, k, offsets,
                     counts, slot_oligo, slot_kmer);
  return (int)hipGetLastError();
}

int launch_mi_rank(const int32_t* slot_oligo, const uint32_t* slot_kmer, uint32_t pairs, int32_t k, const uint32_t* offsets, int32_t* lists,
                   void* stream) {
  if (pairs == 0) return 0;
  if (k < kMpMinK || k > kMpMaxK) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(mi_rank, dim3(grid_for(pairs, kMiThreads)), dim3(kMiThreads), 0, (hipStream_t)stream, slot_oligo, slot_kmer, pairs,
                     (uint32_t)mi_table(k), offsets, lists);
  return (int)hipGetLastError();
}

}  // namespace lva
