// mi_kernels.h -- launchers of the kernels in mi_kernels.hip: the read-mapping index built on
// the device from the uploaded oligos.  The index is the one read_map.py defines (ReferenceIndex) in the layout mp_vote and
// the distance kernels read: offsets [4^k + 1], lists ascending inside a k-mer, the match masks of mp_kernels.h -- the bytes
// build_map_index (lva_stages.cpp) makes on the host.  All pointers are device pointers; oligo o is refs[ref_off[o] ..
// ref_off[o + 1]), its length in 1 .. kMaxRef.  Every launcher returns a hipError_t as int and launches nothing on a
// zero-length piece.  The steps, in the order a build runs them:
//   masks   the match masks, every word written (rows past an oligo's length stay clear);
//   count   counts [4^k], zeroed by the caller: + 1 per oligo for every distinct k-mer it holds;
//   clip    a counter above max_occ becomes 0; stats[0] += the counters that stay above 0, stats[1] += the ones dropped;
//   scan    offsets = the exclusive prefix sum of counts, offsets[4^k] = stats[2] = the sum: three launches, no workgroup
//           waits for another;
//   fill    every kept (k-mer, oligo) pair into its k-mer's segment of slot_oligo, in the order the atomics ran (counts
//           serves as the cursor and ends all zero), its k-mer beside it in slot_kmer;
//   rank    lists[offsets[c] + r] = an oligo of segment c, r the number of smaller ones in it: ascending, whatever the order
//           was, for a segment of any length.  A thread reads its whole segment, so the pass costs the sum of the squared list
//           lengths: nothing beside the rest at the default max_occ of 64, a kernel of seconds where max_occ is in the
//           tens of thousands and that many oligos share most of their k-mers.  Lists past 2 000 entries are not tested.
#pragma once
#include <cstddef>
#include <cstdint>

#include "mp_kernels.h"

namespace lva {

constexpr int kMiThreads = 256;            // masks, clip, scan, rank
constexpr int kMiOligoThreads = 64;        // count, fill: one wavefront works through an oligo
constexpr int kMiScanTile = 4096;          // counters a workgroup of the scan takes: 16 per thread
constexpr uint32_t kMiNoKmer = 0xFFFFFFFFu;
// LDS of mi_count / mi_fill: the oligo as codes and the k-mer of every position
constexpr int kMiOligoLdsBytes = 5120;
// LDS of the scan kernels: one partial sum per wavefront; mi_clip reduces two numbers at once
constexpr int kMiScanLdsBytes = 16;
constexpr int kMiClipLdsBytes = 32;
static_assert(kMiOligoLdsBytes == kMaxRef + 4 * kMaxRef && kMiScanLdsBytes == 4 * (kMiThreads / 64) && kMiClipLdsBytes == 2 * kMiScanLdsBytes,
              "the LDS constants are what the kernels declare");
static_assert(((size_t)1 << (2 * kMpMinK)) % kMiScanTile == 0 && kMiScanTile == 16 * kMiThreads, "every table is whole tiles");

inline size_t mi_table(int32_t k) { return (size_t)1 << (2 * k); }
inline size_t mi_scan_tiles(int32_t k) { return mi_table(k) / kMiScanTile; }      // the length of `sums`

int launch_mi_masks(const uint8_t* refs, const int64_t* ref_off, int32_t n_refs, int32_t ref_len, uint64_t* masks, void* stream);
int launch_mi_count(const uint8_t* refs, const int64_t* ref_off, int32_t n_refs, int32_t k, uint32_t* counts, void* stream);
int launch_mi_clip(uint32_t* counts, int32_t k, int32_t max_occ, uint32_t* stats, void* stream);
int launch_mi_scan(const uint32_t* counts, int32_t k, uint32_t* sums /* [mi_scan_tiles(k)] */, uint32_t* offsets, uint32_t* stats, void* stream);
int launch_mi_fill(const uint8_t* refs, const int64_t* ref_off, int32_t n_refs, int32_t k, const uint32_t* offsets, uint32_t* counts,
                   int32_t* slot_oligo, uint32_t* slot_kmer, void* stream);
int launch_mi_rank(const int32_t* slot_oligo, const uint32_t* slot_kmer, uint32_t pairs, int32_t k, const uint32_t* offsets, int32_t* lists,
                   void* stream);

}  // namespace lva
