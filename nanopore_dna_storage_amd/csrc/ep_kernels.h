// ep_kernels.h -- launchers of the kernels in ep_kernels.hip: the error profile of a set of reads (DESIGN.md section 1,
// row N5): every read is aligned to its oligo by unit-cost global edit distance, walked back by a fixed rule, and its
// matches, substitutions, deletions and insertions are tallied by oligo position.  The definition is
// nanopore_dna_storage_amd/error_profile.py (reference_profile).  All pointers are device pointers.  A call works on a
// chunk of reads; the per-read arrays below start at the chunk's first read.  Every launcher returns a hipError_t as int
// and launches nothing for n_reads <= 0.
#pragma once
#include <cstddef>
#include <cstdint>

#include "seq_bits.h"

namespace lva {

constexpr int kEpStripe = 64;          // reference rows a wavefront fills at a time

// Bytes of move codes that ep_fill writes for a read of n bases against ref_len positions: per stripe of 64 rows one
// 64-byte line per anti-diagonal, n + 63 of them.  0 for an empty window (the walk is all deletions and reads no code).
inline size_t ep_move_bytes(int32_t ref_len, int32_t n) {
  return n <= 0 ? 0 : (size_t)((ref_len + kEpStripe - 1) / kEpStripe) * (size_t)(n + kEpStripe - 1) * kEpStripe;
}

// One wavefront per read.  bases: the windows packed one after the other, read i at bases[win_off[i] .. + n_bases[i]);
// refs [n_refs][ref_len]; ref_id [n_reads] (< 0: the read is skipped); rc [n_reads] (non-zero: the window is
// reverse-complemented first).  Bytes are A C G T or 0 1 2 3, anything else is N.  Writes the move taken from every cell
// (i, j), 1 <= i <= ref_len, 1 <= j <= n_bases[i], to moves[move_off[i] + ...], ep_move_bytes(ref_len, n_bases[i]) bytes.
int launch_ep_fill(const uint8_t* bases, const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const uint8_t* refs,
                   int32_t ref_len, const int32_t* ref_id, const uint8_t* rc, const int64_t* move_off, uint8_t* moves, void* stream);
// One thread per read: the walk from (ref_len, n) back to (0, 0) over the moves of launch_ep_fill.
//   out_read [n_reads][4] int32 = (distance, substitutions, deletions, insertions), all -1 for a skipped read;
//   pos [ref_len + 1][4], conf [4][6], ins [5] int64: added to with integer atomics (the caller zeroes them once).
int launch_ep_walk(const uint8_t* bases, const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const uint8_t* refs,
                   int32_t ref_len, const int32_t* ref_id, const uint8_t* rc, const int64_t* move_off, const uint8_t* moves,
                   int32_t* out_read, int64_t* pos, int64_t* conf, int64_t* ins, void* stream);

}  // namespace lva
