// mq_kernels.h -- launchers of the kernels in mq_kernels.hip: a pooled run mapped in one call (DESIGN.md section 1, row
// N6; the definition is nanopore_dna_storage_amd/read_map.py).  The oligos of one index differ in length, so the free-end
// distance of mp_kernels.hip is taken with every lane's oligo at its own length (mq_verify), and a supplementary pass
// maps the longer unaligned flank of every mapped read as a read of its own (mq_flank, then launch_mp_vote of
// mp_kernels.h as it is, then mq_verify again).  Keys, candidate lists and limits are those of mp_kernels.h.  All
// pointers are device pointers; a call works on a chunk of reads and the per-read arrays start at the chunk's first
// read.  Every launcher returns a hipError_t as int and launches nothing for n_reads <= 0.
#pragma once
#include <cstddef>
#include <cstdint>

#include "mp_kernels.h"

namespace lva {

// Match masks at ONE stride: masks[((oligo * 2 + reversed) * 4 + base) * words + w] with words = ceil(max_len / 64) for
// every oligo, max_len the longest; the reversed oligo is reversed within its own length lens[oligo]; rows past
// lens[oligo] are clear (mp_mask_words(n_refs, max_len) words in all).
//
// The distance of every candidate at its oligo's own length, the winner and the runner-up: out [n_reads][8] as
// launch_mp_verify writes it, ref = best if dist <= max_dist[best].  lens, max_dist: [n_refs].
int launch_mq_verify(const uint8_t* bases, const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const uint64_t* cand,
                     const uint64_t* masks, const int32_t* lens, int32_t max_len, int32_t cands, const int32_t* max_dist,
                     int32_t* out, void* stream);
// The anchored reverse pass with the winner's own length: `end` becomes (start, count) in the coordinates of the window
// as given, plus shift[read] where shift is not null (a flank's place in the window it was cut from).
int launch_mq_start(const uint8_t* bases, const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const uint64_t* masks,
                    const int32_t* lens, int32_t max_len, const int32_t* shift, int32_t* out, void* stream);
// One thread per read, from the finished primary rows: the longer of the flanks [0, start) and [start + count, n) of a
// mapped read (ref >= 0), the left one on a tie, if it has at least min_flank bases -- flank_off (into the packed bases),
// flank_len, flank_shift (its first base in the window); flank_len = 0 where there is no supplementary pass.
int launch_mq_flank(const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const int32_t* out, int32_t min_flank,
                    int32_t* flank_off, int32_t* flank_len, int32_t* flank_shift, void* stream);

}  // namespace lva
