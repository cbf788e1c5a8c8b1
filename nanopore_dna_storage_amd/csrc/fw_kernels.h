// fw_kernels.h -- launcher of the kernel in fw_kernels.hip: the forward score of ONE base sequence on a read, the log of the
// total weight of all its alignments inside the band (the definition is
// nanopore_dna_storage_amd/trellis_score.py, reference_forward).  sc_score's trellis with every maximum replaced by a
// log-sum-exp and every cell outside its block's band counted as -inf.  All pointers are device pointers.  The launcher
// returns a hipError_t as int and launches nothing for n_pairs <= 0.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sc_kernels.h"

namespace lva {

// LDS of one workgroup: sc_score's layout and nothing beside it (sc_kernels.h) -- the band of the block before is carried
// in a scalar, and nothing is written for a position that leaves the band.  5.9 KB for 187 positions, 20 KB for the longest
// sequence: eight workgroups of 1024 bases fit a CU.
constexpr size_t fw_lds_bytes(int max_len) { return sc_lds_bytes(max_len); }

// out[pair] = (flip, flop): the forward scores of the two states of the last base at the last position after the last block,
// float32.  pairs, bases, band and max_len as launch_sc_score takes them.
int launch_fw_forward(const float* post, const uint8_t* bases, const ScPair* pairs, const uint32_t* band, int32_t n_pairs,
                      int32_t max_len, float* out, void* stream);

}  // namespace lva
