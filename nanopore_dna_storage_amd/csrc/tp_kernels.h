// tp_kernels.h -- launchers of the kernels in tp_kernels.hip: flappie's transition posteriors of a flip-flop CRF
// (DESIGN.md section 1, row N0).  scores / post: float32 [blocks][40], 16-byte aligned; row_off: n_reads + 1 block
// offsets on the device; fwd: 8 floats per block of scratch.  A batch needs at least one block.
#pragma once
#include <cstdint>

namespace lva {

// 8 lanes per read, lane = target state: forward vector before every block -> fwd
int launch_tp_forward(const float* scores, const int64_t* row_off, int32_t n_reads, float* fwd, void* stream);
// 8 lanes per read, lane = source state: backward vector, posteriors, normalisation.  post may be scores.
int launch_tp_backward(const float* scores, const int64_t* row_off, int32_t n_reads, const float* fwd, float* post,
                       void* stream);

}  // namespace lva
