// rs_kernels.h -- launcher of the kernel in rs_kernels.hip: the Reed-Solomon outer code,
// RS(65535, 65535 - fec) over GF(2^16) shortened to n_total symbols.  All pointers are device pointers.
// The launcher returns a hipError_t as int.
#pragma once
#include <cstdint>

namespace lva {

constexpr int kRsN = 65535;            // code length: fec < n_total <= kRsN
constexpr int kRsMaxFec = 4096;        // parity symbols the decoder's LDS holds

// One workgroup per codeword: sym [n_codewords][n_total] received symbols, er [n_er] erased positions in [0, n_total) shared
// by all codewords, gexp / glog the GF(2^16) tables (tr_gf_tables).  out [n_codewords][n_out] the first n_out decoded symbols,
// fail_sym in every one where the decoder gives up; ok [n_codewords] 1 = decoded, 0 = given up (always written).
int launch_rs_decode(const uint16_t* sym, int32_t n_codewords, int32_t n_total, int32_t fec, const int32_t* er, int32_t n_er,
                     uint16_t pad_sym, uint16_t fail_sym, const uint16_t* gexp, const uint16_t* glog, uint16_t* out, int32_t n_out,
                     int32_t* ok, void* stream);

}  // namespace lva
