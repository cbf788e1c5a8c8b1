// rs_kernels.hip -- SURVEY.md section 8(f) row N4: the Reed-Solomon outer code on the device.
//
// The reference decodes the outer code one 16-bit column of the oligo payloads at a time: for every column
// RSCode_schifra/RSCode_16bit_fileio.py (MainDecoder :289-299 -> RS_decode_16bit :87-137) recompiles
// schifra_RS_16bit_fileio.cpp and runs it on a full-length RS(65535, 65535 - redundancy) block over GF(2^16)
// whose first 65535 - n_total symbols are padding (ASCII "00").  Columns are independent codewords that share
// one erasure list (a missing oligo erases its symbol in every column), so here ONE launch decodes all columns:
// one workgroup per codeword, the polynomials of schifra's decoder (schifra_reed_solomon_decoder.hpp:64-424;
// citations ":NNN" below are lines of that file) in LDS, the loops over syndromes / coefficients / field
// elements spread over the 256 threads:
//   syndromes        S_i = R(alpha^i), i < fec (:227-240); the padding's contribution is a closed-form geometric sum
//   erasure locator  Gamma = prod (1 + alpha^loc x) (:211-225, :242-248)
//   modified Berlekamp-Massey from round = #erasures (:296-337), discrepancy by a workgroup reduction (:275-294)
//   Chien search     over alpha^1 .. alpha^65535 (:250-273), 256 field elements per thread, roots kept in order
//   Forney           omega = Lambda S mod x^fec, Lambda', error values (:339-385)
// with schifra's own success / failure decisions (:66-75, :105-146, :362-383), so that a column the reference gives
// up on comes back as the reference's fill bytes and a miscorrection is the same miscorrection.
// Field: primitive polynomial x^16+x^12+x^3+x+1 (schifra_galois_field.hpp:511), generator roots alpha^0..alpha^(fec-1)
// (schifra_RS_16bit_fileio.cpp:60-75 with generator_polynomial_index 0).  Integer work throughout: bit-exact.
#include <hip/hip_runtime.h>

#include "rs_kernels.h"
#include "rs_decode.h"

namespace {

using namespace lva::rs;

// grid = codewords, block = 256 threads, dynamic LDS (rs_lds_bytes).
// sym [cw][n_total] received symbols; er [S] erased positions in [0, n_total); out [cw][n_out]; ok [cw].
__global__ __launch_bounds__(kThreads) void rs_decode_kernel(const uint16_t* __restrict__ sym, int n_total, int fec,
                                                              const int* __restrict__ er, int S, uint32_t pad_sym, uint32_t fail_sym,
                                                              const uint16_t* __restrict__ gexp, const uint16_t* __restrict__ glog,
                                                              uint16_t* __restrict__ out, int n_out, int* __restrict__ ok_out) {
  extern __shared__ uint32_t lds[];
  const int cw = blockIdx.x;
  const bool ok = rs_decode_codeword(sym + (size_t)cw * n_total, n_total, fec, er, S, pad_sym, fail_sym, gexp, glog,
                                     out + (size_t)cw * n_out, n_out, lds);
  if (threadIdx.x == 0) ok_out[cw] = ok ? 1 : 0;
}

}  // namespace

namespace lva {

int launch_rs_decode(const uint16_t* sym, int32_t n_codewords, int32_t n_total, int32_t fec, const int32_t* er, int32_t n_er,
                     uint16_t pad_sym, uint16_t fail_sym, const uint16_t* gexp, const uint16_t* glog, uint16_t* out, int32_t n_out,
                     int32_t* ok, void* stream) {
  static_assert(kRsN == rs::kN && kRsMaxFec == rs::kMaxFec, "the limits the entry points check are the decoder's");
  const size_t lds = rs::rs_lds_bytes(fec);
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(rs_decode_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(rs_decode_kernel, dim3((uint32_t)n_codewords), dim3(rs::kThreads), lds, (hipStream_t)stream, sym, n_total, fec,
                     er, n_er, (uint32_t)pad_sym, (uint32_t)fail_sym, gexp, glog, out, n_out, ok);
  return (int)hipGetLastError();
}

}  // namespace lva
