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

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lva_decoder.h"
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

thread_local std::string g_rs_error;

int rs_run(int device, const uint16_t* symbols, int n_cw, int n_total, int fec, const int32_t* erasures, int S,
           uint16_t pad_sym, uint16_t fail_sym, uint16_t* out, int n_out, int32_t* ok) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return LVA_ERR_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return LVA_ERR_NO_DEVICE;
  std::vector<uint16_t> ex, lg;
  make_tables(&ex, &lg);
  const size_t sym_b = (size_t)n_cw * n_total * 2, out_b = (size_t)n_cw * n_out * 2, ex_b = ex.size() * 2, lg_b = lg.size() * 2;
  const size_t er_b = (size_t)std::max(S, 1) * 4, ok_b = (size_t)n_cw * 4;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  char* base = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&base), up(sym_b) + up(out_b) + up(ex_b) + up(lg_b) + up(er_b) + up(ok_b)) != hipSuccess)
    return LVA_ERR_NOMEM;
  char* p = base;
  uint16_t* d_sym = reinterpret_cast<uint16_t*>(p); p += up(sym_b);
  uint16_t* d_out = reinterpret_cast<uint16_t*>(p); p += up(out_b);
  uint16_t* d_ex = reinterpret_cast<uint16_t*>(p); p += up(ex_b);
  uint16_t* d_lg = reinterpret_cast<uint16_t*>(p); p += up(lg_b);
  int* d_er = reinterpret_cast<int*>(p); p += up(er_b);
  int* d_ok = reinterpret_cast<int*>(p);
  hipError_t e = hipMemcpy(d_sym, symbols, sym_b, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_ex, ex.data(), ex_b, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_lg, lg.data(), lg_b, hipMemcpyHostToDevice);
  if (e == hipSuccess && S > 0) e = hipMemcpy(d_er, erasures, (size_t)S * 4, hipMemcpyHostToDevice);
  const size_t lds = rs_lds_bytes(fec);
  if (e == hipSuccess && lds > 48 * 1024)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(rs_decode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(rs_decode_kernel, dim3(n_cw), dim3(kThreads), lds, nullptr, d_sym, n_total, fec, d_er, S, (uint32_t)pad_sym,
                       (uint32_t)fail_sym, d_ex, d_lg, d_out, n_out, d_ok);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, out_b, hipMemcpyDeviceToHost);
  if (e == hipSuccess && ok) e = hipMemcpy(ok, d_ok, ok_b, hipMemcpyDeviceToHost);
  (void)hipFree(base);
  if (e != hipSuccess) { g_rs_error = hipGetErrorString(e); return LVA_ERR_HIP; }
  return LVA_OK;
}

int check_common(int n_cw, int n_total, int fec) {
  if (n_cw < 0 || fec < 1 || fec > kMaxFec || n_total <= fec || n_total > kN) return LVA_ERR_ARG;
  return LVA_OK;
}

}  // namespace

extern "C" {

const char* lva_rs_last_error(void) { return g_rs_error.c_str(); }

int lva_rs_decode(int32_t device, const uint16_t* symbols, int32_t n_codewords, int32_t n_total, int32_t redundancy,
                  const int32_t* erasures, int32_t n_erasures, uint16_t pad_symbol, uint16_t fail_symbol, uint16_t* out,
                  int32_t* ok) {
  const int st = check_common(n_codewords, n_total, redundancy);
  if (st != LVA_OK) return st;
  if (n_erasures < 0 || (n_codewords > 0 && (!symbols || !out)) || (n_erasures > 0 && !erasures)) return LVA_ERR_ARG;
  std::vector<uint8_t> seen((size_t)n_total, 0);             // "erasure positions must be unique and inside the block" (:213-218)
  for (int i = 0; i < n_erasures; ++i) {
    if (erasures[i] < 0 || erasures[i] >= n_total || seen[(size_t)erasures[i]]) return LVA_ERR_ARG;
    seen[(size_t)erasures[i]] = 1;
  }
  if (n_codewords == 0) return LVA_OK;
  return rs_run(device, symbols, n_codewords, n_total, redundancy, erasures, n_erasures, pad_symbol, fail_symbol, out,
                n_total - redundancy, ok);
}

int lva_rs_encode(int32_t device, const uint16_t* data, int32_t n_codewords, int32_t n_data, int32_t redundancy,
                  uint16_t pad_symbol, uint16_t* out) {
  if (n_data < 1) return LVA_ERR_ARG;
  const int n_total = n_data + redundancy;
  const int st = check_common(n_codewords, n_total, redundancy);
  if (st != LVA_OK) return st;
  if (n_codewords > 0 && (!data || !out)) return LVA_ERR_ARG;
  if (n_codewords == 0) return LVA_OK;
  // systematic encoding = filling in the parity symbols as erasures: the unique codeword with these data symbols
  std::vector<uint16_t> rx((size_t)n_codewords * n_total, 0);
  for (int c = 0; c < n_codewords; ++c) std::memcpy(&rx[(size_t)c * n_total], data + (size_t)c * n_data, (size_t)n_data * 2);
  std::vector<int32_t> er((size_t)redundancy), ok((size_t)n_codewords, 0);
  for (int i = 0; i < redundancy; ++i) er[(size_t)i] = n_data + i;
  const int rc = rs_run(device, rx.data(), n_codewords, n_total, redundancy, er.data(), redundancy, pad_symbol, 0, out, n_total, ok.data());
  if (rc != LVA_OK) return rc;
  for (int c = 0; c < n_codewords; ++c)
    if (!ok[(size_t)c]) { g_rs_error = "encode: the erasure decode of the parity symbols failed"; return LVA_ERR_HIP; }
  return LVA_OK;
}

}  // extern "C"
