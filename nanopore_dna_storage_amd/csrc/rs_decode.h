// rs_decode.h -- the decode of ONE Reed-Solomon codeword by one workgroup of 256 threads, as a __device__ function, and what
// its callers share with it: the field, the LDS size, the tables.  rs_kernels.hip (rs_decode_kernel: all columns of one
// received file, one erasure list) and tr_kernels.hip (rs_trials_kernel: the columns of many trials, an erasure list per
// trial) both launch it.  What it computes and which lines of schifra's decoder each step follows is in the head of
// rs_kernels.hip; citations ":NNN" are lines of schifra_reed_solomon_decoder.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

namespace lva {
namespace rs {

constexpr int kN = 65535;           // code length = field size - 1
constexpr int kMaxFec = 4096;       // LDS budget: 4 polynomials of 2 fec + 8 coefficients, syndromes, omega, roots
constexpr int kThreads = 256;

struct Gf {
  const uint16_t* ex;               // alpha^i for i in [0, 2N)  (doubled: no reduction after adding two logarithms)
  const uint16_t* lg;               // log_alpha(v), v in [1, 65535]
  __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) const { return (a && b) ? ex[lg[a] + lg[b]] : 0u; }
  __device__ __forceinline__ uint32_t div(uint32_t a, uint32_t b) const { return (a && b) ? ex[lg[a] + kN - lg[b]] : 0u; }
  __device__ __forceinline__ uint32_t pw(uint32_t e) const { return ex[e % kN]; }       // alpha^e
};

// XOR of one value per thread over the workgroup; every thread gets the result.  `red` = 8 words of LDS.
__device__ __forceinline__ uint32_t block_xor(uint32_t v, uint32_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] ^ red[1] ^ red[2] ^ red[3];
}

__device__ __forceinline__ uint32_t block_max(uint32_t v, uint32_t* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const uint32_t w = __shfl_xor(v, o); v = w > v ? w : v; }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t m = red[0];
  for (int i = 1; i < 4; ++i) m = red[i] > m ? red[i] : m;
  return m;
}

// the 8 reduction words inside rs_decode_codeword's LDS: free again once it has returned
__device__ __forceinline__ uint32_t* rs_red(uint32_t* lds, int fec) {
  const int cap = 2 * fec + 8;
  return reinterpret_cast<uint32_t*>(reinterpret_cast<uint16_t*>(lds) + 4 * cap + 2 * fec) + cap;
}

// One codeword, the whole workgroup (kThreads threads, every one of them calls it; the result is uniform).
// r [n_total] received symbols; er [S] erased positions in [0, n_total); o [n_out] the decoded symbols, or fail_sym in
// every one when the decoder gives up (false is returned then); lds: rs_lds_bytes(fec) bytes.  On return the workgroup
// has passed a barrier since the last store to o and the last use of the LDS.
__device__ __forceinline__ bool rs_decode_codeword(const uint16_t* __restrict__ r, int n_total, int fec, const int* __restrict__ er,
                                                   int S, uint32_t pad_sym, uint32_t fail_sym, const uint16_t* __restrict__ gexp,
                                                   const uint16_t* __restrict__ glog, uint16_t* __restrict__ o, int n_out,
                                                   uint32_t* lds) {
  const int tid = threadIdx.x;
  const int cap = 2 * fec + 8;
  uint16_t* lam = reinterpret_cast<uint16_t*>(lds);          // Lambda
  uint16_t* tmp = lam + cap;                                 // tau / scratch
  uint16_t* prv = tmp + cap;                                 // previous_lambda without its x^shift factor
  uint16_t* llg = prv + cap;                                 // log of the coefficients of the polynomial being evaluated
  uint16_t* syn = llg + cap;                                 // [fec]
  uint16_t* omg = syn + fec;                                 // [fec]
  uint32_t* roots = reinterpret_cast<uint32_t*>(omg + fec);   // [cap]  (4 cap + 2 fec halfwords before it: aligned)
  uint32_t* red = roots + cap;                               // [8] reductions, [8..] flags / scan
  uint32_t* scan = red + 16;                                 // [kThreads + 1]
  const Gf gf{gexp, glog};
  const int pad = kN - n_total;
  auto finish = [&](bool ok) {                               // uniform over the workgroup
    if (!ok) for (int j = tid; j < n_out; j += kThreads) o[j] = (uint16_t)fail_sym;
    __syncthreads();                                         // o is complete for every thread of the workgroup
    return ok;
  };

  // ---- syndromes (:227-240) ----
  uint32_t any = 0;
  for (int i = tid; i < fec; i += kThreads) {
    uint32_t acc = 0;
    uint32_t t = (uint32_t)(((uint64_t)i * (uint64_t)(n_total - 1)) % kN);   // i * exponent of symbol 0
    for (int j = 0; j < n_total; ++j) {
      const uint32_t v = r[j];
      if (v) acc ^= gexp[glog[v] + t];
      t = t >= (uint32_t)i ? t - i : t + kN - i;
    }
    if (pad > 0 && pad_sym) {            // sum over the padding of pad_sym * x^e, e = n_total .. N-1, x = alpha^i
      if (i == 0) { if (pad & 1) acc ^= pad_sym; }
      else {
        const uint32_t num = gf.pw((uint32_t)(((uint64_t)i * pad) % kN)) ^ 1u;
        const uint32_t den = gf.pw(i) ^ 1u;
        acc ^= gf.mul(gf.mul(pad_sym, gf.pw((uint32_t)(((uint64_t)i * n_total) % kN))), gf.div(num, den));
      }
    }
    syn[i] = (uint16_t)acc;
    any |= acc;
  }
  for (int j = tid; j < n_out; j += kThreads) o[j] = r[j];   // the word as received; corrections are XORed in below
  any = block_max(any, red);
  if (S > fec) return finish(false);                         // more erasures than parity symbols: refused before anything else (:66-75)
  if (any == 0) return finish(true);                         // already a codeword (:82-90)

  // ---- erasure locator (:211-225, :242-248): Lambda = prod (1 + alpha^loc x), loc = N-1-(pad+p) = n_total-1-p ----
  if (tid == 0) lam[0] = 1;
  int len = 1;
  __syncthreads();
  for (int e = 0; e < S; ++e) {
    const uint32_t alog = (uint32_t)(n_total - 1 - er[e]);
    for (int k = tid; k <= len; k += kThreads) {
      const uint32_t a = k < len ? lam[k] : 0u, b = k >= 1 ? lam[k - 1] : 0u;
      tmp[k] = (uint16_t)(a ^ (b ? gexp[glog[b] + alog] : 0u));
    }
    __syncthreads();
    { uint16_t* sw = lam; lam = tmp; tmp = sw; }
    len += 1;                                                // the leading coefficient is a product of non-zero elements
  }

  // ---- modified Berlekamp-Massey (:296-337) ----
  int psh = 1, plen = len;                                   // previous_lambda = prv * x^psh
  for (int k = tid; k < len; k += kThreads) prv[k] = lam[k];
  __syncthreads();
  if (S < fec) {
    int bi = -1, l = S;
    for (int rnd = S; rnd < fec; ++rnd) {
      const int ub = min(l, len - 1);                        // compute_discrepancy (:275-294)
      uint32_t part = 0;
      for (int k = tid; k <= ub; k += kThreads) part ^= gf.mul(lam[k], syn[rnd - k]);
      const uint32_t d = block_xor(part, red);
      if (d != 0) {
        const int n = max(len, plen + psh);
        uint32_t top = 0;
        for (int k = tid; k < n; k += kThreads) {            // tau = lambda - d * previous_lambda, then simplify
          const uint32_t a = k < len ? lam[k] : 0u;
          const uint32_t b = (k >= psh && k - psh < plen) ? prv[k - psh] : 0u;
          const uint32_t v = a ^ gf.mul(b, d);
          tmp[k] = (uint16_t)v;
          if (v) top = (uint32_t)k + 1;
        }
        const int nlen = (int)block_max(top, red);           // (barriers inside: tmp is complete, lam / prv fully read)
        if (l < rnd - bi) {
          const int t2 = rnd - bi;
          bi = rnd - l;
          l = t2;
          for (int k = tid; k < len; k += kThreads) prv[k] = (uint16_t)gf.div(lam[k], d);   // lambda / discrepancy (:327)
          plen = len; psh = 0;
        }
        __syncthreads();
        { uint16_t* sw = lam; lam = tmp; tmp = sw; }
        len = nlen;
      }
      psh += 1;                                              // previous_lambda <<= 1
      if (plen + psh > cap - 2) return finish(false);        // cannot happen for fec <= kMaxFec (guard only)
    }
  }
  const int deg = len - 1;

  // ---- Chien search (:250-273): roots alpha^i, i = 1..N in increasing order (at most deg of them exist) ----
  for (int k = tid; k < len; k += kThreads) llg[k] = lam[k] ? glog[lam[k]] : (uint16_t)0xFFFF;
  __syncthreads();
  uint32_t found[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t cnt = 0;
  for (int q = 0; q < 256; q += 4) {
    uint32_t iv[4], tv[4], acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { iv[u] = (uint32_t)tid * 256u + 1u + q + u; tv[u] = 0; acc[u] = 0; }
    for (int k = 0; k < len; ++k) {
      const uint32_t lgk = llg[k];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (lgk != 0xFFFFu) acc[u] ^= gexp[lgk + tv[u]];
        tv[u] += iv[u] % kN;
        tv[u] = tv[u] >= (uint32_t)kN ? tv[u] - kN : tv[u];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (iv[u] <= (uint32_t)kN && acc[u] == 0) { found[(q + u) >> 5] |= 1u << ((q + u) & 31); ++cnt; }
  }
  scan[tid + 1] = cnt;
  if (tid == 0) scan[0] = 0;
  __syncthreads();
  if (tid == 0) for (int i = 1; i <= kThreads; ++i) scan[i] += scan[i - 1];
  __syncthreads();
  const int L = (int)scan[kThreads];
  if (L > cap) return finish(false);                         // (a polynomial of degree deg has at most deg roots)
  {
    uint32_t at = scan[tid];
    for (int w = 0; w < 8; ++w) {
      uint32_t bits = found[w];
      while (bits) {
        const int b = __builtin_ctz(bits);
        bits &= bits - 1;
        roots[at++] = (uint32_t)tid * 256u + 1u + 32u * w + b;
      }
    }
  }
  __syncthreads();
  if (L == 0) return finish(false);                                               // :105-121
  if ((uint64_t)(2ull * (uint64_t)L - (uint64_t)S) > (uint64_t)fec) return finish(false);   // size_t arithmetic (:122-146)

  // ---- Forney (:339-385): omega = first fec coefficients of Lambda * S; derivative = odd coefficients of Lambda ----
  for (int k = tid; k < fec; k += kThreads) {
    uint32_t acc = 0;
    const int amax = min(k, len - 1);
    for (int a = 0; a <= amax; ++a) acc ^= gf.mul(lam[a], syn[k - a]);
    omg[k] = acc ? glog[acc] : (uint16_t)0xFFFF;                                 // kept as logarithms for the evaluation
  }
  __syncthreads();
  uint32_t bad = 0;
  for (int x = tid; x < L; x += kThreads) {
    const uint32_t i = roots[x], im = i % kN;
    uint32_t ov = 0, dv = 0, t = 0;
    for (int k = 0; k < fec; ++k) {                                               // omega(alpha^i)
      const uint32_t lgk = omg[k];
      if (lgk != 0xFFFFu) ov ^= gexp[lgk + t];
      t += im; t = t >= (uint32_t)kN ? t - kN : t;
    }
    t = 0;
    const uint32_t i2 = (2u * im) % kN;
    for (int k = 0; k + 1 < len; k += 2) {                                        // Lambda'(alpha^i): coefficient k = Lambda[k+1], k even
      const uint32_t lgk = llg[k + 1];
      if (lgk != 0xFFFFu) dv ^= gexp[lgk + t];
      t += i2; t = t >= (uint32_t)kN ? t - kN : t;
    }
    const uint32_t num = gf.mul(ov, gf.pw((uint32_t)kN - im));                    // root_exponent_table_[i] = alpha^(N-i) (:193-196)
    if (num != 0) {
      if (dv != 0) {
        const int p = (int)i - 1 - pad;                                          // rsblock[error_location - 1] (:364)
        if (p >= 0 && p < n_out) o[p] ^= (uint16_t)gf.div(num, dv);
      } else bad = 1;                                                             // e_decoder_error3
    }
  }
  bad = block_max(bad, red);
  return finish(bad == 0 && deg == L);                                            // :376-383
}

// dynamic LDS of a launch that calls rs_decode_codeword; above 48 KB the kernel has to opt in
// (hipFuncAttributeMaxDynamicSharedMemorySize)
inline size_t rs_lds_bytes(int fec) {
  const size_t cap = 2 * (size_t)fec + 8;
  return (4 * cap + 2 * (size_t)fec + 2) * sizeof(uint16_t) + (cap + 16 + kThreads + 1 + 4) * sizeof(uint32_t);
}

constexpr size_t kGexpWords = 2 * (size_t)kN + 2, kGlogWords = 65536;

// GF(2^16) tables, generated as schifra_galois_field.hpp:317-357 does
inline void make_tables(std::vector<uint16_t>* ex, std::vector<uint16_t>* lg) {
  ex->assign(kGexpWords, 0);
  lg->assign(kGlogWords, 0);
  uint32_t x = 1;
  for (int i = 0; i < kN; ++i) {
    (*ex)[i] = (uint16_t)x;
    (*lg)[x] = (uint16_t)i;
    x <<= 1;
    if (x & 0x10000u) x ^= 0x1100Bu;
  }
  for (int i = kN; i < 2 * kN + 2; ++i) (*ex)[i] = (*ex)[i - kN];
}

}  // namespace rs
}  // namespace lva
