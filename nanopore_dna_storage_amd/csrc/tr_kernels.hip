// tr_kernels.hip -- DESIGN.md section 1 row N4': reading-cost trials on the device.
//
// The reference measures how many reads the outer code needs by repeating, NUM_TRIALS times per sample size
// (decode_RS_from_decoded_lists.py:30-66): draw NUM_READS_TO_USE read numbers, filter their lists, take the per-index
// vote (:37-51), RS-decode, compare with the original file.  The filter's result and the reads of every index do not
// depend on the trial (ls_filter; ls_bucket_count, ls_bucket_scan and tr_bucket_list: once per call); what does is done
// here for a chunk of trials and all sample sizes at once:
//   tr_consensus      which reads of an index a trial's sample holds, and the vote among them -> the RS input
//   tr_erasures       the absent indices of every (sample size, trial)
//   rs_trials_kernel  the decode of rs_decode_kernel (rs_decode.h) per codeword, each with its trial's erasure list,
//                     and the comparison with the original
//   tr_fold           columns -> (passed, present, columns_ok, success)
// The sample of trial t is defined by a keyed permutation of the read numbers (trials.py: 8 Feistel rounds over Philox,
// stream 5, with cycle walking), so "is read q in the sample of size u" is place(q) < u, and place(q) takes one lane a
// loop without memory traffic.  Integer work throughout, no atomics: every result is exact and the same from run to run.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "ls_bucket.h"
#include "philox.h"
#include "rs_decode.h"
#include "tr_kernels.h"

namespace lva {

namespace {

constexpr uint32_t kPadSym = 0x3030;                   // two ASCII '0': dummy reads, padding and a failed column (rs_code.PAD)
constexpr int kRounds = 8;

// sigma_t^-1(q), trials.py: walk the inverse Feistel pass until the value is a read number again
__device__ __forceinline__ uint32_t trial_place(uint32_t q, uint32_t n, int h, uint32_t t, uint32_t k0, uint32_t k1) {
  const uint32_t mask = (1u << h) - 1u;
  uint32_t x = q;
  do {
    uint32_t l = x >> h, r = x & mask;
    for (int i = kRounds - 1; i >= 0; --i) {
      const uint32_t f = philox(l, (uint32_t)i, t, kStreamTrial, k0, k1).x & mask;
      const uint32_t nl = r ^ f;
      r = l;
      l = nl;
    }
    x = (l << h) | r;
  } while (x >= n);
  return x;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w);
  return v;
}

// grid = indices, block = one wavefront: order[bucket[x] .. bucket[x + 1]) = the reads of index x in read order
__global__ __launch_bounds__(64) void tr_bucket_list(const int32_t* __restrict__ index, int n_reads,
                                                     const int32_t* __restrict__ bucket, int32_t* __restrict__ order) {
  const int x = blockIdx.x, s = bucket[x];
  list_bucket(index, n_reads, x, bucket[x + 1] - s, order + s, (int)threadIdx.x);
}

// grid = num_oligos * chunk (index x fastest), block = one wavefront.
//
// The vote (ls_consensus's comment proves the rule for read order): the winner has the largest final count, and among
// those it reached that count first, "first" now by place in the trial's order.  With c_j = the number of reads i of the
// index with place_i <= place_j that carry the payload of read j, the winner inside the sample of size u is the payload
// of the member j (place_j < u) with the largest c_j, and among those the smallest place.  c_j does not depend on u --
// place_i <= place_j < u puts read i into the sample too -- so it is counted once, for the members of the largest sample,
// and every sample size is then one reduction to (max c, then min place) over lanes; places are distinct, so the
// reduction has one winner.  Work is quadratic in the reads of ONE index, linear in everything else.
__global__ __launch_bounds__(64) void tr_consensus(TrShape sh, int h, const int32_t* __restrict__ bucket,
                                                   const int32_t* __restrict__ order, const uint8_t* __restrict__ payload,
                                                   int32_t* __restrict__ place, int32_t* __restrict__ cnt, int32_t* __restrict__ nmem,
                                                   uint16_t* __restrict__ sym, uint8_t* __restrict__ cons) {
  const int lane = threadIdx.x;
  const int x = (int)(blockIdx.x % (uint32_t)sh.num_oligos), j = (int)(blockIdx.x / (uint32_t)sh.num_oligos);
  const int s0 = bucket[x], m = bucket[x + 1] - s0;
  const int bpo = sh.bpo, s = bpo >> 1, no = sh.num_oligos;
  const int32_t* mem = order + s0;
  int32_t* pl = place + (size_t)j * sh.n_reads + s0;
  int32_t* cn = cnt + (size_t)j * sh.n_reads + s0;
  const uint32_t t = sh.first_trial + (uint32_t)j;
  const int umax = sh.points[sh.n_points - 1];
  for (int a = lane; a < m; a += 64) pl[a] = (int32_t)trial_place((uint32_t)mem[a], (uint32_t)sh.n_reads, h, t, sh.k0, sh.k1);
  __syncthreads();                                       // the places are read back by other lanes
  for (int a = lane; a < m; a += 64) {
    const int pa = pl[a];
    int c = 0;
    if (pa < umax) {
      const uint8_t* ya = payload + (size_t)mem[a] * bpo;
      for (int i = 0; i < m; ++i)
        if (pl[i] <= pa && same_payload(payload + (size_t)mem[i] * bpo, ya, bpo)) ++c;
    }
    cn[a] = c;                                           // (read back by this lane only)
  }
  for (int k = 0; k < sh.n_points; ++k) {
    const int u = sh.points[k];
    int best_c = 0, best_p = INT_MAX, best_r = 0, mine = 0;
    for (int a = lane; a < m; a += 64) {
      const int pa = pl[a];
      if (pa < u) {
        const int c = cn[a];
        ++mine;
        if (c > best_c || (c == best_c && pa < best_p)) { best_c = c; best_p = pa; best_r = mem[a]; }
      }
    }
    const int members = wave_sum(mine);
    int top = best_c;
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) top = max(top, __shfl_xor(top, w));
    best_p = (mine > 0 && best_c == top) ? best_p : INT_MAX;
    int first = best_p;
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) first = min(first, __shfl_xor(first, w));
    const unsigned long long won = __ballot(mine > 0 && best_p == first);
    const size_t kt = (size_t)k * sh.chunk + j;
    if (lane == 0) nmem[kt * no + x] = members;
    if (members > 0) {                                   // uniform; `won` has exactly one bit
      const int rd = __shfl(best_r, __ffsll(won) - 1);
      const uint8_t* win = payload + (size_t)rd * bpo;
      for (int c = lane; c < s; c += 64) sym[(kt * s + c) * no + x] = (uint16_t)(win[2 * c] | ((uint32_t)win[2 * c + 1] << 8));
      if (cons) for (int b = lane; b < bpo; b += 64) cons[(kt * no + x) * bpo + b] = win[b];
    } else {
      for (int c = lane; c < s; c += 64) sym[(kt * s + c) * no + x] = (uint16_t)kPadSym;
      if (cons) for (int b = lane; b < bpo; b += 64) cons[(kt * no + x) * bpo + b] = 0;
    }
  }
}

// grid = n_points * chunk, block = one wavefront: ballot compaction of the absent indices, 64 at a time
__global__ __launch_bounds__(64) void tr_erasures(int no, const int32_t* __restrict__ nmem, int32_t* __restrict__ erl,
                                                  int32_t* __restrict__ ern, int32_t* __restrict__ pp, uint8_t* __restrict__ pres) {
  const int lane = threadIdx.x;
  const size_t kt = blockIdx.x;
  const int32_t* row = nmem + kt * no;
  int32_t* er = erl + kt * no;
  int S = 0, passed = 0;
  for (int x0 = 0; x0 < no; x0 += 64) {
    const int x = x0 + lane;
    const int c = x < no ? row[x] : 0;
    const bool absent = x < no && c == 0;
    const unsigned long long mask = __ballot(absent);
    if (absent) er[S + __popcll(mask & ((1ull << lane) - 1ull))] = x;      // S + hits below < no: they are distinct indices
    S += __popcll(mask);
    passed += c;
    if (pres && x < no) pres[kt * no + x] = c > 0 ? 1 : 0;
  }
  passed = wave_sum(passed);
  if (lane == 0) { ern[kt] = S; pp[2 * kt] = passed; pp[2 * kt + 1] = no - S; }
}

// grid = codewords of the chunk = n_points * chunk * s, block = 256 threads, dynamic LDS rs_lds_bytes(fec)
__global__ __launch_bounds__(rs::kThreads) void rs_trials_kernel(const uint16_t* __restrict__ sym, int n_total, int fec, int s,
                                                                 const int32_t* __restrict__ erl, const int32_t* __restrict__ ern,
                                                                 const uint16_t* __restrict__ gexp, const uint16_t* __restrict__ glog,
                                                                 uint16_t* __restrict__ dec, const uint16_t* __restrict__ truth,
                                                                 long long original_bytes, int bpo, int32_t* __restrict__ okeq) {
  extern __shared__ uint32_t lds[];
  const size_t cw = blockIdx.x, kt = cw / (uint32_t)s;
  const int c = (int)(cw % (uint32_t)s), n_out = n_total - fec;
  uint16_t* o = dec + cw * n_out;
  const bool ok = rs::rs_decode_codeword(sym + cw * n_total, n_total, fec, erl + kt * n_total, ern[kt], kPadSym, kPadSym, gexp, glog,
                                         o, n_out, lds);
  // symbol j of column c holds bytes j * bpo + 2 c and + 1 of the file (low byte first)
  uint32_t diff = 0;                                     // (o: stores of other threads, behind the barrier the decode ends with)
  for (int j = (int)threadIdx.x; j < n_out; j += rs::kThreads) {
    const long long at = (long long)j * bpo + 2 * c;
    const uint32_t mask = at + 1 < original_bytes ? 0xFFFFu : at < original_bytes ? 0x00FFu : 0u;
    diff |= ((uint32_t)o[j] ^ truth[(size_t)c * n_out + j]) & mask;
  }
  diff = rs::block_max(diff, rs::rs_red(lds, fec));
  if (threadIdx.x == 0) { okeq[2 * cw] = ok ? 1 : 0; okeq[2 * cw + 1] = diff == 0 ? 1 : 0; }
}

// one thread per kt.  No index present: the reference dies in MainDecoder; counted as a failure with no column decoded.
__global__ __launch_bounds__(64) void tr_fold(int K, int chunk, int s, const int32_t* __restrict__ okeq,
                                              const int32_t* __restrict__ pp, int32_t* __restrict__ stats, int n_trials,
                                              int trial_at) {
  const int kt = blockIdx.x * 64 + threadIdx.x;
  if (kt >= K * chunk) return;
  const int k = kt / chunk, j = kt % chunk;
  int cols = 0, eq = 1;
  for (int c = 0; c < s; ++c) { cols += okeq[2 * ((size_t)kt * s + c)]; eq &= okeq[2 * ((size_t)kt * s + c) + 1]; }
  const int passed = pp[2 * kt], present = pp[2 * kt + 1];
  *reinterpret_cast<int4*>(stats + ((size_t)k * n_trials + trial_at + j) * 4) =
      make_int4(passed, present, present > 0 ? cols : 0, present > 0 && eq ? 1 : 0);
}

int half_bits(int32_t n) {                               // trials.half_bits
  int bits = 0;
  while (bits < 31 && ((int64_t)1 << bits) < (int64_t)n) ++bits;
  return bits < 2 ? 1 : (bits + 1) / 2;
}

}  // namespace

void tr_gf_tables(std::vector<uint16_t>* ex, std::vector<uint16_t>* lg) {
  static_assert(kTrGexpWords == rs::kGexpWords && kTrGlogWords == rs::kGlogWords, "table sizes");
  rs::make_tables(ex, lg);
}

int launch_tr_bucket_list(const int32_t* index, int32_t n_reads, int32_t num_oligos, const int32_t* bucket, int32_t* order,
                          void* stream) {
  hipLaunchKernelGGL(tr_bucket_list, dim3((uint32_t)num_oligos), dim3(64), 0, (hipStream_t)stream, index, n_reads, bucket, order);
  return (int)hipGetLastError();
}

int launch_tr_consensus(const TrShape& sh, const int32_t* bucket, const int32_t* order, const uint8_t* payload, int32_t* place,
                        int32_t* cnt, int32_t* nmem, uint16_t* sym, uint8_t* cons, void* stream) {
  hipLaunchKernelGGL(tr_consensus, dim3((uint32_t)sh.num_oligos * (uint32_t)sh.chunk), dim3(64), 0, (hipStream_t)stream, sh,
                     half_bits(sh.n_reads), bucket, order, payload, place, cnt, nmem, sym, cons);
  return (int)hipGetLastError();
}

int launch_tr_erasures(const TrShape& sh, const int32_t* nmem, int32_t* erl, int32_t* ern, int32_t* pp, uint8_t* pres, void* stream) {
  hipLaunchKernelGGL(tr_erasures, dim3((uint32_t)sh.n_points * (uint32_t)sh.chunk), dim3(64), 0, (hipStream_t)stream, sh.num_oligos,
                     nmem, erl, ern, pp, pres);
  return (int)hipGetLastError();
}

int launch_tr_decode(const TrShape& sh, const uint16_t* sym, const int32_t* erl, const int32_t* ern, const uint16_t* gexp,
                     const uint16_t* glog, uint16_t* dec, const uint16_t* truth, int64_t original_bytes, int32_t* okeq, void* stream) {
  const size_t lds = rs::rs_lds_bytes(sh.fec);
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(rs_trials_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const int s = sh.bpo / 2;
  hipLaunchKernelGGL(rs_trials_kernel, dim3((uint32_t)sh.n_points * (uint32_t)sh.chunk * (uint32_t)s), dim3(rs::kThreads), lds,
                     (hipStream_t)stream, sym, sh.num_oligos, sh.fec, s, erl, ern, gexp, glog, dec, truth, (long long)original_bytes,
                     sh.bpo, okeq);
  return (int)hipGetLastError();
}

int launch_tr_fold(const TrShape& sh, const int32_t* okeq, const int32_t* pp, int32_t* stats, int32_t n_trials, int32_t trial_at,
                   void* stream) {
  const int kt = sh.n_points * sh.chunk;
  hipLaunchKernelGGL(tr_fold, dim3((uint32_t)((kt + 63) / 64)), dim3(64), 0, (hipStream_t)stream, sh.n_points, sh.chunk, sh.bpo / 2,
                     okeq, pp, stats, n_trials, trial_at);
  return (int)hipGetLastError();
}

}  // namespace lva
