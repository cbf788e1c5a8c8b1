// ls_kernels.hip -- SURVEY.md section 8(f) row N2: what happens to a decoded list, on the device.
//
// The reference handles a decoded list in Python, on '0'/'1' strings:
//   helper.decode_list_CRC_index (helper.py:371-388)      first entry whose CRC-8 and index check      -> ls_filter
//   decode_RS_from_decoded_lists.py:37-51                  per-index vote over the payloads that passed -> ls_consensus
//   helper.simulate_and_decode (helper.py:326-329)         "the first payload seen stands"              -> ls_consensus, first_only
//   simulator.py:92-110                                    per-trial statistics against the truth       -> ls_stats + ls_edit
// The kernels read the decoder's own output array, uint8 [n_reads][list_size][msg_len] of 0/1 (only bit 0 of a byte
// is looked at) with counts [n_reads]; nothing is converted on the host.  Integer work throughout, no atomics:
// every result is exact and the same from run to run.
//
// A message (helper.py:253-262) is  PRP(index) : 12 bits | payload : 8 * bytes_per_oligo bits | CRC-8 : 8 bits [| pad bit].
// The reference left-pads it with zero bits to whole bytes -- 12 + 8 (b + 1) bits: always four of them -- and takes the
// CRC over all bytes but the last.  Leading zero bits leave a CRC register that starts at 0 untouched, so the CRC is
// taken here over the first 12 + 8 b message bits directly, a bit at a time, and the payload bytes are the bits from 12 on.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "ls_bucket.h"
#include "ls_kernels.h"
#include "seq_bits.h"

namespace lva {

namespace {

constexpr uint32_t kPrpAInv = 3303, kPrpB = 2532;      // helper.py:28-32: index = a_inv * (x - b) mod 2^12
constexpr int kIndexLen = 12;

// CRC-8, polynomial x^8+x^2+x+1 (0x07), register starts at 0, no reflection, no final xor: one message bit per step.
__device__ __forceinline__ uint32_t crc8_bit(uint32_t c, uint32_t bit) {
  c ^= bit << 7;
  return ((c << 1) ^ ((c & 0x80u) ? 0x07u : 0u)) & 0xFFu;
}

__device__ __forceinline__ uint32_t pack_byte(const uint8_t* b) {       // 8 bits, first one on top
  uint32_t v = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) v = (v << 1) | (b[i] & 1u);
  return v;
}

// grid = reads, block = one wavefront.  Up to 64 entries of the read are copied to LDS as the dwords they lie in (an
// entry starts anywhere: msg_len is arbitrary), then lane e checks entry e.  A list longer than 64 takes more passes,
// and the loop ends at the first pass with a hit, so a later entry never replaces an earlier one.
__global__ __launch_bounds__(64) void ls_filter(const uint8_t* __restrict__ msgs, const int32_t* __restrict__ counts,
                                                int list_size, int msg_len, int use, int bpo, int num_oligos,
                                                int32_t* __restrict__ out_index, int32_t* __restrict__ out_rank,
                                                uint8_t* __restrict__ out_payload) {
  extern __shared__ uint32_t ls_lds[];
  const int lane = threadIdx.x;
  const size_t read = blockIdx.x;
  const int lim = min(counts[read], use);               // <= 0: no list
  const int crc_bits = kIndexLen + 8 * bpo;
  uint8_t* pay = out_payload + read * (size_t)bpo;
  for (int e0 = 0; e0 < lim; e0 += 64) {
    const int ne = min(64, lim - e0);
    const size_t a = (read * (size_t)list_size + (size_t)e0) * (size_t)msg_len;      // first byte of the pass
    const int sh = (int)(a & 3);
    const int ndw = (sh + ne * msg_len + 3) >> 2;
    const uint32_t* g = reinterpret_cast<const uint32_t*>(msgs + (a - sh));
    __syncthreads();                                     // the pass before has been read
    for (int i = lane; i < ndw; i += 64) ls_lds[i] = g[i];
    __syncthreads();
    bool ok = false;
    uint32_t idx = 0;
    const uint8_t* b = reinterpret_cast<const uint8_t*>(ls_lds) + sh + lane * msg_len;
    if (lane < ne) {
      uint32_t c = 0, x = 0;
      for (int i = 0; i < kIndexLen; ++i) { const uint32_t bit = b[i] & 1u; x = (x << 1) | bit; c = crc8_bit(c, bit); }
      for (int i = kIndexLen; i < crc_bits; ++i) c = crc8_bit(c, b[i] & 1u);
      idx = (kPrpAInv * (x - kPrpB)) & 0xFFFu;           // (two's complement: the low 12 bits are those of the Python expression)
      ok = c == pack_byte(b + crc_bits) && idx < (uint32_t)num_oligos;
    }
    const unsigned long long hits = __ballot(ok);
    if (hits) {                                          // uniform
      if (lane == __ffsll(hits) - 1) {
        out_index[read] = (int32_t)idx;
        out_rank[read] = e0 + lane;
        for (int k = 0; k < bpo; ++k) pay[k] = (uint8_t)pack_byte(b + kIndexLen + 8 * k);
      }
      return;
    }
  }
  if (lane == 0) { out_index[read] = -1; out_rank[read] = -1; }
  for (int k = lane; k < bpo; k += 64) pay[k] = 0;
}

// ---- consensus ----

// grid = indices, block = one wavefront: cnt[x] = reads whose index is x.
__global__ __launch_bounds__(64) void ls_bucket_count(const int32_t* __restrict__ index, int n_reads, int32_t* __restrict__ cnt) {
  const int lane = threadIdx.x, x = blockIdx.x;
  int c = 0;
  for (int i0 = 0; i0 < n_reads; i0 += 64) {
    const int i = i0 + lane;
    c += __popcll(__ballot(i < n_reads && index[i] == x));
  }
  if (lane == 0) cnt[x] = c;
}

// one block of 256: bucket [n] counts -> bucket [n + 1] exclusive prefix sums, n <= 4096 (16 per thread)
__global__ __launch_bounds__(256) void ls_bucket_scan(int32_t* __restrict__ bucket, int n) {
  __shared__ int part[256];
  const int tid = threadIdx.x, per = (n + 255) / 256;
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += bucket[i];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; }
    bucket[n] = run;
  }
  __syncthreads();
  int run = part[tid];
  for (int i = lo; i < hi; ++i) { const int v = bucket[i]; bucket[i] = run; run += v; }
}

// grid = indices, block = one wavefront.  The wavefront first lists the reads of its index in read order
// (order[bucket[x] ..): a ballot over 64 reads at a time, each hit placed behind the hits of lower lanes), then votes.
//
// The vote.  The reference keeps, per index, a list of [payload, count] and after every read re-sorts it with a stable
// sort by -count (decode_RS_from_decoded_lists.py:37-51); the winner is the head of the list at the end.  By induction
// the list is always ordered by count, and among equal counts by the time that count was reached: a payload going
// from c to c + 1 stood behind every payload with count >= c + 1 before the sort, so the stable sort puts it last
// among those with c + 1, and it is the latest to have reached c + 1; a new payload is appended last among the 1s.
// So the winner has the largest final count M, and among those it reached M first.  With c_j = number of reads
// i <= j of the index that carry the payload of read j (the count that vote j produced), that is the payload of the
// smallest j with c_j = M = max c_j: lanes take j, count, and the wavefront reduces to (max c, then min j).
// Work is quadratic in the reads of ONE index (its coverage), linear in everything else.
// first_only (helper.py:326-329): the first payload seen stands; votes = the reads that agree with it.
__global__ __launch_bounds__(64) void ls_consensus(const int32_t* __restrict__ index, const uint8_t* __restrict__ payload,
                                                   int n_reads, int bpo, int first_only, const int32_t* __restrict__ bucket,
                                                   int32_t* __restrict__ order, uint8_t* __restrict__ present,
                                                   uint8_t* __restrict__ out_payload, int32_t* __restrict__ votes) {
  const int lane = threadIdx.x, x = blockIdx.x;
  const int s = bucket[x], t = bucket[x + 1] - s;
  uint8_t* o = out_payload + (size_t)x * bpo;
  if (t <= 0) {
    if (lane == 0) { present[x] = 0; votes[x] = 0; }
    for (int k = lane; k < bpo; k += 64) o[k] = 0;
    return;
  }
  int32_t* mem = order + s;
  list_bucket(index, n_reads, x, t, mem, lane);
  __syncthreads();                                       // the list is read back by other lanes
  int best_c = 0, best_j = INT_MAX;
  if (first_only) {
    const uint8_t* p0 = payload + (size_t)mem[0] * bpo;
    for (int j = lane; j < t; j += 64) best_c += same_payload(payload + (size_t)mem[j] * bpo, p0, bpo) ? 1 : 0;
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) best_c += __shfl_xor(best_c, w);
    best_j = 0;
  } else {
    for (int j = lane; j < t; j += 64) {                 // j grows: a later j replaces the lane's best only with a larger count
      const uint8_t* pj = payload + (size_t)mem[j] * bpo;
      int c = 0;
      for (int i = 0; i <= j; ++i) c += same_payload(payload + (size_t)mem[i] * bpo, pj, bpo) ? 1 : 0;
      if (c > best_c) { best_c = c; best_j = j; }
    }
    int top = best_c;
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) top = max(top, __shfl_xor(top, w));
    best_j = best_c == top ? best_j : INT_MAX;
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) best_j = min(best_j, __shfl_xor(best_j, w));
    best_c = top;
  }
  const uint8_t* win = payload + (size_t)mem[best_j] * bpo;
  for (int k = lane; k < bpo; k += 64) o[k] = win[k];
  if (lane == 0) { present[x] = 1; votes[x] = best_c; }
}

// ---- statistics ----

__device__ __forceinline__ int blocks_set(unsigned long long d, int width) {     // non-zero width-bit blocks of d (8 or 16)
  d |= d >> 4; d |= d >> 2; d |= d >> 1;                                         // bit 0 of every byte = OR of the byte
  if (width == 16) { d |= d >> 8; return __popcll(d & 0x0001000100010001ull); }
  return __popcll(d & 0x0101010101010101ull);
}

// grid = reads, block = one wavefront, lane l holds bits l, 64 + l, 128 + l, 192 + l: a ballot is one 64-bit word of
// the message, and 8- and 16-bit blocks never straddle words (a short last block ends in zero bits).
// simulator.py:92-110 without the edit distance; truth and top entry go to `packed` as bit words for ls_edit.
__global__ __launch_bounds__(64) void ls_stats(const uint8_t* __restrict__ msgs, const int32_t* __restrict__ counts,
                                               const uint8_t* __restrict__ truth, int list_size, int msg_len,
                                               unsigned long long* __restrict__ packed, int32_t* __restrict__ out) {
  const int lane = threadIdx.x;
  const size_t read = blockIdx.x;
  const int c = min(counts[read], list_size);
  int32_t* o = out + read * kLsStatFields;
  if (c <= 0) {
    if (lane < kLsStatFields) o[lane] = -1;
    return;
  }
  const uint8_t* tr = truth + read * (size_t)msg_len;
  const uint8_t* row = msgs + read * (size_t)list_size * (size_t)msg_len;
  uint32_t tb[4];
  unsigned long long tw[4], dw[4];
  int ham = 0, h8 = 0, h16 = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int p = 64 * w + lane;
    tb[w] = p < msg_len ? (tr[p] & 1u) : 0u;
    const uint32_t ob = p < msg_len ? (row[p] & 1u) : 0u;
    tw[w] = __ballot(tb[w]);
    dw[w] = __ballot(tb[w] != ob);
    ham += __popcll(dw[w]);
    h8 += blocks_set(dw[w], 8);
    h16 += blocks_set(dw[w], 16);
  }
  int in_list = ham == 0;
  for (int e = 1; e < c && !in_list; ++e) {              // uniform
    row += msg_len;
    bool diff = false;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int p = 64 * w + lane;
      if (p < msg_len) diff |= (row[p] & 1u) != tb[w];
    }
    in_list = __ballot(diff) == 0ull;
  }
  if (lane == 0) {
    o[0] = ham == 0; o[1] = in_list; o[2] = ham; o[3] = h8; o[4] = h16;
    unsigned long long* pk = packed + read * kLsPackWords;
#pragma unroll
    for (int w = 0; w < 4; ++w) { pk[w] = tw[w]; pk[4 + w] = tw[w] ^ dw[w]; }
  }
}

// Unit-cost Levenshtein distance of two m-bit strings, m <= 64 W: seq_bits.h's bit-vector step over the W words of a
// column, for the whole-string distance (the horizontal delta entering row 0 is +1, each word's leaving delta enters
// the next).  a = pattern, b = text, bit i of word k = position 64 k + i; rows past m take part but never reach the
// rows below them (deltas and shifts only move up).
template <int W>
__device__ __forceinline__ int myers(const unsigned long long* a, const unsigned long long* b, int m) {
  uint64_t pv[W], mv[W], tx[W];
#pragma unroll
  for (int k = 0; k < W; ++k) { pv[k] = ~0ull; mv[k] = 0; tx[k] = b[k]; }
  const int hw = (m - 1) >> 6, hb = (m - 1) & 63;
  int score = m;
  for (int j = 0; j < m; ++j) {
    const uint64_t flip = (tx[0] & 1ull) ? 0ull : ~0ull;                 // Eq = positions of the pattern equal to text bit j
    int h = 1;
#pragma unroll
    for (int k = 0; k < W; ++k) {
      if (k + 1 < W) tx[k] = (tx[k] >> 1) | (tx[k + 1] << 63); else tx[k] >>= 1;
      const uint64_t eq = a[k] ^ flip;
      uint64_t ph, mh;
      h = bv_step_word(pv[k], mv[k], eq, h, ph, mh);
      if (k == hw) score += bv_row_delta(ph, mh, hb);
    }
  }
  return score;
}

// one thread per read: the edit distance between truth and top entry (simulator.py:108, distance.levenshtein)
__global__ __launch_bounds__(64) void ls_edit(const int32_t* __restrict__ counts, const unsigned long long* __restrict__ packed,
                                              int n_reads, int msg_len, int32_t* __restrict__ out) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= n_reads || counts[r] <= 0) return;            // (ls_stats wrote -1)
  unsigned long long a[4], b[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) { a[w] = packed[(size_t)r * kLsPackWords + w]; b[w] = packed[(size_t)r * kLsPackWords + 4 + w]; }
  int d;
  if (msg_len <= 64) d = myers<1>(a, b, msg_len);
  else if (msg_len <= 128) d = myers<2>(a, b, msg_len);
  else if (msg_len <= 192) d = myers<3>(a, b, msg_len);
  else d = myers<4>(a, b, msg_len);
  out[(size_t)r * kLsStatFields + 5] = d;
}

}  // namespace

uint32_t ls_filter_lds_bytes(int32_t use_entries, uint32_t msg_len) {
  const uint32_t ne = use_entries < 64 ? (uint32_t)use_entries : 64u;
  return (ne * msg_len + 3u + 3u + 15u) & ~15u;          // up to 3 bytes in front of the first entry, whole dwords
}

int launch_ls_filter(const uint8_t* msgs, const int32_t* counts, int32_t n_reads, int32_t list_size, uint32_t msg_len,
                     int32_t use_entries, int32_t bytes_per_oligo, int32_t num_oligos, int32_t pad, int32_t* out_index,
                     int32_t* out_rank, uint8_t* out_payload, void* stream) {
  if (n_reads <= 0) return 0;
  (void)pad;                                             // the pad bit is the last one and is never read
  hipLaunchKernelGGL(ls_filter, dim3(n_reads), dim3(64), ls_filter_lds_bytes(use_entries, msg_len), (hipStream_t)stream, msgs,
                     counts, list_size, (int)msg_len, use_entries, bytes_per_oligo, num_oligos, out_index, out_rank, out_payload);
  return (int)hipGetLastError();
}

int launch_ls_consensus(const int32_t* index, const uint8_t* payload, int32_t n_reads, int32_t bytes_per_oligo,
                        int32_t num_oligos, int32_t first_only, int32_t* bucket, int32_t* order, uint8_t* present,
                        uint8_t* out_payload, int32_t* votes, void* stream) {
  if (n_reads <= 0) return 0;
  if (const int e = launch_ls_bucket_scan(index, n_reads, num_oligos, bucket, stream)) return e;
  hipLaunchKernelGGL(ls_consensus, dim3(num_oligos), dim3(64), 0, (hipStream_t)stream, index, payload, n_reads, bytes_per_oligo,
                     first_only, bucket, order, present, out_payload, votes);
  return (int)hipGetLastError();
}

int launch_ls_bucket_scan(const int32_t* index, int32_t n_reads, int32_t num_oligos, int32_t* bucket, void* stream) {
  if (n_reads <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ls_bucket_count, dim3(num_oligos), dim3(64), 0, st, index, n_reads, bucket);
  hipLaunchKernelGGL(ls_bucket_scan, dim3(1), dim3(256), 0, st, bucket, num_oligos);
  return (int)hipGetLastError();
}

int launch_ls_stats(const uint8_t* msgs, const int32_t* counts, const uint8_t* truth, int32_t n_reads, int32_t list_size,
                    uint32_t msg_len, uint64_t* packed, int32_t* out, void* stream) {
  if (n_reads <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* pk = reinterpret_cast<unsigned long long*>(packed);
  hipLaunchKernelGGL(ls_stats, dim3(n_reads), dim3(64), 0, st, msgs, counts, truth, list_size, (int)msg_len, pk, out);
  hipLaunchKernelGGL(ls_edit, dim3((n_reads + 63) / 64), dim3(64), 0, st, counts, pk, n_reads, (int)msg_len, out);
  return (int)hipGetLastError();
}

}  // namespace lva
