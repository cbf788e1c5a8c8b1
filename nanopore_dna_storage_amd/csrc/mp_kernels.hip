// mp_kernels.hip -- DESIGN.md section 1 row N6: reads mapped to oligos on the device.
//
// The reference maps every basecall against merged.fa with minimap2 (util/align_compute_stats.sh:21-33) and splits,
// counts and profiles the reads from that mapping.  Here the definition is the project's own (read_map.reference_map),
// exact integers throughout, and the device is held to it bit for bit:
//   mp_vote     one workgroup per read: the window is staged once in LDS as codes, one rolling pass forms the k-mer of
//               every position and the k-mer its reverse complement shows there, the oligos that hold them get a vote
//               in uint16 LDS counters, and the counters are folded into the read's first `cands` candidates;
//   mp_verify   a lane per candidate: the bit-vector edit distance of the oligo against the oriented window, the
//               window's ends free, W = ceil(ref_len / 64) words per column; then the winner and the runner-up of each
//               read.  Launched a second time per chunk in its anchored form (one lane per read): the winner's reversed
//               oligo against the window read backwards from the alignment's end, which gives its start.
//
// How mp_verify lays work onto lanes.  A wavefront takes 64 / L reads, L = 2, 4 or 8 lanes per read (the next power of
// two that holds `cands`); the anchored pass takes 64 reads, one lane each.  The lanes of a wavefront hold windows of
// different lengths and strands, so no lane reads its window from memory: for every block of 64 columns the wavefront
// stages the next 64 bases of each of its streams (a read and a direction) into an LDS tile -- one 64-byte line per
// load, lane l takes byte l -- as codes, complemented where the stream is a reverse strand.  A lane then takes its
// column's code from its stream's row, a dword per four columns; the lanes of one read share the address (a broadcast)
// and rows are padded to 17 dwords so that different reads fall on different banks.  A lane past its window's end idles.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mp_kernels.h"

namespace lva {

namespace {

constexpr int kTileRow = 17;          // dwords of a tile row: 64 codes and one of padding

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int o) {
  const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
  return ((uint64_t)hi << 32) | lo;
}

// a thread's partial list: the kMpMaxCands smallest keys it has seen, ascending
struct TopList {
  uint64_t l[kMpMaxCands];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < kMpMaxCands; ++i) l[i] = kMpNoCand;
  }
  __device__ __forceinline__ void insert(uint64_t key) {
    if (key >= l[kMpMaxCands - 1]) return;
    l[kMpMaxCands - 1] = key;
#pragma unroll
    for (int i = kMpMaxCands - 1; i > 0; --i) {
      const uint64_t a = l[i - 1], b = l[i];
      l[i - 1] = a < b ? a : b;
      l[i] = a < b ? b : a;
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int i = 0; i + 1 < kMpMaxCands; ++i) l[i] = l[i + 1];
    l[kMpMaxCands - 1] = kMpNoCand;
  }
};

// one vote for every oligo of [base, base + kMpVoteRange) that holds the k-mer: the lists are ascending
__device__ __forceinline__ void vote(uint32_t* __restrict__ cnt, const uint32_t* __restrict__ offsets, const int32_t* __restrict__ lists,
                                     uint32_t kmer, int base) {
  const uint32_t lo = offsets[kmer], hi = offsets[kmer + 1];
  for (uint32_t p = lo; p < hi; ++p) {
    const int o = lists[p] - base;
    if (o >= kMpVoteRange) break;
    if (o >= 0) atomicAdd(&cnt[o >> 1], 1u << (16 * (o & 1)));      // a vote is at most 4096: no carry into the neighbour
  }
}

// grid = reads of the chunk, block = kMpVoteThreads
__global__ __launch_bounds__(kMpVoteThreads) void mp_vote(const uint8_t* __restrict__ bases, const int32_t* __restrict__ win_off,
                                                          const int32_t* __restrict__ n_bases, const uint32_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ lists, int k, int n_refs, int min_votes,
                                                          int cands, uint64_t* __restrict__ cand) {
  __shared__ uint64_t top[kMpMaxCands];                        // the first candidates of the ranges so far, in order
  __shared__ uint64_t red[kMpVoteThreads / 64];
  __shared__ uint32_t cnt[2][kMpVoteRange / 2];                // uint16 [2][kMpVoteRange], two counters to a word
  __shared__ uint8_t rd[kMaxRead];                             // the window as given, 0..4
  static_assert(sizeof(top) + sizeof(red) + sizeof(cnt) + sizeof(rd) == kMpVoteLdsBytes, "kMpVoteLdsBytes");
  const int tid = threadIdx.x;
  const size_t r = blockIdx.x;
  const int n = n_bases[r];
  const uint8_t* w = bases + win_off[r];
  for (int j = tid; j < n; j += kMpVoteThreads) rd[j] = (uint8_t)base_code(w[j]);
  if (tid < kMpMaxCands) top[tid] = kMpNoCand;
  __syncthreads();
  const int npos = n - k + 1;
  if (npos > 0) {                                              // uniform
    const int seg = (npos + kMpVoteThreads - 1) / kMpVoteThreads;
    const int a = tid * seg, b = min(a + seg, npos);           // this thread's positions, one rolling run
    const uint32_t mask = (1u << (2 * k)) - 1u;
    const int hi_shift = 2 * (k - 1);
    uint32_t* flat = &cnt[0][0];
    for (int base = 0; base < n_refs; base += kMpVoteRange) {
      for (int i = tid; i < kMpVoteRange; i += kMpVoteThreads) flat[i] = 0;
      __syncthreads();
      if (a < b) {
        // fwd: the k-mer of the window at the position; rev: the k-mer of the reverse-complemented window that covers
        // the same bases, built from the other end (the last base's complement is its first)
        uint32_t fwd = 0, rev = 0;
        int run = 0;                                           // bases since the last N
        for (int j = a; j < b + k - 1; ++j) {
          const uint32_t c = rd[j];
          if (c < kBaseN) {
            fwd = ((fwd << 2) | c) & mask;
            rev = (rev >> 2) | (complement_code(c) << hi_shift);
            ++run;
          } else {
            run = 0;
          }
          if (j >= a + k - 1 && run >= k) {
            vote(cnt[0], offsets, lists, fwd, base);
            vote(cnt[1], offsets, lists, rev, base);
          }
        }
      }
      __syncthreads();
      // fold the range into the running list: partial lists per thread, then one round per place
      TopList mine;
      mine.clear();
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < kMpMaxCands; ++i) mine.insert(top[i]);
      }
      for (int i = tid; i < kMpVoteRange; i += kMpVoteThreads) {
        const uint32_t word = flat[i];
        if (word == 0) continue;
        const uint32_t strand = (uint32_t)i / (kMpVoteRange / 2);
        const uint32_t o = (uint32_t)base + 2u * ((uint32_t)i % (kMpVoteRange / 2));
        const uint32_t v0 = word & 0xFFFFu, v1 = word >> 16;
        if ((int)v0 >= min_votes) mine.insert(mp_cand_key(v0, strand, o));
        if ((int)v1 >= min_votes) mine.insert(mp_cand_key(v1, strand, o + 1));
      }
      for (int place = 0; place < kMpMaxCands; ++place) {
        uint64_t m = mine.l[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const uint64_t other = shfl_xor64(m, o);
          m = other < m ? other : m;
        }
        if ((tid & 63) == 0) red[tid >> 6] = m;
        __syncthreads();
        uint64_t g = red[0];
#pragma unroll
        for (int q = 1; q < kMpVoteThreads / 64; ++q) g = red[q] < g ? red[q] : g;
        if (tid == 0) top[place] = g;                          // (a key names one strand and oligo: one thread holds it)
        if (g != kMpNoCand && mine.l[0] == g) mine.pop();
        __syncthreads();                                       // red is read before the next round writes it
      }
    }
  }
  if (tid < kMpMaxCands) cand[r * kMpMaxCands + tid] = tid < cands ? top[tid] : kMpNoCand;
}

// WT = 2, 4: the vertical vectors of WT words in registers (ref_len <= 64 WT; words past the oligo's last carry no
// match and change nothing below them).  WT = 0: any ref_len <= kMaxRef, the vectors in LDS.
// grid = ceil(reads / (64 / L)), block = one wavefront.  anchored = 0: L lanes per read, lane c of a read takes its
// candidate c.  anchored = 1: L = 1, the winner that the first pass left in `out`.
template <int WT>
__global__ __launch_bounds__(64) void mp_verify(const uint8_t* __restrict__ bases, const int32_t* __restrict__ win_off,
                                                const int32_t* __restrict__ n_bases, int n_reads, const uint64_t* __restrict__ cand,
                                                const uint64_t* __restrict__ masks, int ref_len, int L, int cands, int max_dist,
                                                int anchored, int32_t* __restrict__ out) {
  __shared__ uint32_t tile[64][kTileRow];                      // per stream the codes of 64 columns
  __shared__ int32_t s_off[64], s_len[64], s_how[64];          // per stream: first base, bases, bit 0: backwards, bit 1: complemented
  __shared__ int32_t s_use[64];                                // per stream: a lane of the wavefront has a job on it
  const int lane = threadIdx.x;
  const int W = (ref_len + 63) >> 6;
  const int rpw = 64 / L;                                      // reads of this wavefront
  const int S = anchored ? 1 : 2;                              // streams per read: both strands, or the winner's
  {                                                            // lane sl describes stream sl
    const int q = lane / S, r = blockIdx.x * rpw + q;
    int off = 0, len = 0, how = 0;
    if (lane < rpw * S && r < n_reads) {
      const int n = n_bases[r], w0 = win_off[r];
      if (!anchored) {                                         // strand 0: the window; strand 1: from its end, complemented
        const int strand = lane & 1;
        len = n; off = strand ? w0 + n - 1 : w0; how = strand ? 3 : 0;
      } else if (out[(size_t)r * 8 + 1] >= 0) {                // the oriented window's first e bases, backwards
        const int strand = out[(size_t)r * 8 + 2], e = out[(size_t)r * 8 + 4];
        len = e; off = strand ? w0 + n - e : w0 + e - 1; how = strand ? 2 : 1;
      }
    }
    s_off[lane] = off; s_len[lane] = len; s_how[lane] = how; s_use[lane] = 0;
  }
  // this lane's job
  const int q = lane / L, c = lane % L, r = blockIdx.x * rpw + q;
  bool job = false;
  int oligo = 0, strand = 0, votes = 0, slot = 0;
  if (r < n_reads) {
    if (!anchored) {
      const uint64_t key = c < cands ? cand[(size_t)r * kMpMaxCands + c] : kMpNoCand;
      if (key != kMpNoCand) { job = true; oligo = mp_key_oligo(key); strand = mp_key_strand(key); votes = mp_key_votes(key); }
      slot = 2 * q + strand;
    } else {
      const int best = out[(size_t)r * 8 + 1];
      if (best >= 0) { job = true; oligo = best; strand = out[(size_t)r * 8 + 2]; }
      slot = q;
    }
  }
  __syncthreads();
  if (job) s_use[slot] = 1;                                    // (the lanes of a stream all write the same)
  __syncthreads();
  const int mylen = job ? s_len[slot] : 0;
  int steps = mylen;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) steps = max(steps, __shfl_xor(steps, o));
  const int nslots = rpw * S;

  const uint64_t* mrow = masks + (size_t)(oligo * 2 + (anchored ? 1 : 0)) * 4 * (size_t)W;
  const int wl = (ref_len - 1) >> 6, bit = (ref_len - 1) & 63;          // the word and bit of row m
  const int hin0 = anchored ? 1 : 0;                           // D[0][j] = 0: the read's ends are free; anchored: D[0][j] = j
  int score = ref_len, best = ref_len, arg = 0;                // column 0: D[m][0] = m
  uint64_t peq[4][WT > 0 ? WT : 1], pv[WT > 0 ? WT : 1], mv[WT > 0 ? WT : 1];
  if constexpr (WT > 0) {
#pragma unroll
    for (int w = 0; w < WT; ++w) {
      pv[w] = ~0ull; mv[w] = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) peq[b][w] = (job && w < W) ? mrow[b * W + w] : 0ull;
    }
  }
  __shared__ uint64_t s_pv[WT == 0 ? kMpMaxWords : 1][64], s_mv[WT == 0 ? kMpMaxWords : 1][64];
  if constexpr (WT == 0) {
    for (int w = 0; w < W; ++w) { s_pv[w][lane] = ~0ull; s_mv[w][lane] = 0; }
  }

  for (int t0 = 0; t0 < steps; t0 += 64) {
    for (int sl = 0; sl < nslots; ++sl) {                      // stage: one 64-byte line per stream
      const int len = s_use[sl] ? s_len[sl] : 0;               // a strand that no candidate is on is not staged
      if (t0 >= len) continue;                                 // uniform
      const int t = t0 + lane, how = s_how[sl];
      uint32_t code = kBaseN;
      if (t < len) {
        code = base_code(bases[s_off[sl] + ((how & 1) ? -t : t)]);
        if ((how & 2) && code < kBaseN) code = complement_code(code);      // (asked for bases only: one select per byte)
      }
      reinterpret_cast<uint8_t*>(tile[sl])[lane] = (uint8_t)code;
    }
    __syncthreads();
    for (int qd = 0; qd < 16; ++qd) {
      const uint32_t word = tile[slot][qd];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = t0 + 4 * qd + u;
        if (t < mylen) {
          const uint32_t ch = (word >> (8 * u)) & 0xFFu;
          int h = hin0;
          if constexpr (WT > 0) {
#pragma unroll
            for (int w = 0; w < WT; ++w) {
              const uint64_t eq = ch == 0 ? peq[0][w] : ch == 1 ? peq[1][w] : ch == 2 ? peq[2][w] : ch == 3 ? peq[3][w] : 0ull;
              uint64_t ph, mh;
              h = bv_step_word(pv[w], mv[w], eq, h, ph, mh);
              if (w == wl) score += bv_row_delta(ph, mh, bit);
            }
          } else {
            for (int w = 0; w < W; ++w) {
              uint64_t p = s_pv[w][lane], m = s_mv[w][lane], ph, mh;
              const uint64_t eq = ch < kBaseN ? mrow[ch * W + w] : 0ull;
              h = bv_step_word(p, m, eq, h, ph, mh);
              s_pv[w][lane] = p; s_mv[w][lane] = m;
              if (w == wl) score += bv_row_delta(ph, mh, bit);
            }
          }
          if (score < best) { best = score; arg = t + 1; }     // the smallest column that attains the minimum
        }
      }
    }
    __syncthreads();                                           // the tile is read before the next block overwrites it
  }

  if (anchored) {                                              // E[m][j] >= d and attains it: arg = j'
    if (job) {
      const int n = n_bases[r], e = out[(size_t)r * 8 + 4];
      out[(size_t)r * 8 + 4] = strand ? n - e : e - arg;
      out[(size_t)r * 8 + 5] = arg;
    }
    return;
  }
  // the winner: the smallest (distance, place in the candidate order); the runner-up: the best other oligo
  constexpr int kNone = 0x7FFFFFFF;
  int key = job ? (best << 4) | c : kNone;
  for (int o = 1; o < L; o <<= 1) key = min(key, __shfl_xor(key, o));
  const int src = key == kNone ? lane : (lane & ~(L - 1)) | (key & 15);
  const int w_oligo = __shfl(oligo, src), w_strand = __shfl(strand, src), w_votes = __shfl(votes, src), w_end = __shfl(arg, src);
  int second = (job && oligo != w_oligo) ? best : kNone;
  for (int o = 1; o < L; o <<= 1) second = min(second, __shfl_xor(second, o));
  if (c == 0 && r < n_reads) {
    int32_t* o = out + (size_t)r * 8;
    if (key == kNone) {
      o[0] = -1; o[1] = -1; o[2] = 0; o[3] = -1; o[4] = 0; o[5] = 0; o[6] = 0; o[7] = -1;
    } else {
      const int d = key >> 4;
      o[0] = d <= max_dist ? w_oligo : -1; o[1] = w_oligo; o[2] = w_strand; o[3] = d; o[4] = w_end; o[5] = 0; o[6] = w_votes;
      o[7] = second == kNone ? -1 : second;
    }
  }
}

int lanes_per_read(int cands) { return cands <= 2 ? 2 : cands <= 4 ? 4 : 8; }

int launch_verify(const uint8_t* bases, const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const uint64_t* cand,
                  const uint64_t* masks, int32_t ref_len, int L, int32_t cands, int32_t max_dist, int anchored, int32_t* out,
                  void* stream) {
  if (n_reads <= 0) return 0;
  const int rpw = 64 / L;
  const dim3 grid((n_reads + rpw - 1) / rpw), block(64);
  const hipStream_t s = (hipStream_t)stream;
  if (ref_len <= 128)
    hipLaunchKernelGGL(mp_verify<2>, grid, block, 0, s, bases, win_off, n_bases, n_reads, cand, masks, ref_len, L, cands, max_dist, anchored, out);
  else if (ref_len <= 256)
    hipLaunchKernelGGL(mp_verify<4>, grid, block, 0, s, bases, win_off, n_bases, n_reads, cand, masks, ref_len, L, cands, max_dist, anchored, out);
  else
    hipLaunchKernelGGL(mp_verify<0>, grid, block, 0, s, bases, win_off, n_bases, n_reads, cand, masks, ref_len, L, cands, max_dist, anchored, out);
  return (int)hipGetLastError();
}

}  // namespace

int launch_mp_vote(const uint8_t* bases, const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const uint32_t* offsets,
                   const int32_t* lists, int32_t k, int32_t n_refs, int32_t min_votes, int32_t cands, uint64_t* cand, void* stream) {
  if (n_reads <= 0) return 0;
  hipLaunchKernelGGL(mp_vote, dim3(n_reads), dim3(kMpVoteThreads), 0, (hipStream_t)stream, bases, win_off, n_bases, offsets, lists, k,
                     n_refs, min_votes, cands, cand);
  return (int)hipGetLastError();
}

int launch_mp_verify(const uint8_t* bases, const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const uint64_t* cand,
                     const uint64_t* masks, int32_t ref_len, int32_t cands, int32_t max_dist, int32_t* out, void* stream) {
  return launch_verify(bases, win_off, n_bases, n_reads, cand, masks, ref_len, lanes_per_read(cands), cands, max_dist, 0, out, stream);
}

int launch_mp_start(const uint8_t* bases, const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const uint64_t* masks,
                    int32_t ref_len, int32_t* out, void* stream) {
  return launch_verify(bases, win_off, n_bases, n_reads, nullptr, masks, ref_len, 1, 0, 0, 1, out, stream);
}

}  // namespace lva
