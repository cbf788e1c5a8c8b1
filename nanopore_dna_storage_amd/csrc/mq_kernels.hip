// mq_kernels.hip -- DESIGN.md section 1 row N6: a pooled run mapped in one call.
//
// The reference maps one sequencing run of thirteen experiments against merged.fa, whose oligos differ in length, and
// drops chimeric alignments (util/align_compute_stats.sh:21-33).  The definition is read_map.reference_map; the device is
// held to it bit for bit (tests/test_gpu_read_map_pooled.py).
//   mq_verify   mp_verify (mp_kernels.hip) with every lane's oligo at its own length: the word and bit of the last row,
//               the score's start and the number of words are the lane's, read from lens[oligo]; the masks of all
//               oligos lie at one stride, the words of the longest, with the rows past an oligo's last clear, so the
//               register forms step through words that carry no match and change nothing.  The threshold of `ref` is
//               max_dist[winner].  Its anchored form takes the winner's reversed oligo, reversed within its own length,
//               and adds a read's shift to the start it reports;
//   mq_flank    one thread per read: the longer unaligned flank of a mapped read, as a window of its own.  mp_vote and
//               mq_verify then map the flanks like reads (the supplementary pass); nothing returns to the host between.
//
// The lane layout is mp_verify's (its header comment): 64 / L reads per wavefront, an LDS tile of 64 columns per
// stream, no lane reads its window from memory, control flow around __syncthreads is uniform.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mq_kernels.h"

namespace lva {

namespace {

constexpr int kTileRow = 17;          // dwords of a tile row: 64 codes and one of padding

// WT = 2, 4: the vertical vectors of WT words in registers (max_len <= 64 WT).  WT = 0: any max_len <= kMaxRef, the
// vectors in LDS, a lane steps through the words of its own oligo.  W: the masks' stride, ceil(max_len / 64).
// grid = ceil(reads / (64 / L)), block = one wavefront.  anchored = 0: L lanes per read, lane c of a read takes its
// candidate c.  anchored = 1: L = 1, the winner that the first pass left in `out`.
template <int WT>
__global__ __launch_bounds__(64) void mq_verify(const uint8_t* __restrict__ bases, const int32_t* __restrict__ win_off,
                                                const int32_t* __restrict__ n_bases, int n_reads, const uint64_t* __restrict__ cand,
                                                const uint64_t* __restrict__ masks, const int32_t* __restrict__ lens, int W, int L,
                                                int cands, const int32_t* __restrict__ max_dist, const int32_t* __restrict__ shift,
                                                int anchored, int32_t* __restrict__ out) {
  __shared__ uint32_t tile[64][kTileRow];                      // per stream the codes of 64 columns
  __shared__ int32_t s_off[64], s_len[64], s_how[64];          // per stream: first base, bases, bit 0: backwards, bit 1: complemented
  __shared__ int32_t s_use[64];                                // per stream: a lane of the wavefront has a job on it
  const int lane = threadIdx.x;
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
  const int m = job ? lens[oligo] : 1;                         // this lane's oligo: rows 0 .. m
  const int wl = (m - 1) >> 6, bit = (m - 1) & 63;             // the word and bit of row m
  const int hin0 = anchored ? 1 : 0;                           // D[0][j] = 0: the read's ends are free; anchored: D[0][j] = j
  int score = m, best = m, arg = 0;                            // column 0: D[m][0] = m
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
            for (int w = 0; w <= wl; ++w) {                    // the words of this lane's oligo
              uint64_t p = s_pv[w][lane], mm = s_mv[w][lane], ph, mh;
              const uint64_t eq = ch < kBaseN ? mrow[ch * W + w] : 0ull;
              h = bv_step_word(p, mm, eq, h, ph, mh);
              s_pv[w][lane] = p; s_mv[w][lane] = mm;
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
      out[(size_t)r * 8 + 4] = (strand ? n - e : e - arg) + (shift ? shift[r] : 0);
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
      o[0] = d <= max_dist[w_oligo] ? w_oligo : -1; o[1] = w_oligo; o[2] = w_strand; o[3] = d; o[4] = w_end; o[5] = 0; o[6] = w_votes;
      o[7] = second == kNone ? -1 : second;
    }
  }
}

// grid = ceil(reads / 256), block = 256
__global__ __launch_bounds__(256) void mq_flank(const int32_t* __restrict__ win_off, const int32_t* __restrict__ n_bases, int n_reads,
                                                const int32_t* __restrict__ out, int min_flank, int32_t* __restrict__ flank_off,
                                                int32_t* __restrict__ flank_len, int32_t* __restrict__ flank_shift) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_reads) return;
  int first = 0, len = 0;
  if (out[(size_t)r * 8] >= 0) {
    const int start = out[(size_t)r * 8 + 4], end = start + out[(size_t)r * 8 + 5];
    const int right = n_bases[r] - end;
    if (start >= right) { len = start; } else { first = end; len = right; }      // the longer one, the left one on a tie
    if (len < min_flank) { first = 0; len = 0; }
  }
  flank_off[r] = win_off[r] + first; flank_len[r] = len; flank_shift[r] = first;
}

int lanes_per_read(int cands) { return cands <= 2 ? 2 : cands <= 4 ? 4 : 8; }

int launch_verify(const uint8_t* bases, const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const uint64_t* cand,
                  const uint64_t* masks, const int32_t* lens, int32_t max_len, int L, int32_t cands, const int32_t* max_dist,
                  const int32_t* shift, int anchored, int32_t* out, void* stream) {
  if (n_reads <= 0) return 0;
  const int rpw = 64 / L, W = (max_len + 63) / 64;
  const dim3 grid((n_reads + rpw - 1) / rpw), block(64);
  const hipStream_t s = (hipStream_t)stream;
  if (max_len <= 128)                                          // the form, once per launch, from the index's longest oligo
    hipLaunchKernelGGL(mq_verify<2>, grid, block, 0, s, bases, win_off, n_bases, n_reads, cand, masks, lens, W, L, cands, max_dist, shift, anchored, out);
  else if (max_len <= 256)
    hipLaunchKernelGGL(mq_verify<4>, grid, block, 0, s, bases, win_off, n_bases, n_reads, cand, masks, lens, W, L, cands, max_dist, shift, anchored, out);
  else
    hipLaunchKernelGGL(mq_verify<0>, grid, block, 0, s, bases, win_off, n_bases, n_reads, cand, masks, lens, W, L, cands, max_dist, shift, anchored, out);
  return (int)hipGetLastError();
}

}  // namespace

int launch_mq_verify(const uint8_t* bases, const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const uint64_t* cand,
                     const uint64_t* masks, const int32_t* lens, int32_t max_len, int32_t cands, const int32_t* max_dist,
                     int32_t* out, void* stream) {
  return launch_verify(bases, win_off, n_bases, n_reads, cand, masks, lens, max_len, lanes_per_read(cands), cands, max_dist, nullptr, 0, out,
                       stream);
}

int launch_mq_start(const uint8_t* bases, const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const uint64_t* masks,
                    const int32_t* lens, int32_t max_len, const int32_t* shift, int32_t* out, void* stream) {
  return launch_verify(bases, win_off, n_bases, n_reads, nullptr, masks, lens, max_len, 1, 0, nullptr, shift, 1, out, stream);
}

int launch_mq_flank(const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const int32_t* out, int32_t min_flank,
                    int32_t* flank_off, int32_t* flank_len, int32_t* flank_shift, void* stream) {
  if (n_reads <= 0) return 0;
  hipLaunchKernelGGL(mq_flank, dim3((n_reads + 255) / 256), dim3(256), 0, (hipStream_t)stream, win_off, n_bases, n_reads, out, min_flank,
                     flank_off, flank_len, flank_shift);
  return (int)hipGetLastError();
}

}  // namespace lva
