// ep_kernels.hip -- DESIGN.md section 1 row N5: the error profile of a set of reads, on the device.
//
// The reference measures its channel outside the decoder:
//   util/align_compute_stats.sh:45-52     minimap2 maps the basecalls to the oligos, samtools stats counts
//   util/compile_plot_stats.py            mismatches, insertions and deletions per position -> <prefix>.error_stats.csv
// Here a read names its oligo already (the index that lva_list_filter accepted, or the simulator's truth), so what is
// left is the alignment and the tally, in two kernels per chunk of reads:
//   ep_fill   one wavefront per read fills the unit-cost edit-distance matrix D and writes, for every inner cell, the
//             move the walk takes from it;
//   ep_walk   one thread per read walks back from (ref_len, n) and adds to the tallies with integer atomics.
// The move order (diagonal, then up, then left) is part of the definition (error_profile.reference_profile): homopolymers
// make ties the normal case.  Integer work throughout: every result is exact and independent of the order of the atomics.
//
// ep_fill.  Lane l of stripe s owns reference row i = 64 s + l + 1 and moves along it one column per step; at step t
// it is at column j = t - l + 1, so the wavefront works on an anti-diagonal.  D[i-1][j] is what the lane above computed
// one step ago and D[i-1][j-1] what it computed two steps ago: one __shfl_up per step, kept for one more step.  Lane 0
// reads both from the bottom row of the stripe above (LDS, 16-bit: D <= 4096), lane 63 writes the bottom row of its own
// stripe to the other of two buffers.  The codes of one step form one 64-byte line: coalesced stores in the fill, and the
// walk finds cell (i, j) at line (stripe, t = j - 1 + l), byte l.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ep_kernels.h"

namespace lva {

namespace {

constexpr int kMoveDiag = 0, kMoveUp = 1, kMoveLeft = 2;

// base j (from 0) of the window w of n bytes as it is aligned: reverse-complemented if flip
__device__ __forceinline__ uint32_t read_base(const uint8_t* w, int n, int j, bool flip) {
  if (!flip) return base_code(w[j]);
  return complement_code(base_code(w[n - 1 - j]));
}

// N equals nothing, itself included
__device__ __forceinline__ bool same_base(uint32_t a, uint32_t b) { return a == b && a < kBaseN; }

// grid = reads of the chunk, block = one wavefront
__global__ __launch_bounds__(64) void ep_fill(const uint8_t* __restrict__ bases, const int32_t* __restrict__ win_off,
                                              const int32_t* __restrict__ n_bases, const uint8_t* __restrict__ refs, int ref_len,
                                              const int32_t* __restrict__ ref_id, const uint8_t* __restrict__ rc,
                                              const int64_t* __restrict__ move_off, uint8_t* __restrict__ moves) {
  __shared__ uint8_t rd[kMaxRead];                       // the window as it is aligned, 0..4
  __shared__ uint16_t row[2][kMaxRead + 1];              // D[64 s][0 .. n]: the row above stripe s, and the one it leaves
  const int lane = threadIdx.x;
  const size_t r = blockIdx.x;
  const int id = ref_id[r], n = n_bases[r];
  if (id < 0 || n <= 0) return;                          // uniform; an empty window is all deletions: the walk reads no code
  const uint8_t* w = bases + win_off[r];
  const bool flip = rc[r] != 0;
  for (int j = lane; j < n; j += 64) rd[j] = (uint8_t)read_base(w, n, j, flip);
  for (int j = lane; j <= n; j += 64) row[0][j] = (uint16_t)j;
  __syncthreads();
  const uint8_t* ref = refs + (size_t)id * (size_t)ref_len;
  uint8_t* mv = moves + move_off[r];
  const int steps = n + kEpStripe - 1;
  const int stripes = (ref_len + kEpStripe - 1) / kEpStripe;
  for (int s = 0; s < stripes; ++s) {
    const uint16_t* prev = row[s & 1];
    uint16_t* next = row[(s & 1) ^ 1];
    const int i = kEpStripe * s + lane + 1;
    const bool live = i <= ref_len;                      // a lane past the last row computes along and writes nothing
    const uint32_t rb = live ? base_code(ref[i - 1]) : kBaseN;
    int mine = i;                                        // D[i][j - 1], at first D[i][0]
    int diag = i - 1;                                    // D[i - 1][j - 1], at first D[i - 1][0]
    if (lane == 63) next[0] = (uint16_t)i;
    uint8_t* line = mv + (size_t)s * (size_t)steps * kEpStripe + lane;
    for (int t = 0; t < steps; ++t) {
      const int j = t - lane + 1;
      const bool on = j >= 1 && j <= n;
      int up = __shfl_up(mine, 1);                       // D[i - 1][j]: the lane above was at column j one step ago
      if (lane == 0) up = on ? (int)prev[j] : 0;
      if (on) {
        const int dg = diag + (same_base(rb, rd[j - 1]) ? 0 : 1), u = up + 1, l = mine + 1;
        const int d = min(dg, min(u, l));
        if (live) line[(size_t)t * kEpStripe] = (uint8_t)(dg == d ? kMoveDiag : u == d ? kMoveUp : kMoveLeft);
        mine = d;
        if (lane == 63) next[j] = (uint16_t)d;
      }
      diag = up;
    }
    __syncthreads();                                     // the bottom row is complete before the next stripe reads it
  }
}

__device__ __forceinline__ void tally(int64_t* at) { atomicAdd(reinterpret_cast<unsigned long long*>(at), 1ull); }

// grid = reads of the chunk / 64, one thread per read: at most ref_len + n moves, each one code byte
__global__ __launch_bounds__(64) void ep_walk(const uint8_t* __restrict__ bases, const int32_t* __restrict__ win_off,
                                              const int32_t* __restrict__ n_bases, int n_reads, const uint8_t* __restrict__ refs,
                                              int ref_len, const int32_t* __restrict__ ref_id, const uint8_t* __restrict__ rc,
                                              const int64_t* __restrict__ move_off, const uint8_t* __restrict__ moves,
                                              int32_t* __restrict__ out_read, int64_t* __restrict__ pos, int64_t* __restrict__ conf,
                                              int64_t* __restrict__ ins) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= n_reads) return;
  int32_t* o = out_read + (size_t)r * 4;
  const int id = ref_id[r];
  if (id < 0) { o[0] = o[1] = o[2] = o[3] = -1; return; }
  const int n = n_bases[r];
  const uint8_t* w = bases + win_off[r];
  const bool flip = rc[r] != 0;
  const uint8_t* ref = refs + (size_t)id * (size_t)ref_len;
  const uint8_t* mv = moves + move_off[r];
  const size_t steps = (size_t)(n + kEpStripe - 1);
  int i = ref_len, j = n, nsub = 0, ndel = 0, nins = 0;
  while (i > 0 || j > 0) {                               // every move lowers i + j
    int code;
    if (i == 0) code = kMoveLeft;
    else if (j == 0) code = kMoveUp;
    else {
      const int l = (i - 1) & (kEpStripe - 1);
      code = mv[((size_t)((i - 1) / kEpStripe) * steps + (size_t)(j - 1 + l)) * kEpStripe + l];
    }
    if (code == kMoveDiag) {                             // match or substitution at position i - 1
      const uint32_t rb = base_code(ref[i - 1]), qb = read_base(w, n, j - 1, flip);
      const bool eq = same_base(rb, qb);
      tally(pos + (size_t)(i - 1) * 4 + (eq ? 0 : 1));
      if (rb < kBaseN) tally(conf + rb * 6 + qb);
      nsub += eq ? 0 : 1;
      --i; --j;
    } else if (code == kMoveUp) {                        // deletion at position i - 1
      const uint32_t rb = base_code(ref[i - 1]);
      tally(pos + (size_t)(i - 1) * 4 + 2);
      if (rb < kBaseN) tally(conf + rb * 6 + 5);
      ++ndel;
      --i;
    } else {                                             // insertion in front of position i
      tally(pos + (size_t)i * 4 + 3);
      tally(ins + read_base(w, n, j - 1, flip));
      ++nins;
      --j;
    }
  }
  o[0] = nsub + ndel + nins;                             // the walk's moves cost D[ref_len][n]
  o[1] = nsub; o[2] = ndel; o[3] = nins;
}

}  // namespace

int launch_ep_fill(const uint8_t* bases, const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const uint8_t* refs,
                   int32_t ref_len, const int32_t* ref_id, const uint8_t* rc, const int64_t* move_off, uint8_t* moves, void* stream) {
  if (n_reads <= 0) return 0;
  hipLaunchKernelGGL(ep_fill, dim3(n_reads), dim3(64), 0, (hipStream_t)stream, bases, win_off, n_bases, refs, ref_len, ref_id, rc,
                     move_off, moves);
  return (int)hipGetLastError();
}

int launch_ep_walk(const uint8_t* bases, const int32_t* win_off, const int32_t* n_bases, int32_t n_reads, const uint8_t* refs,
                   int32_t ref_len, const int32_t* ref_id, const uint8_t* rc, const int64_t* move_off, const uint8_t* moves,
                   int32_t* out_read, int64_t* pos, int64_t* conf, int64_t* ins, void* stream) {
  if (n_reads <= 0) return 0;
  hipLaunchKernelGGL(ep_walk, dim3((n_reads + 63) / 64), dim3(64), 0, (hipStream_t)stream, bases, win_off, n_bases, n_reads, refs,
                     ref_len, ref_id, rc, move_off, moves, out_read, pos, conf, ins);
  return (int)hipGetLastError();
}

}  // namespace lva
