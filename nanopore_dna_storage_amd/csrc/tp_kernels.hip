// tp_kernels.hip -- gfx950 kernels of DESIGN.md section 1 row N0: the step in front of everything else on the
// device.  A flip-flop CRF network emits transition SCORES; flappie turns them into the transition log-posteriors
// a .post file holds with a forward-backward pass over the 8 flip-flop states
// (transpost_crf_flipflop, flappie/src/decode.c:377-497, then log_row_normalise_inplace, flappie_matrix.c:450-467).
//   tp_forward    alpha[blk][s]: log-sum over the paths that are in state s before block blk, 8 floats per block
//                 to the decoder's scratch buffer.
//   tp_backward   beta, the five posteriors every source state owns in a block, their normalisation over the
//                 block's 40 entries, written over the scores the same lane has read (in place is allowed).
// Both are bc_basecall's shape (bc_kernels.hip): 8 lanes per read, 8 reads per wavefront, a dependent chain of
// nblk steps.  The arithmetic is sum-product in fp32: max, then one expf per candidate and one logf per state and
// step.  alpha and beta are carried relative to the largest entry of the previous step's vector -- a constant per
// block that the normalisation removes -- so their magnitude stays that of a few scores however long the read is
// (flappie's grow by about 5 per block and lose absolute precision with them).
// No address depends on the data: non-finite scores give whatever IEEE arithmetic gives for that read alone.
#include <hip/hip_runtime.h>

#include <cmath>

#include "tp_kernels.h"

namespace lva {

namespace {
constexpr uint32_t kTpChunk = 4;       // blocks per chunk: the next chunk's rows are in flight while this one is consumed

__device__ __forceinline__ float max8(const float (&v)[8]) {
  return fmaxf(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7])));
}
}  // namespace

// Lane s of a group is TARGET state s (0-3 flip, 4-7 flop).  A flip target reads the 8 scores into it (32 contiguous
// bytes, as bc_basecall::load_block does); a flop target needs two of the 8 floats of the flop row and reads the
// whole row -- the four flop lanes of a group ask for the same 32 bytes -- so that every lane issues the same two
// 16-byte requests and a chunk is 2 * kTpChunk requests in a row with no branch between them.  Block indices are
// clamped into the read instead of guarded: a request past the end re-reads the last block and is never used.
__global__ __launch_bounds__(64) void tp_forward(const float* __restrict__ scores, const int64_t* __restrict__ row_off,
                                                 int32_t n_reads, float* __restrict__ fwd) {
  const uint32_t lane = threadIdx.x, s = lane & 7u, grp = lane & ~7u;
  const int32_t r = blockIdx.x * 8 + (int32_t)(lane >> 3);
  const bool live = r < n_reads;
  const int64_t off = live ? row_off[r] : 0;
  const uint32_t nblk = live ? (uint32_t)(row_off[r + 1] - off) : 0u;
  const uint32_t last = nblk ? nblk - 1u : 0u;
  const bool flip = s < 4u;
  const float* p = (nblk ? scores + off * 40 : scores) + (flip ? s * 8u : 32u);   // an empty read looks at block 0 of the batch
  float* fw = fwd + off * 8 + s;
  const float ninf = -INFINITY;
  auto request = [&](uint32_t blk0, float4 (&a)[kTpChunk], float4 (&b)[kTpChunk]) {
#pragma unroll
    for (uint32_t u = 0; u < kTpChunk; ++u) {
      const uint32_t blk = blk0 + u;
      const float* q = p + (size_t)(blk < last ? blk : last) * 40;
      a[u] = *reinterpret_cast<const float4*>(q);
      b[u] = *reinterpret_cast<const float4*>(q + 4);
    }
  };
  float mine = 0.0f;                                                      // calloc'd first column (decode.c:386)
  auto consume = [&](uint32_t blk0, const float4 (&a)[kTpChunk], const float4 (&b)[kTpChunk]) {
#pragma unroll
    for (uint32_t u = 0; u < kTpChunk; ++u) {
      const uint32_t blk = blk0 + u;
      const bool on = blk < nblk;
      float t[8] = {a[u].x, a[u].y, a[u].z, a[u].w, b[u].x, b[u].y, b[u].z, b[u].w};
      if (!flip) {
        // flop b2 = s: "move from flip" is entry 32 + s - 4, "stay in flop" is entry 32 + s (:403-410); the other six
        // sources do not reach it
#pragma unroll
        for (uint32_t f = 0; f < 8; ++f) t[f] = (f == s || f + 4u == s) ? t[f] : ninf;
      }
      if (on) fw[(size_t)blk * 8] = mine;                                 // alpha before block blk
      float pv[8];
#pragma unroll
      for (int f = 0; f < 8; ++f) pv[f] = __shfl(mine, (int)(grp | (uint32_t)f));
      const float c = max8(pv);                                           // the read's running offset
      float cand[8];
#pragma unroll
      for (int f = 0; f < 8; ++f) cand[f] = t[f] + pv[f];
      const float m = max8(cand);
      float sum = 0.0f;
#pragma unroll
      for (int f = 0; f < 8; ++f) sum += expf(cand[f] - m);
      const float next = (m - c) + logf(sum);
      mine = on ? next : mine;
    }
  };
  // two chunks per trip, each consumed while the other's rows are in flight: no register copies, so no wait on a
  // request before its chunk is consumed
  float4 a0[kTpChunk], b0[kTpChunk], a1[kTpChunk], b1[kTpChunk];
  request(0, a0, b0);
  for (uint32_t blk0 = 0; __any(blk0 < nblk); blk0 += 2 * kTpChunk) {     // forwards pass (:396-423)
    request(blk0 + kTpChunk, a1, b1);
    consume(blk0, a0, b0);
    request(blk0 + 2 * kTpChunk, a0, b0);
    consume(blk0 + kTpChunk, a1, b1);
  }
}

// Lane f of a group is SOURCE state f.  Of a block it owns exactly the five transitions that leave f: into flip b at
// b * 8 + f (b = 0..3) and into flop at 32 + f (to flop f + 4 from flip f, staying in flop f otherwise).  It reads them
// from `scores`, and writes their log-posteriors to the same five places of `post`: the two may be one buffer.  The
// reads of the next chunk (lower blocks) are issued before this chunk's stores, to addresses no store of the read
// has touched yet; no __restrict__ on the two, so the compiler keeps that order.
__global__ __launch_bounds__(64) void tp_backward(const float* scores, const int64_t* __restrict__ row_off, int32_t n_reads,
                                                  const float* __restrict__ fwd, float* post) {
  const uint32_t lane = threadIdx.x, f = lane & 7u, grp = lane & ~7u;
  const int32_t r = blockIdx.x * 8 + (int32_t)(lane >> 3);
  const bool live = r < n_reads;
  const int64_t off = live ? row_off[r] : 0;
  const int32_t nblk = live ? (int32_t)(row_off[r + 1] - off) : 0;
  const float* p = (nblk ? scores + off * 40 : scores) + f;
  const float* fw = (nblk ? fwd + off * 8 : fwd) + f;
  float* o = post + off * 40 + f;
  auto load_block = [&](int32_t blk, float (&t)[5], float& a) {
    const size_t b = (size_t)(blk > 0 ? blk : 0);
    const float* q = p + b * 40;
    t[0] = q[0]; t[1] = q[8]; t[2] = q[16]; t[3] = q[24]; t[4] = q[32];
    a = fw[b * 8];
  };
  float tn[kTpChunk][5], an[kTpChunk];
#pragma unroll
  for (uint32_t u = 0; u < kTpChunk; ++u) load_block(nblk - 1 - (int32_t)u, tn[u], an[u]);
  float mine = 0.0f;                                                      // calloc'd backward vector (decode.c:425)
  for (int32_t top = nblk; __any(top > 0); top -= (int32_t)kTpChunk) {    // backwards pass (:434-484)
    float tc[kTpChunk][5], ac[kTpChunk];
#pragma unroll
    for (uint32_t u = 0; u < kTpChunk; ++u) {
#pragma unroll
      for (int k = 0; k < 5; ++k) tc[u][k] = tn[u][k];
      ac[u] = an[u];
      load_block(top - 1 - (int32_t)(kTpChunk + u), tn[u], an[u]);
    }
#pragma unroll
    for (uint32_t u = 0; u < kTpChunk; ++u) {
      const int32_t blk = top - 1 - (int32_t)u;
      const bool on = blk >= 0;
      float pv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pv[j] = __shfl(mine, (int)(grp | (uint32_t)j));
      const float c = max8(pv);                                           // the read's running offset
      float flop = pv[4];                                                 // beta of the flop state f leads to: 4 + (f & 3)
#pragma unroll
      for (uint32_t j = 1; j < 4; ++j) flop = (f & 3u) == j ? pv[4 + j] : flop;
      float e[5];
#pragma unroll
      for (int b = 0; b < 4; ++b) e[b] = tc[u][b] + pv[b];
      e[4] = tc[u][4] + flop;
      const float m = fmaxf(fmaxf(fmaxf(e[0], e[1]), fmaxf(e[2], e[3])), e[4]);
      float sum = 0.0f;
#pragma unroll
      for (int k = 0; k < 5; ++k) sum += expf(e[k] - m);
      const float next = (m - c) + logf(sum);                             // beta before the block (:466-483)
      // the block's 40 posteriors are alpha[f] + e[k] (:447-462); their log-sum is that of alpha[f] + beta[f] over the
      // group.  xor butterflies: every lane adds the same pairs, so all eight hold the same bits.
      const float z = ac[u] + next;
      float zm = z;
#pragma unroll
      for (int w = 1; w < 8; w <<= 1) zm = fmaxf(zm, __shfl_xor(zm, w));
      float zs = expf(z - zm);
#pragma unroll
      for (int w = 1; w < 8; w <<= 1) zs += __shfl_xor(zs, w);
      const float norm = zm + logf(zs);                                   // log_row_normalise_inplace
      if (on) {
        float* q = o + (size_t)blk * 40;
#pragma unroll
        for (int k = 0; k < 5; ++k) q[k * 8] = (ac[u] + (e[k] - c)) - norm;
        mine = next;
      }
    }
  }
}

int launch_tp_forward(const float* scores, const int64_t* row_off, int32_t n_reads, float* fwd, void* stream) {
  if (n_reads <= 0) return 0;
  hipLaunchKernelGGL(tp_forward, dim3((n_reads + 7) / 8), dim3(64), 0, (hipStream_t)stream, scores, row_off, n_reads, fwd);
  return (int)hipGetLastError();
}

int launch_tp_backward(const float* scores, const int64_t* row_off, int32_t n_reads, const float* fwd, float* post,
                       void* stream) {
  if (n_reads <= 0) return 0;
  hipLaunchKernelGGL(tp_backward, dim3((n_reads + 7) / 8), dim3(64), 0, (hipStream_t)stream, scores, row_off, n_reads, fwd,
                     post);
  return (int)hipGetLastError();
}

}  // namespace lva
