// sim_strand.h -- the body of the simulator's strand kernel, for its two kernels: sim_strand (sim_kernels.hip: a random
// message per read, stream 0) and sim_strand_pool (sim_pool_kernels.hip: the message is an entry of a pool, stream 6).
// Device code only; everything behind the message is the same code in both.
#pragma once
#include <hip/hip_runtime.h>

#include "philox.h"
#include "sim_kernels.h"

namespace lva {

constexpr int kSimMaxEmit = 5 * kSimMaxStrand + 4;     // 4 insertions + the base per position, 4 more behind the last
constexpr int kSimMaxBits = 544;                       // mem_conv initial bits + message + termination (2 * 255 + 14 at most)

__device__ __forceinline__ uint32_t pick(const U4& v, uint32_t i) {      // v[i] without an indexed register array
  return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}

// inclusive scans over the wavefront
__device__ __forceinline__ int wave_scan_add(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}
__device__ __forceinline__ int wave_scan_max(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d, 64);
    if (lane >= d) v = max(v, t);
  }
  return v;
}

__device__ __forceinline__ uint32_t transition_index(uint32_t frm, uint32_t to) { return to < 4 ? to * 8 + frm : 32 + frm; }

// One workgroup of one wavefront per read; lane = position, 64 positions per pass.  kPool: the message is an entry of
// pl.msgs chosen by stream 6 instead of stream 0's bits, and rc_mode 3 takes the orientation from the same draw; the draw
// and the search of pl.cdf are the same for every lane, so they are pinned to scalar registers and scalar loads.  (!kPool:
// pl is not read.)
template <bool kPool>
__device__ __forceinline__ void sim_strand_body(const SimParams& p, const SimPool& pl, const uint16_t* __restrict__ posinfo,
                                                const uint32_t* __restrict__ cdf, const uint8_t* __restrict__ bc,
                                                const int64_t* __restrict__ row_off, const int64_t* __restrict__ base_off,
                                                int32_t* __restrict__ lens, uint8_t* __restrict__ msgs,
                                                uint8_t* __restrict__ bases, uint8_t* __restrict__ true_idx,
                                                int32_t* __restrict__ bad) {
  __shared__ uint8_t xb[kSimMaxBits];        // the register's bit sequence: initial state, message, termination
  __shared__ uint8_t src[kSimMaxStrand];     // the strand the channel reads
  __shared__ uint8_t em[kSimMaxEmit + 60];   // the bases it emits
  __shared__ uint32_t s_cdf[kSimMaxDwell];
  const int lane = (int)threadIdx.x;
  const uint32_t r = blockIdx.x, R = p.first_read + r;
  const bool fill = row_off != nullptr;
  const uint32_t m = p.mem_conv, total = p.msg_len + m;

  // ---- the pool entry and the coin (stream 6): first k with w0 < pl.cdf[k], else n - 1; without a table mulhi(w0, n)
  uint32_t entry = 0;
  bool coin = false;
  if constexpr (kPool) {
    const U4 S = philox(0, 0, R, kStreamSource, p.k0, p.k1);
    const uint32_t w0 = __builtin_amdgcn_readfirstlane(S.x);
    coin = p.rc_mode == 3 && (__builtin_amdgcn_readfirstlane(S.y) >> 31);
    if (pl.cdf == nullptr) {
      entry = __umulhi(w0, pl.n);
    } else {
      uint32_t lo = 0, hi = pl.n - 1;              // the answer is in [lo, hi]
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (w0 < pl.cdf[mid]) hi = mid; else lo = mid + 1;
      }
      entry = lo;
    }
    entry = __builtin_amdgcn_readfirstlane(entry);
  }
  const uint8_t* __restrict__ mine = kPool ? pl.msgs + (size_t)entry * p.msg_len : nullptr;

  // ---- message (stream 0, or the pool entry: lane = bit) and the bits around it
  for (uint32_t jp = (uint32_t)lane; jp < total + m; jp += 64) {
    uint32_t bit;
    if (jp < m) {
      bit = (p.init >> jp) & 1u;
    } else if (jp - m < p.msg_len) {
      const uint32_t i = jp - m;
      if constexpr (kPool) {
        bit = mine[i];
      } else {
        const U4 w = philox(i >> 7, 0, R, kStreamMessage, p.k0, p.k1);
        bit = (pick(w, (i >> 5) & 3u) >> (i & 31u)) & 1u;
      }
      if (fill) msgs[(size_t)r * p.msg_len + i] = (uint8_t)bit;
    } else {
      bit = (p.fin >> (jp - m - p.msg_len)) & 1u;
    }
    xb[jp] = (uint8_t)bit;
  }
  if ((uint32_t)lane < p.dwell_k) s_cdf[lane] = cdf[lane];
  __syncthreads();

  // ---- strand: the oligo alone, or flank + start barcode + oligo + end barcode + flank (stream 4), reverse complement
  const U4 L = philox(0, 0, R, kStreamLead, p.k0, p.k1);
  uint32_t f5 = 0, f3 = 0, o0 = 0, n = p.oligo_len;
  if (p.barcoded) {
    f5 = p.flank_lo + __umulhi(L.y, p.flank_span);
    f3 = p.flank_lo + __umulhi(L.z, p.flank_span);
    o0 = f5 + p.len_start;
    n = o0 + p.oligo_len + p.len_end + f3;
  }
  const bool rc = p.rc_mode == 1 || (p.rc_mode == 2 && (R & 1u)) || coin;
  for (uint32_t i = (uint32_t)lane; i < n; i += 64) {
    uint32_t b;
    if (i < f5 || i >= n - f3) {
      const U4 w = philox(1 + (i >> 6), 0, R, kStreamLead, p.k0, p.k1);
      b = (pick(w, (i >> 4) & 3u) >> (2 * (i & 15u))) & 3u;
    } else if (i < o0) {
      b = bc[i - f5];
    } else if (i >= o0 + p.oligo_len) {
      b = bc[kSimMaxBarcode + i - o0 - p.oligo_len];
    } else {
      // lva_encode (Code::encode): the register at message step s is bits xb[s .. s + m], oldest first
      const uint32_t info = posinfo[i - o0], s0 = info & 0xFFFu, T = info >> 12;
      uint32_t reg0 = 0, reg1 = 0;
      for (uint32_t a = 0; a <= m; ++a) {
        reg0 |= (uint32_t)xb[s0 + a] << a;
        reg1 |= (uint32_t)xb[s0 + 1 + a] << a;      // (xb is padded: s0 + 1 + m < kSimMaxBits)
      }
      uint32_t hi, lo;
      if (T == 0) {
        hi = __popc(reg0 & p.g0) & 1u;
        lo = __popc(reg0 & p.g1) & 1u;
      } else {                                      // two message bits: two of the four parity bits survive
        hi = __popc(reg0 & ((T & 1u) ? p.g1 : p.g0)) & 1u;
        lo = __popc(reg1 & (T == 1 ? p.g0 : p.g1)) & 1u;
      }
      b = 2 * hi + lo;
    }
    src[rc ? n - 1 - i : i] = (uint8_t)(rc ? 3u - b : b);
  }
  __syncthreads();

  // ---- channel (stream 1): position i emits its insertions, then its own base unless deleted
  int nb = 0;
  for (uint32_t i0 = 0; i0 <= n; i0 += 64) {
    const uint32_t i = i0 + (uint32_t)lane;
    const U4 A = philox(i, 0, R, kStreamChannel, p.k0, p.k1), B = philox(i, 1, R, kStreamChannel, p.k0, p.k1);
    int c = 0;
    if (A.x < p.thr_ins) { c = 1; if (A.y < p.thr_ins) { c = 2; if (A.z < p.thr_ins) { c = 3; if (A.w < p.thr_ins) c = 4; } } }
    const bool keep = i < n && !(B.y < p.thr_del);
    const uint32_t s = i < n ? src[i] : 0u;
    const uint32_t own = B.z < p.thr_sub ? (s + 1u + __umulhi(B.w, 3u)) & 3u : s;
    const int e = i <= n ? c + (keep ? 1 : 0) : 0;
    const int incl = wave_scan_add(e, lane);
    int at = nb + incl - e;
    if (i <= n) {
      for (int k = 0; k < c; ++k) em[at++] = (uint8_t)((B.x >> (2 * k)) & 3u);
      if (keep) em[at] = (uint8_t)own;
    }
    nb += __shfl(incl, 63, 64);
  }
  __syncthreads();

  // ---- path and dwell (stream 2): states by synth.state_path's rule, one transition block and d stay blocks per base
  const uint32_t lead = ((nb ? (uint32_t)em[0] : 0u) + 1u + __umulhi(L.x, 3u)) & 3u;
  const int64_t row0 = fill ? row_off[r] : 0, base0 = fill ? base_off[r] : 0;
  const int64_t rows = fill ? row_off[r + 1] - row0 : 0, nbase = fill ? base_off[r + 1] - base0 : 0;
  int run_carry = 0, blocks = 0;
  uint32_t st_carry = lead;
  for (int j0 = 0; j0 < nb; j0 += 64) {
    const int j = j0 + lane;
    const bool act = j < nb;
    const uint32_t b = act ? em[j] : 0u;
    const bool start = act && (j == 0 || em[j - 1] != b);
    const int run = max(wave_scan_max(start ? j : -1, lane), run_carry);      // where the run of equal bases began
    const uint32_t st = b + 4u * (uint32_t)((j - run) & 1);
    uint32_t prev = __shfl_up(st, 1, 64);
    if (lane == 0) prev = st_carry;
    run_carry = __shfl(run, 63, 64);
    st_carry = __shfl(st, 63, 64);
    const U4 w4 = philox((uint32_t)j >> 2, 0, R, kStreamDwell, p.k0, p.k1);
    const uint32_t w = pick(w4, (uint32_t)j & 3u);
    int d = (int)p.dwell_k;
    for (int e = (int)p.dwell_k - 1; e >= 0; --e)
      if (w < s_cdf[e]) d = e;
    const int mine = act ? 1 + d : 0;
    const int incl = wave_scan_add(mine, lane);
    const int64_t at = 1 + blocks + incl - mine;              // the block of this base's transition
    if (fill && act) {
      if (j < nbase) bases[base0 + j] = (uint8_t)b;
      if (at < rows) true_idx[row0 + at] = (uint8_t)transition_index(prev, st);
      const uint8_t stay = (uint8_t)transition_index(st, st);
      for (int q = 1; q <= d; ++q)
        if (at + q < rows) true_idx[row0 + at + q] = stay;
    }
    blocks += __shfl(incl, 63, 64);
  }
  if (lane == 0) {
    if (!fill) {
      lens[2 * r] = nb;
      lens[2 * r + 1] = 1 + blocks;
    } else {
      if (rows > 0) true_idx[row0] = (uint8_t)(lead * 9u);     // one leading stay block
      if constexpr (kPool) {
        pl.source[r] = (int32_t)entry;
        pl.rc[r] = (uint8_t)rc;
      }
      if (nbase != nb || rows != 1 + blocks) *bad = 1;
    }
  }
}

}  // namespace lva
