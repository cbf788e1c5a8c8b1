// sim_kernels.h -- launchers of the kernels in sim_kernels.hip: the read simulator.  The
// definition they are held to, draw by draw, is nanopore_dna_storage_amd/simulate.py.
#pragma once
#include <cstdint>

namespace lva {

constexpr int kSimMaxBarcode = 64;     // bases of one barcode
constexpr int kSimMaxFlank = 256;      // bases of one flank
constexpr int kSimMaxStrand = 1024;    // flanks + barcodes + oligo: what one workgroup keeps in LDS
constexpr int kSimMaxDwell = 64;       // entries of the dwell table
constexpr uint32_t kSimMaxThreshold = 1u << 30;   // probability 0.25

// What a read is drawn from, apart from its number.  Not part of the C ABI.
struct SimParams {
  uint32_t k0, k1;                     // the seed: Philox key
  uint32_t first_read;
  uint32_t thr_sub, thr_del, thr_ins;  // floor(p * 2^32)
  uint32_t dwell_k;
  uint32_t msg_len, mem_conv, g0, g1, init, fin, oligo_len;
  uint32_t barcoded, len_start, len_end, flank_lo, flank_span, rc_mode;
};

// The pool a read's message is drawn from (stream 6), on the device.  Not part of the C ABI.
struct SimPool {
  const uint8_t* msgs = nullptr;       // [n][msg_len] of 0 / 1, n * msg_len < 2^31
  const uint32_t* cdf = nullptr;       // [n] non-decreasing, last entry 0xFFFFFFFF; nullptr: uniform
  uint32_t n = 0;                      // 1 .. kSimMaxPool
  int32_t* source = nullptr;           // [n_reads], written by the fill pass: the entry of every read
  uint8_t* rc = nullptr;               // [n_reads], written by the fill pass: 1 where the strand was reverse-complemented
};
constexpr int32_t kSimMaxPool = 1 << 24;

// One wavefront per read: message, encode, flanks, reverse complement, channel, path and dwell.
// pool == nullptr: the message is stream 0's and rc_mode is 0..2; otherwise an entry of the pool, rc_mode 0..3.
//   posinfo [oligo_len]: message bits consumed before the position | block type << 12;  cdf [dwell_k];
//   bc [2 * kSimMaxBarcode]: start barcode, end barcode as 0..3 (read only when p.barcoded).
// row_off == nullptr: the lengths-only pass, lens [n_reads][2] = (bases, blocks) of every read.
// Otherwise the fill pass: msgs [n_reads][msg_len], bases [base_off[n]], true_idx [row_off[n]] are written inside each read's
// slice of the offsets only; a read whose lengths differ from its slice sets *bad.
int launch_sim_strand(const SimParams& p, const SimPool* pool, int32_t n_reads, const uint16_t* posinfo, const uint32_t* cdf,
                      const uint8_t* bc, const int64_t* row_off, const int64_t* base_off, int32_t* lens, uint8_t* msgs,
                      uint8_t* bases, uint8_t* true_idx, int32_t* bad, void* stream);
// the pool kernel alone (sim_pool_kernels.hip); launch_sim_strand calls it when it is given a pool
int launch_sim_strand_pool(const SimParams& p, const SimPool& pool, int32_t n_reads, const uint16_t* posinfo, const uint32_t* cdf,
                           const uint8_t* bc, const int64_t* row_off, const int64_t* base_off, int32_t* lens, uint8_t* msgs,
                           uint8_t* bases, uint8_t* true_idx, int32_t* bad, void* stream);

// scores [row_off[n]][40] from the noise stream and true_idx: one 16-byte quad per lane.  10 * blocks < 2^32.
int launch_sim_scores(const SimParams& p, int32_t n_reads, const int64_t* row_off, uint32_t blocks, const uint8_t* true_idx,
                      float scale, float margin, float clip, float* scores, void* stream);

}  // namespace lva
