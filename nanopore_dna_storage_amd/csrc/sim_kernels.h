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

// One wavefront per read: message, encode, flanks, reverse complement, channel, path and dwell.
//   posinfo [oligo_len]: message bits consumed before the position | block type << 12;  cdf [dwell_k];
//   bc [2 * kSimMaxBarcode]: start barcode, end barcode as 0..3 (read only when p.barcoded).
// row_off == nullptr: the lengths-only pass, lens [n_reads][2] = (bases, blocks) of every read.
// Otherwise the fill pass: msgs [n_reads][msg_len], bases [base_off[n]], true_idx [row_off[n]] are written inside each read's
// slice of the offsets only; a read whose lengths differ from its slice sets *bad.
int launch_sim_strand(const SimParams& p, int32_t n_reads, const uint16_t* posinfo, const uint32_t* cdf, const uint8_t* bc,
                      const int64_t* row_off, const int64_t* base_off, int32_t* lens, uint8_t* msgs, uint8_t* bases,
                      uint8_t* true_idx, int32_t* bad, void* stream);

// scores [row_off[n]][40] from the noise stream and true_idx: one 16-byte quad per lane.  10 * blocks < 2^32.
int launch_sim_scores(const SimParams& p, int32_t n_reads, const int64_t* row_off, uint32_t blocks, const uint8_t* true_idx,
                      float scale, float margin, float clip, float* scores, void* stream);

}  // namespace lva
