// tr_kernels.h -- launchers of the kernels in tr_kernels.hip: reading-cost trials (DESIGN.md section 1, row N4'): many
// random samples of the reads, each voted on per index and RS-decoded, several sample sizes per trial.  The definition is
// nanopore_dna_storage_amd/trials.py.  All pointers are device pointers.  A call works on a chunk of `chunk` consecutive
// trials; "kt" below is (point k, trial j of the chunk) = k * chunk + j, and s = bpo / 2 is the number of 16-bit columns.
// Every launcher returns a hipError_t as int.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace lva {

constexpr int kTrMaxPoints = 64;
constexpr size_t kTrGexpWords = 2 * 65535 + 2, kTrGlogWords = 65536;      // the GF(2^16) tables of the RS decode

struct TrShape {
  int32_t n_reads, bpo, num_oligos, fec, n_points, chunk;
  uint32_t k0, k1;               // the seed: Philox key, low and high word
  uint32_t first_trial;          // trial number of the chunk's first trial
  int32_t points[kTrMaxPoints];  // sample sizes, ascending, each in [0, n_reads]
};

// the tables rs_decode_codeword reads (host side; upload ex [kTrGexpWords] and lg [kTrGlogWords])
void tr_gf_tables(std::vector<uint16_t>* ex, std::vector<uint16_t>* lg);

// One wavefront per index: order [n_reads] = the reads index by index, each index's in read order, index x's from
// bucket[x] on (bucket [num_oligos + 1]: launch_ls_bucket_scan).  Once per call: it does not depend on the trial.
int launch_tr_bucket_list(const int32_t* index, int32_t n_reads, int32_t num_oligos, const int32_t* bucket, int32_t* order,
                          void* stream);
// One wavefront per (index, trial): bucket / order as above, payload [n_reads][bpo].  Scratch place, cnt: int32 [chunk][n_reads].  Writes, for every kt and index x:
//   nmem [kt][num_oligos]        reads of index x inside the sample (0: the index is absent)
//   sym  [kt][s][num_oligos]     the vote's payload as little-endian 16-bit symbols, 0x3030 where absent: the RS input
//   cons [kt][num_oligos][bpo]   (null: not wanted) the same payload as bytes, zeros where absent
int launch_tr_consensus(const TrShape& sh, const int32_t* bucket, const int32_t* order, const uint8_t* payload, int32_t* place,
                        int32_t* cnt, int32_t* nmem, uint16_t* sym, uint8_t* cons, void* stream);
// One wavefront per kt: erl [kt][num_oligos] the absent indices ascending, ern [kt] how many, pp [kt][2] = reads inside the
// sample that carry an index (passed), indices present; pres [kt][num_oligos] (null: not wanted) 1 where present.
int launch_tr_erasures(const TrShape& sh, const int32_t* nmem, int32_t* erl, int32_t* ern, int32_t* pp, uint8_t* pres, void* stream);
// One workgroup per codeword (kt, column c): the decode of rs_decode_kernel with the erasure list of kt, into
// dec [kt][s][num_oligos - fec]; then the comparison with truth [s][num_oligos - fec] (the original file's columns, zero
// behind its end) on the bytes that lie below original_bytes.  okeq [kt][s][2] = (the decoder did not give up, equal).
int launch_tr_decode(const TrShape& sh, const uint16_t* sym, const int32_t* erl, const int32_t* ern, const uint16_t* gexp,
                     const uint16_t* glog, uint16_t* dec, const uint16_t* truth, int64_t original_bytes, int32_t* okeq, void* stream);
// One thread per kt: stats [n_points][n_trials][4] = (passed, present, columns_ok, success) at trial trial_at + j.
int launch_tr_fold(const TrShape& sh, const int32_t* okeq, const int32_t* pp, int32_t* stats, int32_t n_trials, int32_t trial_at,
                   void* stream);

}  // namespace lva
