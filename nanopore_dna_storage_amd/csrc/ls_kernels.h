// ls_kernels.h -- launchers of the kernels in ls_kernels.hip: what happens to a decoded list (DESIGN.md section 1,
// row N2): CRC-8 / index filter, per-index consensus, per-read statistics.  All pointers are device pointers; `msgs`
// is the decoder's output layout uint8 [n_reads][list_size][msg_len] of 0/1 with counts int32 [n_reads], and has to
// start on a 4-byte boundary inside an allocation that ends on one (the kernels read it a dword at a time).
// Every launcher returns a hipError_t as int and launches nothing for n_reads <= 0.
#pragma once
#include <cstdint>

namespace lva {

constexpr int kLsMaxMsgLen = 255;      // bits of a message: four 64-bit words hold one
constexpr int kLsStatFields = 6;       // int32 per read of ls_stats' output = the fields of lva_list_stat
constexpr int kLsPackWords = 8;        // uint64 per read of ls_stats' scratch: truth and top entry as bit words

// Dynamic LDS of ls_filter for this shape (at most 64 * 255 + 16 bytes).
uint32_t ls_filter_lds_bytes(int32_t use_entries, uint32_t msg_len);
// One wavefront per read, lanes over list entries: first entry among the first min(counts[i], use_entries) whose
// CRC-8 checks and whose de-randomised index is < num_oligos.  msg_len = 12 + 8 * bytes_per_oligo + 8 + (pad ? 1 : 0).
// out_index / out_rank [n_reads] (-1: none), out_payload [n_reads][bytes_per_oligo] (zeros: none).
int launch_ls_filter(const uint8_t* msgs, const int32_t* counts, int32_t n_reads, int32_t list_size, uint32_t msg_len,
                     int32_t use_entries, int32_t bytes_per_oligo, int32_t num_oligos, int32_t pad, int32_t* out_index,
                     int32_t* out_rank, uint8_t* out_payload, void* stream);
// index [n_reads] (< 0: the read passed no entry and is skipped; otherwise < num_oligos), payload [n_reads][bytes_per_oligo].
// Scratch: bucket [num_oligos + 1] and order [n_reads] int32.  Three launches: members per index, their prefix sums,
// then one wavefront per index lists its reads in read order and takes the vote.
// present [num_oligos], out_payload [num_oligos][bytes_per_oligo] (zeros: absent), votes [num_oligos] (0: absent).
int launch_ls_consensus(const int32_t* index, const uint8_t* payload, int32_t n_reads, int32_t bytes_per_oligo,
                        int32_t num_oligos, int32_t first_only, int32_t* bucket, int32_t* order, uint8_t* present,
                        uint8_t* out_payload, int32_t* votes, void* stream);
// The first two launches of the consensus alone, for a consumer of its own (tr_kernels.hip): bucket [num_oligos + 1] =
// where the reads of every index begin in a list of the reads index by index (members per index, then prefix sums).
int launch_ls_bucket_scan(const int32_t* index, int32_t n_reads, int32_t num_oligos, int32_t* bucket, void* stream);
// truth [n_reads][msg_len]; packed [n_reads][kLsPackWords] uint64 scratch; out [n_reads][kLsStatFields] int32:
// top_correct, list_correct, hamming, hamming8, hamming16, edit (all -1 for a read without a list).
// Two launches: one wavefront per read for everything but the edit distance, then one thread per read for it.
int launch_ls_stats(const uint8_t* msgs, const int32_t* counts, const uint8_t* truth, int32_t n_reads, int32_t list_size,
                    uint32_t msg_len, uint64_t* packed, int32_t* out, void* stream);

}  // namespace lva
