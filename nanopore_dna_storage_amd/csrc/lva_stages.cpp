// lva_stages.cpp -- C ABI (include/lva_decoder.h) of the stages beside the list decoder: transition posteriors (N0), basecall
// and barcode localisation (N3), demultiplexing (N3'), the consumers of a decoded list (N2), reading-cost trials (N4'), the read simulator (S).  No algorithm lives here: an entry
// point checks its arguments, declares its device pieces, uploads, launches, copies back and waits, all through the functions below.
#include <algorithm>
#include <cstring>

#include "lva_host.h"
#include "bc_kernels.h"
#include "tp_kernels.h"
#include "ls_kernels.h"
#include "sim_kernels.h"
#include "tr_kernels.h"

using namespace lva;

namespace {

// bc_search packs (edit distance << 20 | window index) into one word for its minimum reduction
// (bc_kernels.hip): a read may have at most 2^20 blocks / called bases.  Real reads have a few thousand.
constexpr int64_t kBcMaxBlocks = (int64_t)1 << 20;

// THE validation of a ragged batch, from the offsets alone: first offset 0, non-decreasing, at most kBcMaxBlocks per
// read, fewer than 2^31 in all (32-bit block offsets inside the kernels).  Every entry point that takes row_offsets or
// base_offsets calls it before it allocates or copies anything; *total = offsets[n].
int check_offsets(const int64_t* offsets, int32_t n, size_t* total) {
  *total = 0;
  if (n == 0) return LVA_OK;
  if (offsets[0] != 0) return LVA_ERR_ARG;
  for (int32_t i = 0; i < n; ++i)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > kBcMaxBlocks) return LVA_ERR_ARG;
  if (offsets[n] >= ((int64_t)1 << 31)) return LVA_ERR_ARG;
  *total = (size_t)offsets[n];
  return LVA_OK;
}

// per-read counts of a batch that check_offsets has passed
std::vector<int32_t> read_lengths(const int64_t* offsets, int32_t n) {
  std::vector<int32_t> len((size_t)n);
  for (int32_t i = 0; i < n; ++i) len[i] = (int32_t)(offsets[i + 1] - offsets[i]);
  return len;
}

// What every decoder-bound stage does once its own arguments, its barcodes and its offsets have passed (an argument
// error wins over an open stream): busy, nothing to do, device -- in this order.  kRun: there is work, the device is set.
constexpr int kRun = 1;
int stage_enter(lva_decoder* d, bool empty) {
  if (d->open_stream) return LVA_ERR_BUSY;   // a stream owns the decoder's HIP stream, the slots and the profile
  if (empty) return LVA_OK;
  if (hipSetDevice(d->device) != hipSuccess) return LVA_ERR_NO_DEVICE;
  return kRun;
}
int stage_enter(lva_decoder* d, const int64_t* offsets, int32_t n, size_t* total) {     // the offsets, then the above
  return check_offsets(offsets, n, total) != LVA_OK ? LVA_ERR_ARG : stage_enter(d, n == 0);
}

// One device allocation for the length of a call, carved into 256-byte aligned and padded pieces.  The pieces are
// declared first (add), alloc() sizes the block from what was declared, ptr() hands them out: the capacity cannot
// disagree with the pieces.  Declare it before the call's StreamDrain, so that it is freed behind the drain.
class Arena {
  static constexpr size_t kAbsent = ~(size_t)0;

 public:
  template <typename T> struct Piece { size_t at = kAbsent; };   // default: a piece that was not asked for, ptr() = null
  Arena() = default;
  Arena(const Arena&) = delete;
  ~Arena() { if (base_) (void)hipFree(base_); }
  // a piece of count 0 still occupies one padded unit; ls_filter reads whole dwords up to the padded end of its messages
  template <typename T> Piece<T> add(size_t count) {
    Piece<T> p;
    p.at = size_;
    size_ += (std::max<size_t>(count, 1) * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
  int alloc() { return hipMalloc(reinterpret_cast<void**>(&base_), size_) == hipSuccess ? LVA_OK : LVA_ERR_NOMEM; }
  template <typename T> T* ptr(Piece<T> p) const { return p.at == kAbsent ? nullptr : reinterpret_cast<T*>(base_ + p.at); }

 private:
  char* base_ = nullptr;
  size_t size_ = 0;
};

int upload_post(lva_decoder* d, const float* post, size_t blocks, HostPost* hp) {     // blocks: check_offsets' total
  if (hipMalloc(reinterpret_cast<void**>(&hp->dev), std::max<size_t>(blocks, 1) * 160) != hipSuccess) return LVA_ERR_NOMEM;
  if (blocks > 0) HIP_TRY(hipMemcpyAsync(hp->dev, post, blocks * 160, hipMemcpyHostToDevice, d->stream));
  return LVA_OK;
}

// ---------------------------------------------------------------------------------------------
// basecall of the posterior matrix and barcode localisation.
// ---------------------------------------------------------------------------------------------

bool rc_pattern(const char* src, int len, char* dst) {        // helper.reverse_complement (helper.py:227-229)
  for (int i = 0; i < len; ++i) {
    char c;
    switch (src[len - 1 - i]) {
      case 'A': c = 'T'; break;
      case 'C': c = 'G'; break;
      case 'G': c = 'C'; break;
      case 'T': c = 'A'; break;
      case 'N': c = 'N'; break;
      default: return false;
    }
    dst[i] = c;
  }
  return true;
}

int make_patterns(const char* start_bc, const char* end_bc, int n_orient, BcPatterns* p) {
  if (!start_bc || !end_bc) return LVA_ERR_ARG;
  const size_t ls = std::strlen(start_bc), le = std::strlen(end_bc);
  if (ls == 0 || le == 0 || ls > (size_t)kMaxBarcode || le > (size_t)kMaxBarcode) return LVA_ERR_ARG;
  std::memset(p, 0, sizeof *p);
  p->len[0] = (uint8_t)ls; p->len[1] = (uint8_t)le;
  std::memcpy(p->pat[0], start_bc, ls);
  std::memcpy(p->pat[1], end_bc, le);
  if (n_orient == 2) {         // generate_decoded_lists.py:33-34: START_BARCODE_RC = rc(END), END_BARCODE_RC = rc(START)
    p->len[2] = (uint8_t)le; p->len[3] = (uint8_t)ls;
    if (!rc_pattern(end_bc, (int)le, p->pat[2]) || !rc_pattern(start_bc, (int)ls, p->pat[3])) return LVA_ERR_ARG;
  }
  return LVA_OK;
}

// Basecalls of n reads (T blocks or bases in all) on the device, as the searches read them: made there by bc_basecall
// (basecall_set: its working set) or the caller's own, uploaded (given_set).  Declaration order = order in the block.
struct Calls {
  Arena::Piece<int64_t> off;
  Arena::Piece<uint32_t> tb;     // 8 back-pointer bytes per block
  Arena::Piece<uint8_t> path;
  Arena::Piece<char> bases;
  Arena::Piece<uint32_t> trans;
  Arena::Piece<int32_t> nb;
};
Calls basecall_set(Arena& a, size_t n, size_t T) {
  return {a.add<int64_t>(n + 1), a.add<uint32_t>(2 * T), a.add<uint8_t>(T + n), a.add<char>(T), a.add<uint32_t>(T), a.add<int32_t>(n)};
}

Calls given_set(Arena& a, size_t n, size_t T) {
  return {a.add<int64_t>(n + 1), {}, {}, a.add<char>(T), a.add<uint32_t>(T), a.add<int32_t>(n)};
}

// offsets up, bc_basecall over posteriors that are on the device
int enqueue_basecall(lva_decoder* d, const Arena& a, const Calls& c, const float* post_dev, const int64_t* row_offsets, int32_t n) {
  HIP_TRY(hipMemcpyAsync(a.ptr(c.off), row_offsets, 8 * ((size_t)n + 1), hipMemcpyHostToDevice, d->stream));
  return launch_status(launch_bc_basecall(post_dev, a.ptr(c.off), n, a.ptr(c.tb), a.ptr(c.path), a.ptr(c.bases), a.ptr(c.trans),
                                          a.ptr(c.nb), d->stream));
}

// the caller's basecalls up; nb (read_lengths) outlives the call's StreamDrain
int enqueue_given(lva_decoder* d, const Arena& a, const Calls& c, const char* bases, const uint32_t* trans,
                  const int64_t* base_offsets, const std::vector<int32_t>& nb, size_t T) {
  const size_t n = nb.size();
  HIP_TRY(hipMemcpyAsync(a.ptr(c.off), base_offsets, 8 * (n + 1), hipMemcpyHostToDevice, d->stream));
  if (T) HIP_TRY(hipMemcpyAsync(a.ptr(c.bases), bases, T, hipMemcpyHostToDevice, d->stream));
  if (T) HIP_TRY(hipMemcpyAsync(a.ptr(c.trans), trans, 4 * T, hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(a.ptr(c.nb), nb.data(), 4 * n, hipMemcpyHostToDevice, d->stream));
  return LVA_OK;
}

struct LocateSet { Arena::Piece<uint32_t> best; Arena::Piece<BcResult> res; };
LocateSet locate_set(Arena& a, size_t n) { return {a.add<uint32_t>(4 * n), a.add<BcResult>(n)}; }

// bc_search + bc_finalize over basecalls that are on the device, and the copy of the windows to the caller
int enqueue_locate(lva_decoder* d, const Arena& a, const Calls& c, const LocateSet& s, int32_t n, const BcPatterns& pat,
                   int n_orient, uint32_t min_len, lva_payload_pos* out) {
  static_assert(sizeof(lva_payload_pos) == sizeof(BcResult), "lva_payload_pos layout");
  int e = launch_bc_search(a.ptr(c.bases), a.ptr(c.off), a.ptr(c.nb), n, pat, n_orient, a.ptr(s.best), d->stream);
  if (!e) e = launch_bc_finalize(a.ptr(c.trans), a.ptr(c.off), a.ptr(c.nb), n, pat, n_orient, min_len, a.ptr(s.best), a.ptr(s.res),
                                 d->stream);
  if (e) return launch_status(e);
  HIP_TRY(hipMemcpyAsync(out, a.ptr(s.res), sizeof(BcResult) * (size_t)n, hipMemcpyDeviceToHost, d->stream));
  return LVA_OK;
}

// lva_basecall_batch[_device] (n_orient = 0: no barcodes, pos_out null) and lva_locate_payload_batch[_device]
// (n_orient = 2); post is the caller's host buffer or the caller's device buffer
int basecall_stage(lva_decoder* d, const float* post, bool post_on_host, const int64_t* row_offsets, int32_t n,
                   const char* start_bc, const char* end_bc, int n_orient, uint32_t min_len, char* bases_out,
                   uint32_t* trans_out, int32_t* nbases_out, lva_payload_pos* pos_out) {
  if (!d || n < 0 || !row_offsets || (n > 0 && (!post || (n_orient ? !pos_out : !nbases_out)))) return LVA_ERR_ARG;
  BcPatterns pat;
  if (n_orient && make_patterns(start_bc, end_bc, n_orient, &pat) != LVA_OK) return LVA_ERR_ARG;
  size_t T = 0;
  int st = stage_enter(d, row_offsets, n, &T);
  if (st != kRun) return st;
  Arena arena;
  HostPost hp;
  const Calls bc = basecall_set(arena, (size_t)n, T);
  const LocateSet loc = locate_set(arena, (size_t)n);
  if (arena.alloc() != LVA_OK) return LVA_ERR_NOMEM;
  StreamDrain drain(d->stream);
  if (post_on_host && (st = upload_post(d, post, T, &hp)) != LVA_OK) return st;
  if ((st = enqueue_basecall(d, arena, bc, post_on_host ? hp.dev : post, row_offsets, n)) != LVA_OK) return st;
  if (n_orient && (st = enqueue_locate(d, arena, bc, loc, n, pat, n_orient, min_len, pos_out)) != LVA_OK) return st;
  if (bases_out && T) HIP_TRY(hipMemcpyAsync(bases_out, arena.ptr(bc.bases), T, hipMemcpyDeviceToHost, d->stream));
  if (trans_out && T) HIP_TRY(hipMemcpyAsync(trans_out, arena.ptr(bc.trans), 4 * T, hipMemcpyDeviceToHost, d->stream));
  if (nbases_out) HIP_TRY(hipMemcpyAsync(nbases_out, arena.ptr(bc.nb), 4 * (size_t)n, hipMemcpyDeviceToHost, d->stream));
  return drain.finish();
}

}  // namespace

extern "C" {

int lva_basecall_batch_device(lva_decoder* d, const float* post_dev, const int64_t* row_offsets, int32_t n_reads, char* bases_out,
                              uint32_t* trans_out, int32_t* nbases_out) {
  return basecall_stage(d, post_dev, false, row_offsets, n_reads, nullptr, nullptr, 0, 0, bases_out, trans_out, nbases_out, nullptr);
}

int lva_basecall_batch(lva_decoder* d, const float* post, const int64_t* row_offsets, int32_t n_reads, char* bases_out,
                       uint32_t* trans_out, int32_t* nbases_out) {
  return basecall_stage(d, post, true, row_offsets, n_reads, nullptr, nullptr, 0, 0, bases_out, trans_out, nbases_out, nullptr);
}

int lva_locate_payload_batch_device(lva_decoder* d, const float* post_dev, const int64_t* row_offsets, int32_t n_reads,
                                    const char* start_barcode, const char* end_barcode, uint32_t min_len, lva_payload_pos* out) {
  return basecall_stage(d, post_dev, false, row_offsets, n_reads, start_barcode, end_barcode, 2, min_len, nullptr, nullptr, nullptr, out);
}

int lva_locate_payload_batch(lva_decoder* d, const float* post, const int64_t* row_offsets, int32_t n_reads,
                             const char* start_barcode, const char* end_barcode, uint32_t min_len, lva_payload_pos* out) {
  return basecall_stage(d, post, true, row_offsets, n_reads, start_barcode, end_barcode, 2, min_len, nullptr, nullptr, nullptr, out);
}

int lva_find_barcode_batch(lva_decoder* d, const char* bases, const uint32_t* trans, const int64_t* base_offsets,
                           int32_t n_reads, const char* start_barcode, const char* end_barcode, lva_payload_pos* out) {
  if (!d || n_reads < 0 || !base_offsets || (n_reads > 0 && (!bases || !trans || !out))) return LVA_ERR_ARG;
  BcPatterns pat;
  if (make_patterns(start_barcode, end_barcode, 1, &pat) != LVA_OK) return LVA_ERR_ARG;
  size_t T = 0;
  int st = stage_enter(d, base_offsets, n_reads, &T);
  if (st != kRun) return st;
  const std::vector<int32_t> nb = read_lengths(base_offsets, n_reads);
  Arena arena;
  const Calls calls = given_set(arena, nb.size(), T);
  const LocateSet loc = locate_set(arena, nb.size());
  if (arena.alloc() != LVA_OK) return LVA_ERR_NOMEM;
  StreamDrain drain(d->stream);
  if ((st = enqueue_given(d, arena, calls, bases, trans, base_offsets, nb, T)) != LVA_OK) return st;
  if ((st = enqueue_locate(d, arena, calls, loc, n_reads, pat, 1, 0, out)) != LVA_OK) return st;
  return drain.finish();
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// transition posteriors from a network's transition scores.
// ---------------------------------------------------------------------------------------------
namespace {

// forward and backward kernel over n reads resident on the device; post_dev may be scores_dev.  Enqueues only.
int tp_run(lva_decoder* d, const float* scores_dev, const int64_t* row_offsets, int32_t n, size_t T, float* post_dev) {
  if (T > d->tp_fwd_cap) {
    HIP_TRY(hipStreamSynchronize(d->stream));
    if (d->d_tp_fwd) (void)hipFree(d->d_tp_fwd);
    d->d_tp_fwd = nullptr; d->tp_fwd_cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(&d->d_tp_fwd), T * 8 * sizeof(float)) != hipSuccess) return LVA_ERR_NOMEM;
    d->tp_fwd_cap = T;
  }
  if ((size_t)n + 1 > d->tp_off_cap) {
    HIP_TRY(hipStreamSynchronize(d->stream));
    if (d->d_tp_off) (void)hipFree(d->d_tp_off);
    d->d_tp_off = nullptr; d->tp_off_cap = 0;
    const size_t cap = std::max<size_t>((size_t)n + 1, 1024);
    if (hipMalloc(reinterpret_cast<void**>(&d->d_tp_off), cap * sizeof(int64_t)) != hipSuccess) return LVA_ERR_NOMEM;
    d->tp_off_cap = cap;
  }
  HIP_TRY(hipMemcpyAsync(d->d_tp_off, row_offsets, 8 * ((size_t)n + 1), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipEventRecord(d->ev_total0, d->stream));
  int e = launch_tp_forward(scores_dev, d->d_tp_off, n, d->d_tp_fwd, d->stream);
  if (!e) e = launch_tp_backward(scores_dev, d->d_tp_off, n, d->d_tp_fwd, post_dev, d->stream);
  if (e) return launch_status(e);
  HIP_TRY(hipEventRecord(d->ev_total1, d->stream));
  return LVA_OK;
}

// the profile after a posterior call: the two kernels' HIP-event time and the blocks they covered
int tp_profile(lva_decoder* d, size_t T, bool timed) {
  const int32_t slots = d->prof.slots, kernel = d->prof.kernel;
  d->prof = lva_profile{};
  d->prof.slots = slots; d->prof.kernel = kernel;
  d->prof.read_steps = T;
  float ms = 0;
  if (timed) HIP_TRY(hipEventElapsedTime(&ms, d->ev_total0, d->ev_total1));
  d->prof.total_ms = ms;
  return LVA_OK;
}

// lva_transpost_batch (scores and post on the host: the kernels run in place on the device copy) and
// lva_transpost_batch_device (both the caller's device buffers, which may be one).  A call with no block resets the profile.
int transpost_stage(lva_decoder* d, const float* scores, bool on_host, const int64_t* row_offsets, int32_t n, float* post) {
  if (!d || n < 0 || !row_offsets) return LVA_ERR_ARG;
  size_t T = 0;
  if (check_offsets(row_offsets, n, &T) != LVA_OK) return LVA_ERR_ARG;
  // (device buffers: 16-byte row requests)
  if (T > 0 && (!scores || !post || (!on_host && (((uintptr_t)scores | (uintptr_t)post) & 15u)))) return LVA_ERR_ARG;
  int st = stage_enter(d, T == 0);
  if (st == LVA_OK) return tp_profile(d, 0, false);
  if (st != kRun) return st;
  HostPost hp;
  StreamDrain drain(d->stream);              // the offsets are copied from the caller's memory
  if (on_host && (st = upload_post(d, scores, T, &hp)) != LVA_OK) return st;
  st = on_host ? tp_run(d, hp.dev, row_offsets, n, T, hp.dev) : tp_run(d, scores, row_offsets, n, T, post);
  if (st != LVA_OK) return st;
  if (on_host) HIP_TRY(hipMemcpyAsync(post, hp.dev, T * 160, hipMemcpyDeviceToHost, d->stream));
  if ((st = drain.finish()) != LVA_OK) return st;
  return tp_profile(d, T, true);
}

}  // namespace

extern "C" {

int lva_transpost_batch_device(lva_decoder* d, const float* scores_dev, const int64_t* row_offsets, int32_t n_reads, float* post_dev) {
  return transpost_stage(d, scores_dev, false, row_offsets, n_reads, post_dev);
}

int lva_transpost_batch(lva_decoder* d, const float* scores, const int64_t* row_offsets, int32_t n_reads, float* post_out) {
  return transpost_stage(d, scores, true, row_offsets, n_reads, post_out);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// DESIGN.md section 1 row N3': demultiplexing a pooled run (bc_search_multi, bc_demux_finalize).
// ---------------------------------------------------------------------------------------------
namespace {

struct DemuxArgs {
  std::vector<BcPatterns> pats;
  std::vector<uint32_t> min_len;
  int32_t max_dist, min_margin;
};

// everything that can be refused without the device
int demux_args(const lva_experiment_barcodes* exps, int32_t n_exps, int32_t max_dist, int32_t min_margin, DemuxArgs* a) {
  if (!exps || n_exps < 1 || n_exps > kMaxExperiments || min_margin < 0) return LVA_ERR_ARG;
  a->pats.resize(n_exps);
  a->min_len.resize(n_exps);
  for (int32_t e = 0; e < n_exps; ++e) {
    // both reverse complements are formed: a character outside ACGTN in either barcode is refused here
    if (make_patterns(exps[e].start_barcode, exps[e].end_barcode, 2, &a->pats[e]) != LVA_OK) return LVA_ERR_ARG;
    a->min_len[e] = exps[e].min_len;
  }
  a->max_dist = max_dist < 0 ? -1 : max_dist;
  a->min_margin = min_margin;
  return LVA_OK;
}

struct DemuxSet {
  Arena::Piece<BcPatterns> pats;
  Arena::Piece<uint32_t> min_len;
  Arena::Piece<uint32_t> best;
  Arena::Piece<BcDemuxResult> res;
  Arena::Piece<BcResult> all;    // only when the caller asks for every experiment's candidate
};
DemuxSet demux_set(Arena& a, size_t n, size_t k, bool all) {
  return {a.add<BcPatterns>(k), a.add<uint32_t>(k), a.add<uint32_t>(4 * n * k), a.add<BcDemuxResult>(n),
          all ? a.add<BcResult>(n * k) : Arena::Piece<BcResult>{}};
}

// search + choice over basecalls that are on the device, and the copies of the results to the caller; x (demux_args)
// outlives the call's StreamDrain
int enqueue_demux(lva_decoder* d, const Arena& a, const Calls& c, const DemuxSet& s, int32_t n_reads, const DemuxArgs& x,
                  lva_demux_pos* out, lva_payload_pos* all_out) {
  static_assert(sizeof(lva_demux_pos) == sizeof(BcDemuxResult), "lva_demux_pos layout");
  const size_t n = (size_t)n_reads, k = x.pats.size();
  HIP_TRY(hipMemcpyAsync(a.ptr(s.pats), x.pats.data(), sizeof(BcPatterns) * k, hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(a.ptr(s.min_len), x.min_len.data(), 4 * k, hipMemcpyHostToDevice, d->stream));
  int e = launch_bc_search_multi(a.ptr(c.bases), a.ptr(c.off), a.ptr(c.nb), n_reads, a.ptr(s.pats), (int32_t)k, a.ptr(s.best), d->stream);
  if (!e) e = launch_bc_demux_finalize(a.ptr(c.trans), a.ptr(c.off), a.ptr(c.nb), n_reads, a.ptr(s.pats), a.ptr(s.min_len), (int32_t)k,
                                       x.max_dist, x.min_margin, a.ptr(s.best), a.ptr(s.res), a.ptr(s.all), d->stream);
  if (e) return launch_status(e);
  HIP_TRY(hipMemcpyAsync(out, a.ptr(s.res), sizeof(BcDemuxResult) * n, hipMemcpyDeviceToHost, d->stream));
  if (all_out) HIP_TRY(hipMemcpyAsync(all_out, a.ptr(s.all), sizeof(BcResult) * n * k, hipMemcpyDeviceToHost, d->stream));
  return LVA_OK;
}

// lva_demux_batch (post on the host) and lva_demux_batch_device: basecall, then search + choice
int demux_stage(lva_decoder* d, const float* post, bool post_on_host, const int64_t* row_offsets, int32_t n,
                const lva_experiment_barcodes* exps, int32_t n_exps, int32_t max_dist, int32_t min_margin, lva_demux_pos* out,
                lva_payload_pos* all_out) {
  if (!d || n < 0 || !row_offsets || (n > 0 && (!post || !out))) return LVA_ERR_ARG;
  DemuxArgs x;
  if (demux_args(exps, n_exps, max_dist, min_margin, &x) != LVA_OK) return LVA_ERR_ARG;
  size_t T = 0;
  int st = stage_enter(d, row_offsets, n, &T);
  if (st != kRun) return st;
  Arena arena;
  HostPost hp;
  const Calls bc = basecall_set(arena, (size_t)n, T);
  const DemuxSet dm = demux_set(arena, (size_t)n, x.pats.size(), all_out != nullptr);
  if (arena.alloc() != LVA_OK) return LVA_ERR_NOMEM;
  StreamDrain drain(d->stream);
  if (post_on_host && (st = upload_post(d, post, T, &hp)) != LVA_OK) return st;
  if ((st = enqueue_basecall(d, arena, bc, post_on_host ? hp.dev : post, row_offsets, n)) != LVA_OK) return st;
  if ((st = enqueue_demux(d, arena, bc, dm, n, x, out, all_out)) != LVA_OK) return st;
  return drain.finish();
}

}  // namespace

extern "C" {

int lva_demux_batch_device(lva_decoder* d, const float* post_dev, const int64_t* row_offsets, int32_t n_reads,
                           const lva_experiment_barcodes* exps, int32_t n_exps, int32_t max_dist, int32_t min_margin,
                           lva_demux_pos* out, lva_payload_pos* all_out) {
  return demux_stage(d, post_dev, false, row_offsets, n_reads, exps, n_exps, max_dist, min_margin, out, all_out);
}

int lva_demux_batch(lva_decoder* d, const float* post, const int64_t* row_offsets, int32_t n_reads,
                    const lva_experiment_barcodes* exps, int32_t n_exps, int32_t max_dist, int32_t min_margin,
                    lva_demux_pos* out, lva_payload_pos* all_out) {
  return demux_stage(d, post, true, row_offsets, n_reads, exps, n_exps, max_dist, min_margin, out, all_out);
}

int lva_demux_bases_batch(lva_decoder* d, const char* bases, const uint32_t* trans, const int64_t* base_offsets,
                          int32_t n_reads, const lva_experiment_barcodes* exps, int32_t n_exps, int32_t max_dist,
                          int32_t min_margin, lva_demux_pos* out, lva_payload_pos* all_out) {
  if (!d || n_reads < 0 || !base_offsets || (n_reads > 0 && (!bases || !trans || !out))) return LVA_ERR_ARG;
  DemuxArgs x;
  if (demux_args(exps, n_exps, max_dist, min_margin, &x) != LVA_OK) return LVA_ERR_ARG;
  size_t T = 0;
  int st = stage_enter(d, base_offsets, n_reads, &T);
  if (st != kRun) return st;
  const std::vector<int32_t> nb = read_lengths(base_offsets, n_reads);
  Arena arena;
  const Calls calls = given_set(arena, nb.size(), T);
  const DemuxSet dm = demux_set(arena, nb.size(), x.pats.size(), all_out != nullptr);
  if (arena.alloc() != LVA_OK) return LVA_ERR_NOMEM;
  StreamDrain drain(d->stream);
  if ((st = enqueue_given(d, arena, calls, bases, trans, base_offsets, nb, T)) != LVA_OK) return st;
  if ((st = enqueue_demux(d, arena, calls, dm, n_reads, x, out, all_out)) != LVA_OK) return st;
  return drain.finish();
}

}  // extern "C"

/* ---------------------------------------------------------------------------------------------
 * the consumers of a decoded list (csrc/ls_kernels.hip).  Like the RS entry
 * points they take a device ordinal, work on a stream of their own and leave every decoder's profile alone.
 * Arguments first, then the device ordinal.
 * ------------------------------------------------------------------------------------------- */
namespace {

struct LsStream {               // a stream for the length of one call
  hipStream_t s = nullptr;
  ~LsStream() { if (s) (void)hipStreamDestroy(s); }
};

int ls_open(int32_t device, LsStream* st) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return LVA_ERR_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return LVA_ERR_NO_DEVICE;
  HIP_TRY(hipStreamCreateWithFlags(&st->s, hipStreamNonBlocking));
  return LVA_OK;
}

// msgs / counts of n reads: the shape every list consumer accepts
bool ls_shape_ok(int32_t n_reads, int32_t list_size, uint32_t msg_len) {
  if (n_reads < 0 || list_size < 1 || msg_len < 1 || msg_len > (uint32_t)kLsMaxMsgLen) return false;
  return (uint64_t)n_reads * (uint64_t)list_size * (uint64_t)msg_len < (1ull << 31);
}

}  // namespace

extern "C" {

int lva_list_filter(int32_t device, const uint8_t* msgs, const int32_t* counts, int32_t n_reads, int32_t list_size,
                    uint32_t msg_len, int32_t use_entries, int32_t bytes_per_oligo, int32_t num_oligos, int32_t pad,
                    int32_t* out_index, int32_t* out_rank, uint8_t* out_payload) {
  if (!msgs || !counts || !out_index || !out_rank || !out_payload) return LVA_ERR_ARG;
  if (!ls_shape_ok(n_reads, list_size, msg_len) || use_entries < 0 || use_entries > list_size) return LVA_ERR_ARG;
  if (bytes_per_oligo < 1 || num_oligos < 1 || num_oligos > 4096) return LVA_ERR_ARG;
  if ((uint64_t)msg_len != 12ull + 8ull + 8ull * (uint64_t)bytes_per_oligo + (pad ? 1ull : 0ull)) return LVA_ERR_ARG;
  if (n_reads == 0) return LVA_OK;
  const int32_t use = use_entries ? use_entries : list_size;
  LsStream st;
  if (const int so = ls_open(device, &st)) return so;
  const size_t n = (size_t)n_reads, mb = n * (size_t)list_size * msg_len, pb = n * (size_t)bytes_per_oligo;
  Arena arena;
  const auto d_msgs = arena.add<uint8_t>(mb);            // 256-byte aligned and padded: whole dwords may be read
  const auto d_counts = arena.add<int32_t>(n), d_index = arena.add<int32_t>(n), d_rank = arena.add<int32_t>(n);
  const auto d_pay = arena.add<uint8_t>(pb);
  if (arena.alloc() != LVA_OK) return LVA_ERR_NOMEM;
  StreamDrain drain(st.s);
  HIP_TRY(hipMemcpyAsync(arena.ptr(d_msgs), msgs, mb, hipMemcpyHostToDevice, st.s));
  HIP_TRY(hipMemcpyAsync(arena.ptr(d_counts), counts, 4 * n, hipMemcpyHostToDevice, st.s));
  const int e = launch_ls_filter(arena.ptr(d_msgs), arena.ptr(d_counts), n_reads, list_size, msg_len, use, bytes_per_oligo, num_oligos,
                                 pad, arena.ptr(d_index), arena.ptr(d_rank), arena.ptr(d_pay), st.s);
  if (e) return launch_status(e);
  HIP_TRY(hipMemcpyAsync(out_index, arena.ptr(d_index), 4 * n, hipMemcpyDeviceToHost, st.s));
  HIP_TRY(hipMemcpyAsync(out_rank, arena.ptr(d_rank), 4 * n, hipMemcpyDeviceToHost, st.s));
  HIP_TRY(hipMemcpyAsync(out_payload, arena.ptr(d_pay), pb, hipMemcpyDeviceToHost, st.s));
  return drain.finish();
}

int lva_list_consensus(int32_t device, const int32_t* index, const uint8_t* payload, int32_t n_reads, int32_t bytes_per_oligo,
                       int32_t num_oligos, int32_t first_only, uint8_t* out_present, uint8_t* out_payload, int32_t* out_votes) {
  if (!index || !payload || !out_present || !out_payload || !out_votes) return LVA_ERR_ARG;
  if (n_reads < 0 || bytes_per_oligo < 1 || num_oligos < 1 || num_oligos > 4096) return LVA_ERR_ARG;
  if ((uint64_t)n_reads * (uint64_t)bytes_per_oligo >= (1ull << 31)) return LVA_ERR_ARG;
  for (int32_t i = 0; i < n_reads; ++i)
    if (index[i] >= num_oligos) return LVA_ERR_ARG;      // (negative: the read passed no entry and has no vote)
  if (n_reads == 0) return LVA_OK;
  LsStream st;
  if (const int so = ls_open(device, &st)) return so;
  const size_t n = (size_t)n_reads, no = (size_t)num_oligos, pb = n * (size_t)bytes_per_oligo, ob = no * (size_t)bytes_per_oligo;
  Arena arena;
  const auto d_index = arena.add<int32_t>(n), d_order = arena.add<int32_t>(n);
  const auto d_pay = arena.add<uint8_t>(pb);
  const auto d_bucket = arena.add<int32_t>(no + 1);
  const auto d_present = arena.add<uint8_t>(no), d_out = arena.add<uint8_t>(ob);
  const auto d_votes = arena.add<int32_t>(no);
  if (arena.alloc() != LVA_OK) return LVA_ERR_NOMEM;
  StreamDrain drain(st.s);
  HIP_TRY(hipMemcpyAsync(arena.ptr(d_index), index, 4 * n, hipMemcpyHostToDevice, st.s));
  HIP_TRY(hipMemcpyAsync(arena.ptr(d_pay), payload, pb, hipMemcpyHostToDevice, st.s));
  const int e = launch_ls_consensus(arena.ptr(d_index), arena.ptr(d_pay), n_reads, bytes_per_oligo, num_oligos, first_only ? 1 : 0,
                                    arena.ptr(d_bucket), arena.ptr(d_order), arena.ptr(d_present), arena.ptr(d_out),
                                    arena.ptr(d_votes), st.s);
  if (e) return launch_status(e);
  HIP_TRY(hipMemcpyAsync(out_present, arena.ptr(d_present), no, hipMemcpyDeviceToHost, st.s));
  HIP_TRY(hipMemcpyAsync(out_payload, arena.ptr(d_out), ob, hipMemcpyDeviceToHost, st.s));
  HIP_TRY(hipMemcpyAsync(out_votes, arena.ptr(d_votes), 4 * no, hipMemcpyDeviceToHost, st.s));
  return drain.finish();
}

int lva_list_stats(int32_t device, const uint8_t* msgs, const int32_t* counts, const uint8_t* truth, int32_t n_reads,
                   int32_t list_size, uint32_t msg_len, lva_list_stat* out) {
  static_assert(sizeof(lva_list_stat) == kLsStatFields * sizeof(int32_t), "ls_stats writes the fields of lva_list_stat in order");
  if (!msgs || !counts || !truth || !out) return LVA_ERR_ARG;
  if (!ls_shape_ok(n_reads, list_size, msg_len)) return LVA_ERR_ARG;
  if (n_reads == 0) return LVA_OK;
  LsStream st;
  if (const int so = ls_open(device, &st)) return so;
  const size_t n = (size_t)n_reads, mb = n * (size_t)list_size * msg_len, tb = n * msg_len;
  Arena arena;
  const auto d_msgs = arena.add<uint8_t>(mb);
  const auto d_counts = arena.add<int32_t>(n);
  const auto d_truth = arena.add<uint8_t>(tb);
  const auto d_packed = arena.add<uint64_t>(kLsPackWords * n);
  const auto d_out = arena.add<int32_t>(kLsStatFields * n);
  if (arena.alloc() != LVA_OK) return LVA_ERR_NOMEM;
  StreamDrain drain(st.s);
  HIP_TRY(hipMemcpyAsync(arena.ptr(d_msgs), msgs, mb, hipMemcpyHostToDevice, st.s));
  HIP_TRY(hipMemcpyAsync(arena.ptr(d_counts), counts, 4 * n, hipMemcpyHostToDevice, st.s));
  HIP_TRY(hipMemcpyAsync(arena.ptr(d_truth), truth, tb, hipMemcpyHostToDevice, st.s));
  const int e = launch_ls_stats(arena.ptr(d_msgs), arena.ptr(d_counts), arena.ptr(d_truth), n_reads, list_size, msg_len,
                                arena.ptr(d_packed), arena.ptr(d_out), st.s);
  if (e) return launch_status(e);
  HIP_TRY(hipMemcpyAsync(out, arena.ptr(d_out), 4 * kLsStatFields * n, hipMemcpyDeviceToHost, st.s));
  return drain.finish();
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// DESIGN.md section 1 row N4': reading-cost trials (csrc/tr_kernels.hip; the definition is trials.py).  Like the list
// consumers: a device ordinal, a stream of its own, complete on return.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr size_t kTrChunkBytes = (size_t)1 << 30;        // what a chunk of trials may occupy on the device

// everything lva_rs_trials can refuse without the device
int trials_args(const int32_t* index, const uint8_t* payload, int32_t n_reads, int32_t bpo, int32_t num_oligos, int32_t redundancy,
                const uint8_t* original, int64_t original_bytes, const int32_t* reads_to_use, int32_t n_points,
                uint32_t first_trial, int32_t n_trials, int32_t chunk_trials, const int32_t* out_stats) {
  if (n_reads < 0 || n_trials < 0 || chunk_trials < 0) return LVA_ERR_ARG;
  if (bpo < 2 || (bpo & 1) || num_oligos < 1 || num_oligos > 4096) return LVA_ERR_ARG;
  if (redundancy < 1 || redundancy > std::min(4096, num_oligos - 1)) return LVA_ERR_ARG;
  if (n_points < 1 || n_points > kTrMaxPoints || !reads_to_use) return LVA_ERR_ARG;
  if (!original || original_bytes < 1 || original_bytes > (int64_t)(num_oligos - redundancy) * bpo) return LVA_ERR_ARG;
  if ((uint64_t)first_trial + (uint64_t)n_trials > ((uint64_t)1 << 32)) return LVA_ERR_ARG;      // trial numbers are 32-bit
  if ((n_reads > 0 && (!index || !payload)) || (n_trials > 0 && !out_stats)) return LVA_ERR_ARG;
  if ((uint64_t)n_reads * (uint64_t)bpo >= (1ull << 31)) return LVA_ERR_ARG;
  for (int32_t k = 0; k < n_points; ++k)
    if (reads_to_use[k] < 0 || reads_to_use[k] > n_reads || (k > 0 && reads_to_use[k] < reads_to_use[k - 1])) return LVA_ERR_ARG;
  for (int32_t i = 0; i < n_reads; ++i)
    if (index[i] >= num_oligos) return LVA_ERR_ARG;      // (negative: the read passed no entry and has no vote)
  return LVA_OK;
}

}  // namespace

extern "C" {

int lva_rs_trials(int32_t device, const int32_t* index, const uint8_t* payload, int32_t n_reads, int32_t bytes_per_oligo,
                  int32_t num_oligos, int32_t redundancy, const uint8_t* original, int64_t original_bytes,
                  const int32_t* reads_to_use, int32_t n_points, uint64_t seed, uint32_t first_trial, int32_t n_trials,
                  int32_t chunk_trials, int32_t* out_stats, uint8_t* out_present, uint8_t* out_payload) {
  if (trials_args(index, payload, n_reads, bytes_per_oligo, num_oligos, redundancy, original, original_bytes, reads_to_use, n_points,
                  first_trial, n_trials, chunk_trials, out_stats) != LVA_OK)
    return LVA_ERR_ARG;
  if (n_trials == 0 || n_reads == 0) return LVA_OK;
  const size_t n = (size_t)n_reads, no = (size_t)num_oligos, bpo = (size_t)bytes_per_oligo, s = bpo / 2, K = (size_t)n_points;
  const size_t nd = no - (size_t)redundancy, T = (size_t)n_trials;
  // bytes of one trial in a chunk: RS input and output, members and erasures per index, the places and counts of the reads
  const size_t per_trial = K * (2 * s * no + 2 * s * nd + 8 * no + 8 * s + 12 + (out_payload ? no * bpo : 0) + (out_present ? no : 0)) + 8 * n;
  size_t chunk = std::min(T, std::max<size_t>(kTrChunkBytes / per_trial, 1));
  if (chunk_trials > 0) chunk = std::min(chunk, (size_t)chunk_trials);
  TrShape sh{};
  sh.n_reads = n_reads; sh.bpo = bytes_per_oligo; sh.num_oligos = num_oligos; sh.fec = redundancy; sh.n_points = n_points;
  sh.k0 = (uint32_t)seed; sh.k1 = (uint32_t)(seed >> 32);
  std::copy(reads_to_use, reads_to_use + n_points, sh.points);
  std::vector<uint16_t> gexp, glog, truth(s * nd, 0);    // (these outlive the call's StreamDrain)
  tr_gf_tables(&gexp, &glog);
  for (size_t c = 0; c < s; ++c)                         // column c of the original file, as the decoder's output is laid out
    for (size_t j = 0; j < nd; ++j) {
      const int64_t at = (int64_t)(j * bpo + 2 * c);
      const uint32_t lo = at < original_bytes ? original[at] : 0u, hi = at + 1 < original_bytes ? original[at + 1] : 0u;
      truth[c * nd + j] = (uint16_t)(lo | (hi << 8));
    }
  LsStream st;
  if (const int so = ls_open(device, &st)) return so;
  Arena arena;
  const auto d_index = arena.add<int32_t>(n), d_order = arena.add<int32_t>(n);
  const auto d_pay = arena.add<uint8_t>(n * bpo);
  const auto d_bucket = arena.add<int32_t>(no + 1);
  const auto d_gexp = arena.add<uint16_t>(kTrGexpWords), d_glog = arena.add<uint16_t>(kTrGlogWords), d_truth = arena.add<uint16_t>(s * nd);
  const auto d_stats = arena.add<int32_t>(4 * K * T);
  const auto d_place = arena.add<int32_t>(chunk * n), d_cnt = arena.add<int32_t>(chunk * n);
  const auto d_nmem = arena.add<int32_t>(K * chunk * no), d_erl = arena.add<int32_t>(K * chunk * no);
  const auto d_ern = arena.add<int32_t>(K * chunk), d_pp = arena.add<int32_t>(2 * K * chunk), d_okeq = arena.add<int32_t>(2 * K * chunk * s);
  const auto d_sym = arena.add<uint16_t>(K * chunk * s * no), d_dec = arena.add<uint16_t>(K * chunk * s * nd);
  const auto d_cons = out_payload ? arena.add<uint8_t>(K * chunk * no * bpo) : Arena::Piece<uint8_t>{};
  const auto d_pres = out_present ? arena.add<uint8_t>(K * chunk * no) : Arena::Piece<uint8_t>{};
  if (arena.alloc() != LVA_OK) return LVA_ERR_NOMEM;
  StreamDrain drain(st.s);
  HIP_TRY(hipMemcpyAsync(arena.ptr(d_index), index, 4 * n, hipMemcpyHostToDevice, st.s));
  HIP_TRY(hipMemcpyAsync(arena.ptr(d_pay), payload, n * bpo, hipMemcpyHostToDevice, st.s));
  HIP_TRY(hipMemcpyAsync(arena.ptr(d_gexp), gexp.data(), 2 * kTrGexpWords, hipMemcpyHostToDevice, st.s));
  HIP_TRY(hipMemcpyAsync(arena.ptr(d_glog), glog.data(), 2 * kTrGlogWords, hipMemcpyHostToDevice, st.s));
  HIP_TRY(hipMemcpyAsync(arena.ptr(d_truth), truth.data(), 2 * s * nd, hipMemcpyHostToDevice, st.s));
  int e = launch_ls_bucket_scan(arena.ptr(d_index), n_reads, num_oligos, arena.ptr(d_bucket), st.s);
  if (!e) e = launch_tr_bucket_list(arena.ptr(d_index), n_reads, num_oligos, arena.ptr(d_bucket), arena.ptr(d_order), st.s);
  if (e) return launch_status(e);
  for (size_t at = 0; at < T; at += chunk) {             // a trial depends on (seed, trial number) alone: chunks change nothing
    const size_t c = std::min(chunk, T - at);
    sh.chunk = (int32_t)c;
    sh.first_trial = first_trial + (uint32_t)at;
    e = launch_tr_consensus(sh, arena.ptr(d_bucket), arena.ptr(d_order), arena.ptr(d_pay), arena.ptr(d_place), arena.ptr(d_cnt),
                            arena.ptr(d_nmem), arena.ptr(d_sym), arena.ptr(d_cons), st.s);
    if (!e) e = launch_tr_erasures(sh, arena.ptr(d_nmem), arena.ptr(d_erl), arena.ptr(d_ern), arena.ptr(d_pp), arena.ptr(d_pres), st.s);
    if (!e) e = launch_tr_decode(sh, arena.ptr(d_sym), arena.ptr(d_erl), arena.ptr(d_ern), arena.ptr(d_gexp), arena.ptr(d_glog),
                                 arena.ptr(d_dec), arena.ptr(d_truth), original_bytes, arena.ptr(d_okeq), st.s);
    if (!e) e = launch_tr_fold(sh, arena.ptr(d_okeq), arena.ptr(d_pp), arena.ptr(d_stats), n_trials, (int32_t)at, st.s);
    if (e) return launch_status(e);
    for (size_t k = 0; k < K; ++k) {                     // the chunk holds [point][trial of the chunk], the caller [point][trial]
      if (out_present)
        HIP_TRY(hipMemcpyAsync(out_present + (k * T + at) * no, arena.ptr(d_pres) + k * c * no, c * no, hipMemcpyDeviceToHost, st.s));
      if (out_payload)
        HIP_TRY(hipMemcpyAsync(out_payload + (k * T + at) * no * bpo, arena.ptr(d_cons) + k * c * no * bpo, c * no * bpo,
                               hipMemcpyDeviceToHost, st.s));
    }
  }
  HIP_TRY(hipMemcpyAsync(out_stats, arena.ptr(d_stats), 16 * K * T, hipMemcpyDeviceToHost, st.s));
  return drain.finish();
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// the read simulator (csrc/sim_kernels.hip; the definition is simulate.py).
// ---------------------------------------------------------------------------------------------
namespace {

static_assert(kSimMaxBarcode == kMaxBarcode, "a simulated barcode is one the searches accept");

struct SimCall {
  SimParams p{};
  std::vector<uint16_t> posinfo;          // per oligo position: message bits consumed before it | block type << 12
  uint8_t bc[2 * kSimMaxBarcode] = {0};   // start barcode, end barcode as 0..3
};

// The pool of the lva_simulate_pool_* pair, as the caller gave it; the other pair passes none.
struct SimPoolHost {
  const uint8_t* msgs;
  int32_t n;
  const uint32_t* cdf;
};

bool sim_pool_ok(const SimPoolHost& pool, uint32_t msg_len) {
  if (!pool.msgs || pool.n < 1 || pool.n > kSimMaxPool || (uint64_t)pool.n * msg_len >= ((uint64_t)1 << 31)) return false;
  const size_t bytes = (size_t)pool.n * msg_len;
  for (size_t i = 0; i < bytes; ++i)
    if (pool.msgs[i] > 1) return false;
  if (pool.cdf) {
    for (int32_t k = 1; k < pool.n; ++k)
      if (pool.cdf[k] < pool.cdf[k - 1]) return false;
    if (pool.cdf[pool.n - 1] != 0xFFFFFFFFu) return false;
  }
  return true;
}

// a call's own arguments, the barcodes apart: everything the entry points share.  pool: null, or what rc_mode 3 needs
int sim_args(lva_decoder* d, uint64_t seed, uint32_t first_read, int32_t n, uint32_t sub_thr, uint32_t del_thr, uint32_t ins_thr,
             const uint32_t* dwell_cdf, int32_t dwell_k, int32_t rc_mode, const SimPoolHost* pool, SimCall* c) {
  if (!d || n < 0 || !dwell_cdf || dwell_k < 1 || dwell_k > kSimMaxDwell || rc_mode < 0 || rc_mode > (pool ? 3 : 2)) return LVA_ERR_ARG;
  if ((uint64_t)first_read + (uint64_t)n > ((uint64_t)1 << 32)) return LVA_ERR_ARG;        // read numbers are 32-bit
  if (sub_thr > kSimMaxThreshold || del_thr > kSimMaxThreshold || ins_thr > kSimMaxThreshold) return LVA_ERR_ARG;
  if (pool && !sim_pool_ok(*pool, d->code[0].msg_len)) return LVA_ERR_ARG;
  if (!d->sync_marker.empty()) return LVA_ERR_UNSUPPORTED;                                 // lva_encode takes no marker
  const Code& code = d->code[0];
  SimParams& p = c->p;
  p.k0 = (uint32_t)seed; p.k1 = (uint32_t)(seed >> 32);
  p.first_read = first_read;
  p.thr_sub = sub_thr; p.thr_del = del_thr; p.thr_ins = ins_thr;
  p.dwell_k = (uint32_t)dwell_k;
  p.msg_len = code.msg_len; p.mem_conv = (uint32_t)code.mem_conv;
  p.g0 = code.g[0]; p.g1 = code.g[1]; p.init = code.init; p.fin = code.fin;
  p.oligo_len = code.oligo_len();
  p.rc_mode = (uint32_t)rc_mode;
  c->posinfo.resize(p.oligo_len);
  for (uint32_t pos = 0; pos < p.oligo_len; ++pos)
    c->posinfo[pos] = (uint16_t)(code.pos2msg[pos] | (uint32_t)code.pattern[pos % (uint32_t)code.plen] << 12);
  return LVA_OK;
}

bool sim_barcode(const char* s, uint8_t* dst, uint32_t* len) {
  const size_t n = std::strlen(s);
  if (n == 0 || n > (size_t)kSimMaxBarcode) return false;
  for (size_t i = 0; i < n; ++i) {
    const char* at = std::strchr("ACGT", s[i]);
    if (!at) return false;
    dst[i] = (uint8_t)(at - "ACGT");
  }
  *len = (uint32_t)n;
  return true;
}

// both barcodes or neither; with them the flank range and the length of the longest strand
int sim_barcodes(const char* start_bc, const char* end_bc, uint32_t flank_lo, uint32_t flank_hi, SimCall* c) {
  if (!start_bc && !end_bc) return LVA_OK;
  if (!start_bc || !end_bc) return LVA_ERR_ARG;
  SimParams& p = c->p;
  if (!sim_barcode(start_bc, c->bc, &p.len_start) || !sim_barcode(end_bc, c->bc + kSimMaxBarcode, &p.len_end)) return LVA_ERR_ARG;
  if (flank_lo > flank_hi || flank_hi > (uint32_t)kSimMaxFlank) return LVA_ERR_ARG;
  if (2 * flank_hi + p.len_start + p.len_end + p.oligo_len > (uint32_t)kSimMaxStrand) return LVA_ERR_ARG;
  p.barcoded = 1; p.flank_lo = flank_lo; p.flank_span = flank_hi - flank_lo + 1;
  return LVA_OK;
}

struct SimTables {
  Arena::Piece<uint16_t> posinfo;
  Arena::Piece<uint32_t> cdf;
  Arena::Piece<uint8_t> bc;
  Arena::Piece<uint8_t> pool;             // with a pool only: its messages, its table if it has one, and per read what was drawn
  Arena::Piece<uint32_t> pool_cdf;
  Arena::Piece<int32_t> source;
  Arena::Piece<uint8_t> rc;
};
SimTables sim_tables(Arena& a, const SimCall& c, const SimPoolHost* pool, size_t n_reads) {
  SimTables t{a.add<uint16_t>(c.posinfo.size()), a.add<uint32_t>(c.p.dwell_k), a.add<uint8_t>(sizeof c.bc), {}, {}, {}, {}};
  if (pool) {
    t.pool = a.add<uint8_t>((size_t)pool->n * c.p.msg_len);
    if (pool->cdf) t.pool_cdf = a.add<uint32_t>((size_t)pool->n);
    t.source = a.add<int32_t>(n_reads);
    t.rc = a.add<uint8_t>(n_reads);
  }
  return t;
}
// c, dwell_cdf and the pool outlive the call's StreamDrain.  *dev: the pool as the kernel takes it (pool == null: untouched)
int upload_sim_tables(lva_decoder* d, const Arena& a, const SimTables& t, const SimCall& c, const uint32_t* dwell_cdf,
                      const SimPoolHost* pool, SimPool* dev) {
  HIP_TRY(hipMemcpyAsync(a.ptr(t.posinfo), c.posinfo.data(), 2 * c.posinfo.size(), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(a.ptr(t.cdf), dwell_cdf, 4 * (size_t)c.p.dwell_k, hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(a.ptr(t.bc), c.bc, sizeof c.bc, hipMemcpyHostToDevice, d->stream));
  if (!pool) return LVA_OK;
  HIP_TRY(hipMemcpyAsync(a.ptr(t.pool), pool->msgs, (size_t)pool->n * c.p.msg_len, hipMemcpyHostToDevice, d->stream));
  if (pool->cdf) HIP_TRY(hipMemcpyAsync(a.ptr(t.pool_cdf), pool->cdf, 4 * (size_t)pool->n, hipMemcpyHostToDevice, d->stream));
  dev->msgs = a.ptr(t.pool);
  dev->cdf = a.ptr(t.pool_cdf);
  dev->n = (uint32_t)pool->n;
  dev->source = a.ptr(t.source);
  dev->rc = a.ptr(t.rc);
  return LVA_OK;
}

// the one body of lva_simulate_plan and lva_simulate_pool_plan (pool == null: the former)
int simulate_plan(lva_decoder* d, uint64_t seed, uint32_t first_read, int32_t n_reads, uint32_t sub_thr, uint32_t del_thr,
                  uint32_t ins_thr, const uint32_t* dwell_cdf, int32_t dwell_k, const char* start_barcode, const char* end_barcode,
                  uint32_t flank_lo, uint32_t flank_hi, int32_t rc_mode, const SimPoolHost* pool, int64_t* row_offsets_out,
                  int64_t* base_offsets_out) {
  SimCall c;
  int st = sim_args(d, seed, first_read, n_reads, sub_thr, del_thr, ins_thr, dwell_cdf, dwell_k, rc_mode, pool, &c);
  if (st == LVA_OK && (!row_offsets_out || !base_offsets_out)) st = LVA_ERR_ARG;
  if (st != LVA_OK) return st;
  if ((st = sim_barcodes(start_barcode, end_barcode, flank_lo, flank_hi, &c)) != LVA_OK) return st;
  st = stage_enter(d, n_reads == 0);
  if (st == LVA_OK) row_offsets_out[0] = base_offsets_out[0] = 0;
  if (st != kRun) return st;
  const size_t n = (size_t)n_reads;
  std::vector<int32_t> lens(2 * n);
  Arena arena;
  const SimTables tab = sim_tables(arena, c, pool, n);
  const auto d_lens = arena.add<int32_t>(2 * n);
  if (arena.alloc() != LVA_OK) return LVA_ERR_NOMEM;
  StreamDrain drain(d->stream);
  SimPool dpool;
  if ((st = upload_sim_tables(d, arena, tab, c, dwell_cdf, pool, &dpool)) != LVA_OK) return st;
  const int e = launch_sim_strand(c.p, pool ? &dpool : nullptr, n_reads, arena.ptr(tab.posinfo), arena.ptr(tab.cdf),
                                  arena.ptr(tab.bc), nullptr, nullptr, arena.ptr(d_lens), nullptr, nullptr, nullptr, nullptr,
                                  d->stream);
  if (e) return launch_status(e);
  HIP_TRY(hipMemcpyAsync(lens.data(), arena.ptr(d_lens), 8 * n, hipMemcpyDeviceToHost, d->stream));
  if ((st = drain.finish()) != LVA_OK) return st;
  row_offsets_out[0] = base_offsets_out[0] = 0;
  for (size_t i = 0; i < n; ++i) {
    base_offsets_out[i + 1] = base_offsets_out[i] + lens[2 * i];
    row_offsets_out[i + 1] = row_offsets_out[i] + lens[2 * i + 1];
  }
  size_t T = 0;                                                   // a batch the other stages would refuse is refused here
  return check_offsets(row_offsets_out, n_reads, &T);
}

// the one body of lva_simulate_fill_device and lva_simulate_pool_fill_device (pool == null: the former)
int simulate_fill(lva_decoder* d, uint64_t seed, uint32_t first_read, int32_t n_reads, uint32_t sub_thr, uint32_t del_thr,
                  uint32_t ins_thr, const uint32_t* dwell_cdf, int32_t dwell_k, const char* start_barcode, const char* end_barcode,
                  uint32_t flank_lo, uint32_t flank_hi, int32_t rc_mode, const SimPoolHost* pool, float scale, float margin,
                  float clip, const int64_t* row_offsets, const int64_t* base_offsets, float* scores_dev, uint8_t* msgs_out,
                  uint8_t* bases_out, uint8_t* true_idx_out, int32_t* source_out, uint8_t* rc_out) {
  SimCall c;
  int st = sim_args(d, seed, first_read, n_reads, sub_thr, del_thr, ins_thr, dwell_cdf, dwell_k, rc_mode, pool, &c);
  if (st != LVA_OK) return st;
  if (!row_offsets || !base_offsets || !(clip > 0.0f) || scale != scale || margin != margin) return LVA_ERR_ARG;
  size_t T = 0, B = 0;
  if (check_offsets(row_offsets, n_reads, &T) != LVA_OK || check_offsets(base_offsets, n_reads, &B) != LVA_OK) return LVA_ERR_ARG;
  if ((uint64_t)T * 10 >= ((uint64_t)1 << 32)) return LVA_ERR_ARG;              // sim_scores counts 16-byte quads in 32 bits
  if (n_reads > 0 && (!scores_dev || ((uintptr_t)scores_dev & 15u) || !msgs_out)) return LVA_ERR_ARG;
  if ((st = sim_barcodes(start_barcode, end_barcode, flank_lo, flank_hi, &c)) != LVA_OK) return st;
  st = stage_enter(d, n_reads == 0);
  if (st != kRun) return st;
  const size_t n = (size_t)n_reads, mb = n * c.p.msg_len;
  int32_t bad = 0;
  Arena arena;
  const SimTables tab = sim_tables(arena, c, pool, n);
  const auto d_row = arena.add<int64_t>(n + 1), d_base = arena.add<int64_t>(n + 1);
  const auto d_msgs = arena.add<uint8_t>(mb), d_bases = arena.add<uint8_t>(B), d_tidx = arena.add<uint8_t>(T);
  const auto d_bad = arena.add<int32_t>(1);
  if (arena.alloc() != LVA_OK) return LVA_ERR_NOMEM;
  StreamDrain drain(d->stream);
  SimPool dpool;
  if ((st = upload_sim_tables(d, arena, tab, c, dwell_cdf, pool, &dpool)) != LVA_OK) return st;
  HIP_TRY(hipMemcpyAsync(arena.ptr(d_row), row_offsets, 8 * (n + 1), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemcpyAsync(arena.ptr(d_base), base_offsets, 8 * (n + 1), hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemsetAsync(arena.ptr(d_bad), 0, sizeof(int32_t), d->stream));
  int e = launch_sim_strand(c.p, pool ? &dpool : nullptr, n_reads, arena.ptr(tab.posinfo), arena.ptr(tab.cdf), arena.ptr(tab.bc),
                            arena.ptr(d_row), arena.ptr(d_base), nullptr, arena.ptr(d_msgs), arena.ptr(d_bases), arena.ptr(d_tidx),
                            arena.ptr(d_bad), d->stream);
  if (e) return launch_status(e);
  HIP_TRY(hipEventRecord(d->ev_total0, d->stream));
  e = launch_sim_scores(c.p, n_reads, arena.ptr(d_row), (uint32_t)T, arena.ptr(d_tidx), scale, margin, clip, scores_dev, d->stream);
  if (e) return launch_status(e);
  HIP_TRY(hipEventRecord(d->ev_total1, d->stream));
  HIP_TRY(hipMemcpyAsync(msgs_out, arena.ptr(d_msgs), mb, hipMemcpyDeviceToHost, d->stream));
  if (bases_out && B) HIP_TRY(hipMemcpyAsync(bases_out, arena.ptr(d_bases), B, hipMemcpyDeviceToHost, d->stream));
  if (true_idx_out && T) HIP_TRY(hipMemcpyAsync(true_idx_out, arena.ptr(d_tidx), T, hipMemcpyDeviceToHost, d->stream));
  if (pool && source_out) HIP_TRY(hipMemcpyAsync(source_out, arena.ptr(tab.source), 4 * n, hipMemcpyDeviceToHost, d->stream));
  if (pool && rc_out) HIP_TRY(hipMemcpyAsync(rc_out, arena.ptr(tab.rc), n, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipMemcpyAsync(&bad, arena.ptr(d_bad), sizeof(int32_t), hipMemcpyDeviceToHost, d->stream));
  if ((st = drain.finish()) != LVA_OK) return st;
  if ((st = tp_profile(d, T, true)) != LVA_OK) return st;
  return bad ? LVA_ERR_ARG : LVA_OK;           // the offsets are not this call's plan: nothing was written outside them
}

}  // namespace

extern "C" {

int lva_simulate_plan(lva_decoder* d, uint64_t seed, uint32_t first_read, int32_t n_reads, uint32_t sub_thr, uint32_t del_thr,
                      uint32_t ins_thr, const uint32_t* dwell_cdf, int32_t dwell_k, const char* start_barcode,
                      const char* end_barcode, uint32_t flank_lo, uint32_t flank_hi, int32_t rc_mode, int64_t* row_offsets_out,
                      int64_t* base_offsets_out) {
  return simulate_plan(d, seed, first_read, n_reads, sub_thr, del_thr, ins_thr, dwell_cdf, dwell_k, start_barcode, end_barcode,
                       flank_lo, flank_hi, rc_mode, nullptr, row_offsets_out, base_offsets_out);
}

int lva_simulate_fill_device(lva_decoder* d, uint64_t seed, uint32_t first_read, int32_t n_reads, uint32_t sub_thr,
                             uint32_t del_thr, uint32_t ins_thr, const uint32_t* dwell_cdf, int32_t dwell_k,
                             const char* start_barcode, const char* end_barcode, uint32_t flank_lo, uint32_t flank_hi,
                             int32_t rc_mode, float scale, float margin, float clip, const int64_t* row_offsets,
                             const int64_t* base_offsets, float* scores_dev, uint8_t* msgs_out, uint8_t* bases_out,
                             uint8_t* true_idx_out) {
  return simulate_fill(d, seed, first_read, n_reads, sub_thr, del_thr, ins_thr, dwell_cdf, dwell_k, start_barcode, end_barcode,
                       flank_lo, flank_hi, rc_mode, nullptr, scale, margin, clip, row_offsets, base_offsets, scores_dev, msgs_out,
                       bases_out, true_idx_out, nullptr, nullptr);
}

int lva_simulate_pool_plan(lva_decoder* d, uint64_t seed, uint32_t first_read, int32_t n_reads, uint32_t sub_thr, uint32_t del_thr,
                           uint32_t ins_thr, const uint32_t* dwell_cdf, int32_t dwell_k, const char* start_barcode,
                           const char* end_barcode, uint32_t flank_lo, uint32_t flank_hi, int32_t rc_mode, const uint8_t* pool,
                           int32_t n_pool, const uint32_t* pool_cdf, int64_t* row_offsets_out, int64_t* base_offsets_out) {
  const SimPoolHost ph{pool, n_pool, pool_cdf};
  return simulate_plan(d, seed, first_read, n_reads, sub_thr, del_thr, ins_thr, dwell_cdf, dwell_k, start_barcode, end_barcode,
                       flank_lo, flank_hi, rc_mode, &ph, row_offsets_out, base_offsets_out);
}

int lva_simulate_pool_fill_device(lva_decoder* d, uint64_t seed, uint32_t first_read, int32_t n_reads, uint32_t sub_thr,
                                  uint32_t del_thr, uint32_t ins_thr, const uint32_t* dwell_cdf, int32_t dwell_k,
                                  const char* start_barcode, const char* end_barcode, uint32_t flank_lo, uint32_t flank_hi,
                                  int32_t rc_mode, const uint8_t* pool, int32_t n_pool, const uint32_t* pool_cdf, float scale,
                                  float margin, float clip, const int64_t* row_offsets, const int64_t* base_offsets,
                                  float* scores_dev, uint8_t* msgs_out, uint8_t* bases_out, uint8_t* true_idx_out,
                                  int32_t* source_out, uint8_t* rc_out) {
  const SimPoolHost ph{pool, n_pool, pool_cdf};
  return simulate_fill(d, seed, first_read, n_reads, sub_thr, del_thr, ins_thr, dwell_cdf, dwell_k, start_barcode, end_barcode,
                       flank_lo, flank_hi, rc_mode, &ph, scale, margin, clip, row_offsets, base_offsets, scores_dev, msgs_out,
                       bases_out, true_idx_out, source_out, rc_out);
}

}  // extern "C"
