// lva_stages.cpp -- C ABI (include/lva_decoder.h) of the stages beside the list decoder: transition posteriors (N0), basecall
// and barcode localisation (N3), demultiplexing (N3'), the consumers of a decoded list (N2), the Reed-Solomon outer code (N4),
// reading-cost trials (N4'), the read simulator (S), the error profile (N5), read mapping (N6), the one-message trellis and its traceback (N7).  No algorithm lives here: an entry point checks its arguments, then works
// through one Frame (below): it declares its device pieces together with their host side, begins (allocate, upload),
// launches, finishes (copy back, wait).
#include <algorithm>
#include <cstring>
#include <new>
#include <utility>

#include "lva_host.h"
#include "bc_kernels.h"
#include "tp_kernels.h"
#include "ls_kernels.h"
#include "rs_kernels.h"
#include "sim_kernels.h"
#include "tr_kernels.h"
#include "ep_kernels.h"
#include "mp_kernels.h"
#include "mq_kernels.h"
#include "mi_kernels.h"
#include "fw_kernels.h"
#include "sc_kernels.h"
#include "st_kernels.h"

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

// What one side-stage call owns on the device: the stream it works on, ONE allocation carved into 256-byte aligned and
// padded pieces, and the drain.  A piece is declared once, with its host side: in (uploaded by begin), out (copied back by
// finish; a null host pointer: no copy), inout (both, two host addresses), scratch (neither); resident: device memory that
// someone else owns and has filled, carried as a piece so that a call reads it like its own.  begin() sizes the block from
// what was declared and every whole-piece copy takes its bytes from the declaration: neither can disagree with a piece.
// The destructor drains, then frees, then destroys an owned stream, on every exit.  Host buffers that the copies read or
// write are declared before the frame, so that they die after it.
class Frame {
  struct Side { size_t at, bytes; const void* src; void* dst; };

 public:
  // Converts to its typed device pointer, valid from begin() on.  Default: a piece that was not asked for, a null pointer.
  template <typename T> struct Piece {
    const Frame* f = nullptr;
    size_t at = 0, count = 0;
    T* elsewhere = nullptr;                            // resident(): not in the frame's block
    T* ptr() const { return elsewhere ? elsewhere : f ? reinterpret_cast<T*>(f->base_ + at) : nullptr; }
    operator T*() const { return ptr(); }
  };
  Frame() = default;                                   // a device-ordinal call: open() makes the stream
  explicit Frame(hipStream_t decoder_stream) : s_(decoder_stream) {}
  Frame(const Frame&) = delete;
  ~Frame() {
    if (!done_ && s_) (void)hipStreamSynchronize(s_);
    if (base_) (void)hipFree(base_);
    if (own_) (void)hipStreamDestroy(s_);
  }
  // the device by its ordinal, and a non-blocking stream of the call's own: no decoder's stream or profile is touched
  int open(int32_t device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return LVA_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return LVA_ERR_NO_DEVICE;
    HIP_TRY(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
    own_ = true;
    return LVA_OK;
  }
  hipStream_t stream() const { return s_; }
  // a piece of count 0 still occupies one padded unit; ls_filter reads whole dwords up to the padded end of its messages
  template <typename T> Piece<T> inout(const T* src, T* dst, size_t count) {
    const Piece<T> p{this, size_, count};
    sides_.push_back({size_, count * sizeof(T), src, dst});
    size_ += (std::max<size_t>(count, 1) * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
  template <typename T> Piece<T> in(const T* src, size_t count) { return inout<T>(src, nullptr, count); }
  template <typename T> Piece<T> out(T* dst, size_t count) { return inout<T>(nullptr, dst, count); }
  template <typename T> Piece<T> scratch(size_t count) { return inout<T>(nullptr, nullptr, count); }
  template <typename T> Piece<T> resident(const T* dev, size_t count) const { return Piece<T>{nullptr, 0, count, const_cast<T*>(dev)}; }
  int begin() {                                        // allocate, enqueue the uploads
    if (size_ && hipMalloc(reinterpret_cast<void**>(&base_), size_) != hipSuccess) return LVA_ERR_NOMEM;
    for (const Side& x : sides_)
      if (x.src && x.bytes) HIP_TRY(hipMemcpyAsync(base_ + x.at, x.src, x.bytes, hipMemcpyHostToDevice, s_));
    return LVA_OK;
  }
  int finish() {                                       // the success exit: enqueue the downloads, wait, report what the wait reports
    for (const Side& x : sides_)
      if (x.dst && x.bytes) HIP_TRY(hipMemcpyAsync(x.dst, base_ + x.at, x.bytes, hipMemcpyDeviceToHost, s_));
    done_ = true;
    HIP_TRY(hipStreamSynchronize(s_));
    return LVA_OK;
  }
  // The escape hatch for what is not a whole piece: bytes to or from a host address on the frame's stream ...
  int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, s_));
    return LVA_OK;
  }
  // ... and `count` elements of a piece from element `first` on, to the host
  template <typename T> int download(T* host, Piece<T> p, size_t first, size_t count) {
    if (first + count > p.count) { set_hip_error("Frame::download: outside the piece"); return LVA_ERR_HIP; }
    return copy(host, p.ptr() + first, count * sizeof(T), hipMemcpyDeviceToHost);
  }

 private:
  hipStream_t s_ = nullptr;
  bool own_ = false, done_ = false;
  char* base_ = nullptr;
  size_t size_ = 0;
  std::vector<Side> sides_;
};
template <typename T> using Piece = Frame::Piece<T>;

constexpr size_t kPostRow = 40;      // floats per block of a posterior or score matrix

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
// (basecall_set: its working set, what the caller wants of it copied back) or the caller's own, uploaded (given_set; nb:
// read_lengths).  Declaration order = order in the block.
struct Calls {
  Piece<int64_t> off;
  Piece<uint32_t> tb;     // 8 back-pointer bytes per block
  Piece<uint8_t> path;
  Piece<char> bases;
  Piece<uint32_t> trans;
  Piece<int32_t> nb;
};
Calls basecall_set(Frame& f, const int64_t* row_offsets, size_t n, size_t T, char* bases_out, uint32_t* trans_out, int32_t* nb_out) {
  return {f.in(row_offsets, n + 1), f.scratch<uint32_t>(2 * T), f.scratch<uint8_t>(T + n), f.out(bases_out, T), f.out(trans_out, T),
          f.out(nb_out, n)};
}
Calls given_set(Frame& f, const char* bases, const uint32_t* trans, const int64_t* base_offsets, const std::vector<int32_t>& nb, size_t T) {
  return {f.in(base_offsets, nb.size() + 1), {}, {}, f.in(bases, T), f.in(trans, T), f.in(nb.data(), nb.size())};
}

// Windows into a caller's base buffer (read i: bases[first_base[i] .. + n_bases[i]); they may overlap or lie far apart), as
// the error profile and read mapping take them: checked, packed one after the other, declared on the call's frame.  A
// call that shortens windows fills nb and packs with it.  Declared before the frame: the uploads read the vectors.
struct Windows {
  std::vector<uint8_t> packed;
  std::vector<int32_t> win_off, nb;
  Piece<uint8_t> bases;
  Piece<int32_t> off, len;
  // everything about n windows that can be refused without the device: a start below 0, a length outside [0, limit], 2^31 bases in all
  static int check(const int64_t* first_base, const int32_t* n_bases, int32_t n, int32_t limit) {
    uint64_t sum = 0;
    for (int32_t i = 0; i < n; ++i) {
      if (first_base[i] < 0 || n_bases[i] < 0 || n_bases[i] > limit) return LVA_ERR_ARG;
      sum += (uint64_t)n_bases[i];
    }
    return sum >= (1ull << 31) ? LVA_ERR_ARG : LVA_OK;
  }
  // lens: n_bases as check() passed them, or nb
  void pack(Frame& f, const uint8_t* src, const int64_t* first_base, const int32_t* lens, size_t n) {
    win_off.resize(n);
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) { win_off[i] = (int32_t)at; at += (size_t)lens[i]; }
    packed.resize(at);
    for (size_t i = 0; i < n; ++i)
      if (lens[i] > 0) std::memcpy(packed.data() + win_off[i], src + first_base[i], (size_t)lens[i]);
    bases = f.in(packed.data(), at); off = f.in(win_off.data(), n); len = f.in(lens, n);
  }
  // what a launcher takes for the chunk of reads that starts at read a
  struct Chunk { const uint8_t* bases; const int32_t* off; const int32_t* len; };
  Chunk from(size_t a) const { return {bases, off.ptr() + a, len.ptr() + a}; }
};

// bc_basecall over posteriors that are on the device
int enqueue_basecall(const Frame& f, const Calls& c, const float* post_dev, int32_t n) {
  return launch_status(launch_bc_basecall(post_dev, c.off, n, c.tb, c.path, c.bases, c.trans, c.nb, f.stream()));
}

struct LocateSet { Piece<uint32_t> best; Piece<BcResult> res; };
LocateSet locate_set(Frame& f, size_t n, lva_payload_pos* out) {       // out: the windows, to the caller
  static_assert(sizeof(lva_payload_pos) == sizeof(BcResult), "lva_payload_pos layout");
  return {f.scratch<uint32_t>(4 * n), f.out(reinterpret_cast<BcResult*>(out), n)};
}

// bc_search + bc_finalize over basecalls that are on the device
int enqueue_locate(const Frame& f, const Calls& c, const LocateSet& s, int32_t n, const BcPatterns& pat, int n_orient, uint32_t min_len) {
  int e = launch_bc_search(c.bases, c.off, c.nb, n, pat, n_orient, s.best, f.stream());
  if (!e) e = launch_bc_finalize(c.trans, c.off, c.nb, n, pat, n_orient, min_len, s.best, s.res, f.stream());
  return launch_status(e);
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
  Frame f(d->stream);
  const Piece<float> up = post_on_host ? f.in(post, kPostRow * T) : Piece<float>{};
  const Calls bc = basecall_set(f, row_offsets, (size_t)n, T, bases_out, trans_out, nbases_out);
  const LocateSet loc = locate_set(f, (size_t)n, pos_out);
  if ((st = f.begin()) != LVA_OK) return st;
  if ((st = enqueue_basecall(f, bc, post_on_host ? up.ptr() : post, n)) != LVA_OK) return st;
  if (n_orient && (st = enqueue_locate(f, bc, loc, n, pat, n_orient, min_len)) != LVA_OK) return st;
  return f.finish();
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
  Frame f(d->stream);
  const Calls calls = given_set(f, bases, trans, base_offsets, nb, T);
  const LocateSet loc = locate_set(f, nb.size(), out);
  if ((st = f.begin()) != LVA_OK) return st;
  if ((st = enqueue_locate(f, calls, loc, n_reads, pat, 1, 0)) != LVA_OK) return st;
  return f.finish();
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// transition posteriors from a network's transition scores.
// ---------------------------------------------------------------------------------------------
namespace {

// A decoder-owned block that outlives the call by design: it grows to `want` units of `unit` bytes and never shrinks.
template <typename T> int tp_grow(lva_decoder* d, T** buf, size_t* cap, size_t want, size_t unit) {
  if (want <= *cap) return LVA_OK;
  HIP_TRY(hipStreamSynchronize(d->stream));
  if (*buf) (void)hipFree(*buf);
  *buf = nullptr; *cap = 0;
  if (hipMalloc(reinterpret_cast<void**>(buf), want * unit) != hipSuccess) return LVA_ERR_NOMEM;
  *cap = want;
  return LVA_OK;
}

// forward and backward kernel over n reads resident on the device; post_dev may be scores_dev.  Enqueues only.
int tp_run(lva_decoder* d, Frame& f, const float* scores_dev, const int64_t* row_offsets, int32_t n, size_t T, float* post_dev) {
  int st = tp_grow(d, &d->d_tp_fwd, &d->tp_fwd_cap, T, 8 * sizeof(float));
  if (st == LVA_OK) st = tp_grow(d, &d->d_tp_off, &d->tp_off_cap, std::max<size_t>((size_t)n + 1, 1024), sizeof(int64_t));
  if (st == LVA_OK) st = f.copy(d->d_tp_off, row_offsets, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice);
  if (st != LVA_OK) return st;
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
  Frame f(d->stream);                        // (the device variant has no piece, but the offsets are copied from the caller's memory)
  const Piece<float> io = on_host ? f.inout(scores, post, kPostRow * T) : Piece<float>{};     // up from scores, in place, down to post
  if ((st = f.begin()) != LVA_OK) return st;
  if ((st = tp_run(d, f, on_host ? io.ptr() : scores, row_offsets, n, T, on_host ? io.ptr() : post)) != LVA_OK) return st;
  if ((st = f.finish()) != LVA_OK) return st;
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
  Piece<BcPatterns> pats;
  Piece<uint32_t> min_len;
  Piece<uint32_t> best;
  Piece<BcDemuxResult> res;
  Piece<BcResult> all;    // only when the caller asks for every experiment's candidate
};
// x (demux_args) is declared before the frame; out, all_out: the results, to the caller
DemuxSet demux_set(Frame& f, size_t n, const DemuxArgs& x, lva_demux_pos* out, lva_payload_pos* all_out) {
  static_assert(sizeof(lva_demux_pos) == sizeof(BcDemuxResult), "lva_demux_pos layout");
  const size_t k = x.pats.size();
  return {f.in(x.pats.data(), k), f.in(x.min_len.data(), k), f.scratch<uint32_t>(4 * n * k), f.out(reinterpret_cast<BcDemuxResult*>(out), n),
          all_out ? f.out(reinterpret_cast<BcResult*>(all_out), n * k) : Piece<BcResult>{}};
}

// search + choice over basecalls that are on the device
int enqueue_demux(const Frame& f, const Calls& c, const DemuxSet& s, int32_t n_reads, const DemuxArgs& x) {
  const int32_t k = (int32_t)x.pats.size();
  int e = launch_bc_search_multi(c.bases, c.off, c.nb, n_reads, s.pats, k, s.best, f.stream());
  if (!e) e = launch_bc_demux_finalize(c.trans, c.off, c.nb, n_reads, s.pats, s.min_len, k, x.max_dist, x.min_margin, s.best, s.res, s.all,
                                       f.stream());
  return launch_status(e);
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
  Frame f(d->stream);
  const Piece<float> up = post_on_host ? f.in(post, kPostRow * T) : Piece<float>{};
  const Calls bc = basecall_set(f, row_offsets, (size_t)n, T, nullptr, nullptr, nullptr);
  const DemuxSet dm = demux_set(f, (size_t)n, x, out, all_out);
  if ((st = f.begin()) != LVA_OK) return st;
  if ((st = enqueue_basecall(f, bc, post_on_host ? up.ptr() : post, n)) != LVA_OK) return st;
  if ((st = enqueue_demux(f, bc, dm, n, x)) != LVA_OK) return st;
  return f.finish();
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
  Frame f(d->stream);
  const Calls calls = given_set(f, bases, trans, base_offsets, nb, T);
  const DemuxSet dm = demux_set(f, nb.size(), x, out, all_out);
  if ((st = f.begin()) != LVA_OK) return st;
  if ((st = enqueue_demux(f, calls, dm, n_reads, x)) != LVA_OK) return st;
  return f.finish();
}

}  // extern "C"

/* ---------------------------------------------------------------------------------------------
 * the consumers of a decoded list (csrc/ls_kernels.hip).  Like the RS entry
 * points they take a device ordinal, work on a stream of their own (Frame::open) and leave every decoder's profile
 * alone.  Arguments first, then the device ordinal.
 * ------------------------------------------------------------------------------------------- */
namespace {

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
  Frame f;
  if (const int so = f.open(device)) return so;
  const size_t n = (size_t)n_reads;
  const auto d_msgs = f.in(msgs, n * (size_t)list_size * msg_len);     // 256-byte aligned and padded: whole dwords may be read
  const auto d_counts = f.in(counts, n);
  const auto d_index = f.out(out_index, n), d_rank = f.out(out_rank, n);
  const auto d_pay = f.out(out_payload, n * (size_t)bytes_per_oligo);
  if (const int st = f.begin()) return st;
  const int e = launch_ls_filter(d_msgs, d_counts, n_reads, list_size, msg_len, use, bytes_per_oligo, num_oligos, pad, d_index, d_rank,
                                 d_pay, f.stream());
  return e ? launch_status(e) : f.finish();
}

int lva_list_consensus(int32_t device, const int32_t* index, const uint8_t* payload, int32_t n_reads, int32_t bytes_per_oligo,
                       int32_t num_oligos, int32_t first_only, uint8_t* out_present, uint8_t* out_payload, int32_t* out_votes) {
  if (!index || !payload || !out_present || !out_payload || !out_votes) return LVA_ERR_ARG;
  if (n_reads < 0 || bytes_per_oligo < 1 || num_oligos < 1 || num_oligos > 4096) return LVA_ERR_ARG;
  if ((uint64_t)n_reads * (uint64_t)bytes_per_oligo >= (1ull << 31)) return LVA_ERR_ARG;
  for (int32_t i = 0; i < n_reads; ++i)
    if (index[i] >= num_oligos) return LVA_ERR_ARG;      // (negative: the read passed no entry and has no vote)
  if (n_reads == 0) return LVA_OK;
  Frame f;
  if (const int so = f.open(device)) return so;
  const size_t n = (size_t)n_reads, no = (size_t)num_oligos;
  const auto d_index = f.in(index, n);
  const auto d_order = f.scratch<int32_t>(n);
  const auto d_pay = f.in(payload, n * (size_t)bytes_per_oligo);
  const auto d_bucket = f.scratch<int32_t>(no + 1);
  const auto d_present = f.out(out_present, no), d_out = f.out(out_payload, no * (size_t)bytes_per_oligo);
  const auto d_votes = f.out(out_votes, no);
  if (const int st = f.begin()) return st;
  const int e = launch_ls_consensus(d_index, d_pay, n_reads, bytes_per_oligo, num_oligos, first_only ? 1 : 0, d_bucket, d_order, d_present,
                                    d_out, d_votes, f.stream());
  return e ? launch_status(e) : f.finish();
}

int lva_list_stats(int32_t device, const uint8_t* msgs, const int32_t* counts, const uint8_t* truth, int32_t n_reads,
                   int32_t list_size, uint32_t msg_len, lva_list_stat* out) {
  static_assert(sizeof(lva_list_stat) == kLsStatFields * sizeof(int32_t), "ls_stats writes the fields of lva_list_stat in order");
  if (!msgs || !counts || !truth || !out) return LVA_ERR_ARG;
  if (!ls_shape_ok(n_reads, list_size, msg_len)) return LVA_ERR_ARG;
  if (n_reads == 0) return LVA_OK;
  Frame f;
  if (const int so = f.open(device)) return so;
  const size_t n = (size_t)n_reads;
  const auto d_msgs = f.in(msgs, n * (size_t)list_size * msg_len);
  const auto d_counts = f.in(counts, n);
  const auto d_truth = f.in(truth, n * msg_len);
  const auto d_packed = f.scratch<uint64_t>(kLsPackWords * n);
  const auto d_out = f.out(reinterpret_cast<int32_t*>(out), kLsStatFields * n);
  if (const int st = f.begin()) return st;
  const int e = launch_ls_stats(d_msgs, d_counts, d_truth, n_reads, list_size, msg_len, d_packed, d_out, f.stream());
  return e ? launch_status(e) : f.finish();
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// the Reed-Solomon outer code (csrc/rs_kernels.hip).  A device ordinal, a stream of its
// own, complete on return; lva_rs_last_error is the text of the calling thread's last failed RS call.
// ---------------------------------------------------------------------------------------------
namespace {

thread_local std::string g_rs_error;

bool rs_shape_ok(int n_cw, int n_total, int fec) { return n_cw >= 0 && fec >= 1 && fec <= kRsMaxFec && n_total > fec && n_total <= kRsN; }

// n_cw > 0 codewords of n_total symbols -> their first n_out decoded symbols; ok may be null (its piece is still written)
int rs_run(int32_t device, const uint16_t* symbols, int32_t n_cw, int32_t n_total, int32_t fec, const int32_t* erasures, int32_t n_er,
           uint16_t pad_sym, uint16_t fail_sym, uint16_t* out, int32_t n_out, int32_t* ok) {
  std::vector<uint16_t> gexp, glog;
  Frame f;
  if (const int so = f.open(device)) return so;
  tr_gf_tables(&gexp, &glog);
  const auto d_sym = f.in(symbols, (size_t)n_cw * n_total);
  const auto d_out = f.out(out, (size_t)n_cw * n_out);
  const auto d_gexp = f.in(gexp.data(), gexp.size()), d_glog = f.in(glog.data(), glog.size());
  const auto d_er = f.in(erasures, (size_t)n_er);
  const auto d_ok = f.out(ok, (size_t)n_cw);
  int st = f.begin();
  if (st == LVA_OK)
    st = launch_status(launch_rs_decode(d_sym, n_cw, n_total, fec, d_er, n_er, pad_sym, fail_sym, d_gexp, d_glog, d_out, n_out, d_ok,
                                        f.stream()));
  if (st == LVA_OK) st = f.finish();
  if (st == LVA_ERR_HIP) g_rs_error = lva_last_hip_error();
  return st;
}

}  // namespace

extern "C" {

const char* lva_rs_last_error(void) { return g_rs_error.c_str(); }

int lva_rs_decode(int32_t device, const uint16_t* symbols, int32_t n_codewords, int32_t n_total, int32_t redundancy,
                  const int32_t* erasures, int32_t n_erasures, uint16_t pad_symbol, uint16_t fail_symbol, uint16_t* out,
                  int32_t* ok) {
  if (!rs_shape_ok(n_codewords, n_total, redundancy)) return LVA_ERR_ARG;
  if (n_erasures < 0 || (n_codewords > 0 && (!symbols || !out)) || (n_erasures > 0 && !erasures)) return LVA_ERR_ARG;
  std::vector<uint8_t> seen((size_t)n_total, 0);             // "erasure positions must be unique and inside the block" (:213-218)
  for (int i = 0; i < n_erasures; ++i) {
    if (erasures[i] < 0 || erasures[i] >= n_total || seen[(size_t)erasures[i]]) return LVA_ERR_ARG;
    seen[(size_t)erasures[i]] = 1;
  }
  if (n_codewords == 0) return LVA_OK;
  return rs_run(device, symbols, n_codewords, n_total, redundancy, erasures, n_erasures, pad_symbol, fail_symbol, out,
                n_total - redundancy, ok);
}

int lva_rs_encode(int32_t device, const uint16_t* data, int32_t n_codewords, int32_t n_data, int32_t redundancy,
                  uint16_t pad_symbol, uint16_t* out) {
  if (n_data < 1) return LVA_ERR_ARG;
  const int n_total = n_data + redundancy;
  if (!rs_shape_ok(n_codewords, n_total, redundancy)) return LVA_ERR_ARG;
  if (n_codewords > 0 && (!data || !out)) return LVA_ERR_ARG;
  if (n_codewords == 0) return LVA_OK;
  // systematic encoding = filling in the parity symbols as erasures: the unique codeword with these data symbols
  std::vector<uint16_t> rx((size_t)n_codewords * n_total, 0);
  for (int c = 0; c < n_codewords; ++c) std::memcpy(&rx[(size_t)c * n_total], data + (size_t)c * n_data, (size_t)n_data * 2);
  std::vector<int32_t> er((size_t)redundancy), ok((size_t)n_codewords, 0);
  for (int i = 0; i < redundancy; ++i) er[(size_t)i] = n_data + i;
  const int rc = rs_run(device, rx.data(), n_codewords, n_total, redundancy, er.data(), redundancy, pad_symbol, 0, out, n_total, ok.data());
  if (rc != LVA_OK) return rc;
  for (int c = 0; c < n_codewords; ++c)
    if (!ok[(size_t)c]) { g_rs_error = "encode: the erasure decode of the parity symbols failed"; return LVA_ERR_HIP; }
  return LVA_OK;
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
  std::vector<uint16_t> gexp, glog, truth(s * nd, 0);    // (these outlive the call's frame)
  tr_gf_tables(&gexp, &glog);
  for (size_t c = 0; c < s; ++c)                         // column c of the original file, as the decoder's output is laid out
    for (size_t j = 0; j < nd; ++j) {
      const int64_t at = (int64_t)(j * bpo + 2 * c);
      const uint32_t lo = at < original_bytes ? original[at] : 0u, hi = at + 1 < original_bytes ? original[at + 1] : 0u;
      truth[c * nd + j] = (uint16_t)(lo | (hi << 8));
    }
  Frame f;
  if (const int so = f.open(device)) return so;
  const auto d_index = f.in(index, n);
  const auto d_order = f.scratch<int32_t>(n);
  const auto d_pay = f.in(payload, n * bpo);
  const auto d_bucket = f.scratch<int32_t>(no + 1);
  const auto d_gexp = f.in(gexp.data(), kTrGexpWords), d_glog = f.in(glog.data(), kTrGlogWords), d_truth = f.in(truth.data(), s * nd);
  const auto d_stats = f.out(out_stats, 4 * K * T);
  const auto d_place = f.scratch<int32_t>(chunk * n), d_cnt = f.scratch<int32_t>(chunk * n);
  const auto d_nmem = f.scratch<int32_t>(K * chunk * no), d_erl = f.scratch<int32_t>(K * chunk * no);
  const auto d_ern = f.scratch<int32_t>(K * chunk), d_pp = f.scratch<int32_t>(2 * K * chunk), d_okeq = f.scratch<int32_t>(2 * K * chunk * s);
  const auto d_sym = f.scratch<uint16_t>(K * chunk * s * no), d_dec = f.scratch<uint16_t>(K * chunk * s * nd);
  const auto d_cons = out_payload ? f.scratch<uint8_t>(K * chunk * no * bpo) : Piece<uint8_t>{};     // copied out chunk by chunk, below
  const auto d_pres = out_present ? f.scratch<uint8_t>(K * chunk * no) : Piece<uint8_t>{};
  int st = f.begin();
  if (st != LVA_OK) return st;
  int e = launch_ls_bucket_scan(d_index, n_reads, num_oligos, d_bucket, f.stream());
  if (!e) e = launch_tr_bucket_list(d_index, n_reads, num_oligos, d_bucket, d_order, f.stream());
  if (e) return launch_status(e);
  for (size_t at = 0; at < T; at += chunk) {             // a trial depends on (seed, trial number) alone: chunks change nothing
    const size_t c = std::min(chunk, T - at);
    sh.chunk = (int32_t)c;
    sh.first_trial = first_trial + (uint32_t)at;
    e = launch_tr_consensus(sh, d_bucket, d_order, d_pay, d_place, d_cnt, d_nmem, d_sym, d_cons, f.stream());
    if (!e) e = launch_tr_erasures(sh, d_nmem, d_erl, d_ern, d_pp, d_pres, f.stream());
    if (!e) e = launch_tr_decode(sh, d_sym, d_erl, d_ern, d_gexp, d_glog, d_dec, d_truth, original_bytes, d_okeq, f.stream());
    if (!e) e = launch_tr_fold(sh, d_okeq, d_pp, d_stats, n_trials, (int32_t)at, f.stream());
    if (e) return launch_status(e);
    for (size_t k = 0; k < K; ++k) {                     // the chunk holds [point][trial of the chunk], the caller [point][trial]
      if (out_present && (st = f.download(out_present + (k * T + at) * no, d_pres, k * c * no, c * no)) != LVA_OK) return st;
      if (out_payload && (st = f.download(out_payload + (k * T + at) * no * bpo, d_cons, k * c * no * bpo, c * no * bpo)) != LVA_OK)
        return st;
    }
  }
  return f.finish();
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
  Piece<uint16_t> posinfo;
  Piece<uint32_t> cdf;
  Piece<uint8_t> bc;
  Piece<uint8_t> pool;             // with a pool only: its messages, its table if it has one, and per read what was drawn
  Piece<uint32_t> pool_cdf;
  Piece<int32_t> source;
  Piece<uint8_t> rc;
  uint32_t n_pool;
  SimPool dev() const {            // the pool as the kernel takes it, once the frame has begun
    SimPool p;
    p.msgs = pool; p.cdf = pool_cdf; p.n = n_pool; p.source = source; p.rc = rc;
    return p;
  }
};
// c, dwell_cdf and the pool are declared before the frame; source_out, rc_out: what was drawn, to the caller (null: not wanted)
SimTables sim_tables(Frame& f, const SimCall& c, const uint32_t* dwell_cdf, const SimPoolHost* pool, size_t n_reads,
                     int32_t* source_out, uint8_t* rc_out) {
  SimTables t{f.in(c.posinfo.data(), c.posinfo.size()), f.in(dwell_cdf, c.p.dwell_k), f.in(c.bc, sizeof c.bc), {}, {}, {}, {}, 0};
  if (pool) {
    t.pool = f.in(pool->msgs, (size_t)pool->n * c.p.msg_len);
    if (pool->cdf) t.pool_cdf = f.in(pool->cdf, (size_t)pool->n);
    t.source = f.out(source_out, n_reads);
    t.rc = f.out(rc_out, n_reads);
    t.n_pool = (uint32_t)pool->n;
  }
  return t;
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
  Frame f(d->stream);
  const SimTables tab = sim_tables(f, c, dwell_cdf, pool, n, nullptr, nullptr);
  const auto d_lens = f.out(lens.data(), 2 * n);
  if ((st = f.begin()) != LVA_OK) return st;
  const SimPool dpool = tab.dev();
  const int e = launch_sim_strand(c.p, pool ? &dpool : nullptr, n_reads, tab.posinfo, tab.cdf, tab.bc, nullptr, nullptr, d_lens, nullptr,
                                  nullptr, nullptr, nullptr, f.stream());
  if (e) return launch_status(e);
  if ((st = f.finish()) != LVA_OK) return st;
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
  Frame f(d->stream);
  const SimTables tab = sim_tables(f, c, dwell_cdf, pool, n, source_out, rc_out);
  const auto d_row = f.in(row_offsets, n + 1), d_base = f.in(base_offsets, n + 1);
  const auto d_msgs = f.out(msgs_out, mb), d_bases = f.out(bases_out, B), d_tidx = f.out(true_idx_out, T);
  const auto d_bad = f.inout(&bad, &bad, 1);             // goes up as 0, comes back as what the strand kernel found
  if ((st = f.begin()) != LVA_OK) return st;
  const SimPool dpool = tab.dev();
  int e = launch_sim_strand(c.p, pool ? &dpool : nullptr, n_reads, tab.posinfo, tab.cdf, tab.bc, d_row, d_base, nullptr, d_msgs, d_bases,
                            d_tidx, d_bad, f.stream());
  if (e) return launch_status(e);
  HIP_TRY(hipEventRecord(d->ev_total0, d->stream));
  e = launch_sim_scores(c.p, n_reads, d_row, (uint32_t)T, d_tidx, scale, margin, clip, scores_dev, f.stream());
  if (e) return launch_status(e);
  HIP_TRY(hipEventRecord(d->ev_total1, d->stream));
  if ((st = f.finish()) != LVA_OK) return st;
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

// ---------------------------------------------------------------------------------------------
// the error profile of a set of reads (csrc/ep_kernels.hip; the definition is
// error_profile.py).  Like the list consumers: a device ordinal, a stream of its own, complete on return.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr size_t kEpChunkBytes = (size_t)1 << 30;        // what the move codes of a chunk of reads may occupy on the device

// everything lva_align_profile can refuse without the device
int profile_args(const uint8_t* bases, const int64_t* first_base, const int32_t* n_bases, int32_t n_reads, const uint8_t* refs,
                 int32_t n_refs, int32_t ref_len, const int32_t* ref_id, int32_t chunk_reads) {
  if (n_reads < 0 || chunk_reads < 0 || !refs) return LVA_ERR_ARG;
  if (ref_len < 1 || ref_len > kMaxRef || n_refs < 1 || (uint64_t)n_refs * (uint64_t)ref_len >= (1ull << 31)) return LVA_ERR_ARG;
  if (n_reads > 0 && (!bases || !first_base || !n_bases || !ref_id)) return LVA_ERR_ARG;
  for (int32_t i = 0; i < n_reads; ++i)
    if (ref_id[i] >= n_refs) return LVA_ERR_ARG;
  return Windows::check(first_base, n_bases, n_reads, kMaxRead);
}

}  // namespace

extern "C" {

int lva_align_profile(int32_t device, const uint8_t* bases, const int64_t* first_base, const int32_t* n_bases, int32_t n_reads,
                      const uint8_t* refs, int32_t n_refs, int32_t ref_len, const int32_t* ref_id, const uint8_t* rc,
                      int32_t chunk_reads, int32_t* out_read, int64_t* out_pos, int64_t* out_conf, int64_t* out_ins) {
  if (profile_args(bases, first_base, n_bases, n_reads, refs, n_refs, ref_len, ref_id, chunk_reads) != LVA_OK) return LVA_ERR_ARG;
  if (n_reads == 0) return LVA_OK;
  const size_t n = (size_t)n_reads, np = 4 * ((size_t)ref_len + 1);
  Windows w;                                             // (these outlive the call's frame)
  std::vector<uint8_t> flip;
  std::vector<int64_t> move_off, zero;
  Frame f;
  if (const int so = f.open(device)) return so;
  // a skipped read has no window: nothing of it is packed
  w.nb.resize(n);
  for (size_t i = 0; i < n; ++i) w.nb[i] = ref_id[i] < 0 ? 0 : n_bases[i];
  w.pack(f, bases, first_base, w.nb.data(), n);
  flip.assign(n, 0); move_off.resize(n);
  zero.assign(std::max<size_t>(np, 24), 0);
  // chunks: reads [cuts[k], cuts[k + 1]), as many as chunk_reads allows and as fit kEpChunkBytes (one read: at most 4.3 MB)
  std::vector<size_t> cuts{0};
  size_t in_chunk = 0, cap = 0;
  for (size_t i = 0; i < n; ++i) {
    if (rc && rc[i]) flip[i] = 1;
    const size_t mb = ep_move_bytes(ref_len, w.nb[i]);
    if (i > cuts.back() && (in_chunk + mb > kEpChunkBytes || (chunk_reads > 0 && i - cuts.back() >= (size_t)chunk_reads))) {
      cuts.push_back(i);
      in_chunk = 0;
    }
    move_off[i] = (int64_t)in_chunk;                     // from the start of the chunk's moves
    in_chunk += mb;
    cap = std::max(cap, in_chunk);
  }
  cuts.push_back(n);
  const auto d_id = f.in(ref_id, n);
  const auto d_flip = f.in(flip.data(), n);
  const auto d_moff = f.in(move_off.data(), n);
  const auto d_refs = f.in(refs, (size_t)n_refs * (size_t)ref_len);
  const auto d_moves = f.scratch<uint8_t>(cap);
  const auto d_read = f.out(out_read, 4 * n);
  const auto d_pos = f.inout(zero.data(), out_pos, np), d_conf = f.inout(zero.data(), out_conf, 24), d_ins = f.inout(zero.data(), out_ins, 5);
  if (const int st = f.begin()) return st;
  for (size_t k = 0; k + 1 < cuts.size(); ++k) {         // the tallies are sums over reads: chunks change nothing
    const size_t a = cuts[k];
    const int32_t c = (int32_t)(cuts[k + 1] - a);
    const Windows::Chunk x = w.from(a);
    int e = launch_ep_fill(x.bases, x.off, x.len, c, d_refs, ref_len, d_id.ptr() + a, d_flip.ptr() + a, d_moff.ptr() + a, d_moves,
                           f.stream());
    if (!e) e = launch_ep_walk(x.bases, x.off, x.len, c, d_refs, ref_len, d_id.ptr() + a, d_flip.ptr() + a, d_moff.ptr() + a, d_moves,
                               d_read.ptr() + 4 * a, d_pos, d_conf, d_ins, f.stream());
    if (e) return launch_status(e);
  }
  return f.finish();
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// reads mapped to oligos (csrc/mp_kernels.hip, csrc/mq_kernels.hip; the definition is
// read_map.py).  Both mapping entry points run one body, map_stage; which of them was called decides the kernels.  The index is built once and owned by the caller; a mapping call takes a device ordinal like the list
// consumers.  Built on the host (lva_map_index_create, lva_map_index_create_pooled) its tables are host vectors that every mapping
// call uploads; built on the device (lva_map_index_create_device, csrc/mi_kernels.hip) they are device memory of that ordinal until
// the index is destroyed, the same bytes, and a mapping call uploads the reads alone.
// ---------------------------------------------------------------------------------------------
struct lva_map_index {
  int32_t n_refs, ref_len, k, max_occ;   // ref_len: the longest oligo; every oligo's where ragged is not set
  bool ragged;                           // the oligos differ in length: lva_map_reads_pooled alone takes the index
  std::vector<int32_t> lens;             // [n_refs]
  std::vector<uint32_t> offsets;         // [4^k + 1]: the oligos of k-mer c are lists[offsets[c] .. offsets[c + 1])
  std::vector<int32_t> lists;            // ascending inside a k-mer
  std::vector<uint64_t> masks;           // mp_mask_words(n_refs, ref_len): per oligo, forward and reversed within its own length, per base, W words
  int64_t kmers, pairs, dropped;         // kept distinct k-mers, kept pairs, k-mers that max_occ dropped
  // built on the device: its ordinal (-1: built on the host, the vectors above hold the tables) and the tables there, the
  // vectors' layouts; d_tables is one allocation (offsets, masks, lens), d_lists its own: its size is known after the scan
  int32_t device = -1;
  char* d_tables = nullptr;
  uint32_t* d_offsets = nullptr;
  uint64_t* d_masks = nullptr;
  int32_t* d_lens = nullptr;
  int32_t* d_lists = nullptr;
  ~lva_map_index() {                     // hipFree finds the owning device from the pointer: the caller's current device stays
    if (d_lists) (void)hipFree(d_lists);
    if (d_tables) (void)hipFree(d_tables);
  }
};

namespace {

constexpr size_t kMpChunkBytes = (size_t)1 << 30;        // what the candidate lists of a chunk of reads may occupy on the device

// everything both mapping entry points can refuse without the device; the threshold and the flanks are each entry's own
int map_args(const lva_map_index* idx, const uint8_t* bases, const int64_t* first_base, const int32_t* n_bases, int32_t n_reads,
             int32_t cands, int32_t min_votes, int32_t chunk_reads, const int32_t* out) {
  if (!idx || n_reads < 0 || chunk_reads < 0 || cands < 1 || cands > kMpMaxCands || min_votes < 1) return LVA_ERR_ARG;
  if (n_reads > 0 && (!bases || !first_base || !n_bases || !out)) return LVA_ERR_ARG;
  return Windows::check(first_base, n_bases, n_reads, kMaxRead);
}

// what both builders know before they build: the parameters and the oligos' lengths (may throw bad_alloc)
void index_shape(lva_map_index* x, const int64_t* ref_off, int32_t n_refs, int32_t k, int32_t max_occ) {
  x->n_refs = n_refs; x->k = k; x->max_occ = max_occ;
  x->lens = read_lengths(ref_off, n_refs);
  x->ref_len = *std::max_element(x->lens.begin(), x->lens.end());
  x->ragged = *std::min_element(x->lens.begin(), x->lens.end()) != x->ref_len;
}

// everything the three index entry points can refuse from the offsets
int index_offsets_args(const int64_t* ref_off, int32_t n_refs) {
  size_t total;
  if (check_offsets(ref_off, n_refs, &total) != LVA_OK) return LVA_ERR_ARG;
  for (int32_t o = 0; o < n_refs; ++o)
    if (ref_off[o + 1] - ref_off[o] < 1 || ref_off[o + 1] - ref_off[o] > kMaxRef) return LVA_ERR_ARG;
  return LVA_OK;
}

// THE host index builder: oligo o is refs[ref_off[o] .. ref_off[o + 1]), its length in 1 .. kMaxRef (the callers have checked)
int build_map_index(const uint8_t* refs, const int64_t* ref_off, int32_t n_refs, int32_t k, int32_t max_occ, lva_map_index** out) {
  lva_map_index* x = new (std::nothrow) lva_map_index{};
  if (!x) return LVA_ERR_NOMEM;
  try {
    index_shape(x, ref_off, n_refs, k, max_occ);
    const size_t W = ((size_t)x->ref_len + 63) / 64, table = (size_t)1 << (2 * k);
    // the distinct pairs (k-mer, oligo), k-mer major
    std::vector<uint64_t> pairs;
    const uint32_t mask = (uint32_t)(table - 1);
    x->masks.assign(mp_mask_words(n_refs, x->ref_len), 0);
    for (int32_t o = 0; o < n_refs; ++o) {
      const uint8_t* ref = refs + ref_off[o];
      const size_t m = (size_t)x->lens[o];
      uint32_t code = 0;
      int run = 0;
      for (size_t i = 0; i < m; ++i) {
        const uint32_t c = base_code(ref[i]);
        if (c < kBaseN) {
          code = ((code << 2) | c) & mask;
          ++run;
          x->masks[(((size_t)o * 2 + 0) * 4 + c) * W + (i >> 6)] |= 1ull << (i & 63);
          x->masks[(((size_t)o * 2 + 1) * 4 + c) * W + ((m - 1 - i) >> 6)] |= 1ull << ((m - 1 - i) & 63);
        } else {
          run = 0;
        }
        if (run >= k) pairs.push_back(((uint64_t)code << 32) | (uint32_t)o);
      }
    }
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    x->offsets.assign(table + 1, 0);
    x->lists.reserve(pairs.size());
    size_t at = 0;
    for (size_t c = 0; c < table; ++c) {
      x->offsets[c] = (uint32_t)x->lists.size();
      size_t end = at;
      while (end < pairs.size() && (pairs[end] >> 32) == c) ++end;
      if (end > at) {
        if (end - at > (size_t)max_occ) {
          ++x->dropped;                  // shared too widely to say anything: it votes for nobody
        } else {
          ++x->kmers;
          for (size_t p = at; p < end; ++p) x->lists.push_back((int32_t)(pairs[p] & 0xFFFFFFFFu));
        }
      }
      at = end;
    }
    x->offsets[table] = (uint32_t)x->lists.size();
    x->pairs = (int64_t)x->lists.size();
  } catch (const std::bad_alloc&) {
    delete x;
    return LVA_ERR_NOMEM;
  }
  *out = x;
  return LVA_OK;
}

// The same index from the same arguments, built on the device and left there (csrc/mi_kernels.h lists the steps).  Two
// frames: the first holds the oligos and the counters and ends with the three counts on the host, which size the lists;
// the second holds the unordered slots and is made only where there are pairs.  x is declared first: the frames drain
// before its device memory can be freed.
int build_map_index_device(int32_t device, const uint8_t* refs, const int64_t* ref_off, int32_t n_refs, int32_t k, int32_t max_occ,
                           lva_map_index** out) {
  struct Owner {
    lva_map_index* x;
    ~Owner() { delete x; }
  } own{new (std::nothrow) lva_map_index{}};
  lva_map_index* x = own.x;
  if (!x) return LVA_ERR_NOMEM;
  const uint32_t zero[4] = {0, 0, 0, 0};
  uint32_t stats[4] = {0, 0, 0, 0};                    // kept k-mers, dropped k-mers, pairs
  try {
    index_shape(x, ref_off, n_refs, k, max_occ);
  } catch (const std::bad_alloc&) {
    return LVA_ERR_NOMEM;
  }
  const size_t table = mi_table(k), nr = (size_t)n_refs, words = mp_mask_words(n_refs, x->ref_len);
  const bool any = x->ref_len >= k;                    // else no oligo holds a k-mer: the table is all zero
  Frame f;
  if (const int so = f.open(device)) return so;
  x->device = device;
  const auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
  const size_t at_masks = pad((table + 1) * sizeof(uint32_t)), at_lens = at_masks + pad(words * sizeof(uint64_t));
  if (hipMalloc(reinterpret_cast<void**>(&x->d_tables), at_lens + pad(nr * sizeof(int32_t))) != hipSuccess) return LVA_ERR_NOMEM;
  x->d_offsets = reinterpret_cast<uint32_t*>(x->d_tables);
  x->d_masks = reinterpret_cast<uint64_t*>(x->d_tables + at_masks);
  x->d_lens = reinterpret_cast<int32_t*>(x->d_tables + at_lens);
  const auto d_refs = f.in(refs, (size_t)ref_off[n_refs]);
  const auto d_ref_off = f.in(ref_off, nr + 1);
  const auto d_counts = f.scratch<uint32_t>(any ? table : 0);
  const auto d_sums = f.scratch<uint32_t>(any ? mi_scan_tiles(k) : 0);
  const auto d_stats = f.inout(zero, stats, 4);
  if (const int st = f.begin()) return st;
  if (const int st = f.copy(x->d_lens, x->lens.data(), nr * sizeof(int32_t), hipMemcpyHostToDevice)) return st;
  int e = launch_mi_masks(d_refs, d_ref_off, n_refs, x->ref_len, x->d_masks, f.stream());
  if (!e && any) {
    HIP_TRY(hipMemsetAsync(d_counts.ptr(), 0, table * sizeof(uint32_t), f.stream()));
    e = launch_mi_count(d_refs, d_ref_off, n_refs, k, d_counts, f.stream());
    if (!e) e = launch_mi_clip(d_counts, k, max_occ, d_stats, f.stream());
    if (!e) e = launch_mi_scan(d_counts, k, d_sums, x->d_offsets, d_stats, f.stream());
  } else if (!e) {
    HIP_TRY(hipMemsetAsync(x->d_offsets, 0, (table + 1) * sizeof(uint32_t), f.stream()));
  }
  if (e) return launch_status(e);
  if (const int st = f.finish()) return st;
  x->kmers = stats[0]; x->dropped = stats[1]; x->pairs = stats[2];
  const size_t pairs = (size_t)stats[2];
  if (hipMalloc(reinterpret_cast<void**>(&x->d_lists), std::max<size_t>(pairs, 1) * sizeof(int32_t)) != hipSuccess) return LVA_ERR_NOMEM;
  if (pairs) {
    Frame g;
    if (const int so = g.open(device)) return so;
    const auto d_slot_oligo = g.scratch<int32_t>(pairs);
    const auto d_slot_kmer = g.scratch<uint32_t>(pairs);
    if (const int st = g.begin()) return st;
    e = launch_mi_fill(d_refs, d_ref_off, n_refs, k, x->d_offsets, d_counts, d_slot_oligo, d_slot_kmer, g.stream());
    if (!e) e = launch_mi_rank(d_slot_oligo, d_slot_kmer, (uint32_t)pairs, k, x->d_offsets, x->d_lists, g.stream());
    if (e) return launch_status(e);
    if (const int st = g.finish()) return st;
  }
  own.x = nullptr;
  *out = x;
  return LVA_OK;
}

// the tables of an index where a mapping call's frame can read them: uploaded with the call, or resident since the build
struct IndexTables {
  Piece<uint32_t> offsets;
  Piece<int32_t> lists;
  Piece<uint64_t> masks;
  Piece<int32_t> lens;
  IndexTables(Frame& f, const lva_map_index* idx, bool with_lens) {
    const size_t nr = (size_t)idx->n_refs;
    if (idx->device >= 0) {
      offsets = f.resident(idx->d_offsets, mi_table(idx->k) + 1);
      lists = f.resident(idx->d_lists, (size_t)idx->pairs);
      masks = f.resident(idx->d_masks, mp_mask_words(idx->n_refs, idx->ref_len));
      if (with_lens) lens = f.resident(idx->d_lens, nr);
    } else {
      offsets = f.in(idx->offsets.data(), idx->offsets.size());
      lists = f.in(idx->lists.data(), idx->lists.size());
      masks = f.in(idx->masks.data(), idx->masks.size());
      if (with_lens) lens = f.in(idx->lens.data(), nr);
    }
  }
};

// THE mapping call behind both entry points, which have checked their arguments: vote, distance and start per chunk of
// reads, and for min_flank > 0 (the pooled entry alone) the same over the longer flank of every mapped read, into supp.
// pooled: lva_map_reads_pooled called (the mq launchers, max_dist [n_refs], whatever the index); else lva_map_reads (the mp
// launchers, max_dist [1] for every oligo of one length, no lens and no thresholds uploaded).
int map_stage(int32_t device, const lva_map_index* idx, const uint8_t* bases, const int64_t* first_base, const int32_t* n_bases,
              int32_t n_reads, int32_t cands, int32_t min_votes, bool pooled, const int32_t* max_dist, int32_t min_flank,
              int32_t chunk_reads, int32_t* out, int32_t* supp) {
  if (idx->device >= 0 && idx->device != device) return LVA_ERR_ARG;       // the tables live on another device
  if (n_reads == 0) return LVA_OK;
  const size_t n = (size_t)n_reads;
  const bool flanks = min_flank > 0;
  Windows w;                                             // (outlives the call's frame)
  Frame f;
  if (const int so = f.open(device)) return so;
  w.pack(f, bases, first_base, n_bases, n);              // every read, as given
  size_t chunk = std::min(n, kMpChunkBytes / (kMpMaxCands * sizeof(uint64_t)));
  if (chunk_reads > 0) chunk = std::min(chunk, (size_t)chunk_reads);
  const IndexTables t(f, idx, pooled);
  const auto d_max = pooled ? f.in(max_dist, (size_t)idx->n_refs) : Piece<int32_t>{};
  const auto d_cand = f.scratch<uint64_t>(chunk * kMpMaxCands);
  const auto d_out = f.out(out, 8 * n);
  // the supplementary pass: per read of a chunk its flank as a window (offset, length) and the flank's place in the read's window
  const auto d_supp = flanks ? f.out(supp, 8 * n) : Piece<int32_t>{};
  Piece<int32_t> d_foff, d_flen, d_fshift;
  if (pooled) {                                          // (empty without flanks)
    d_foff = f.scratch<int32_t>(flanks ? chunk : 0);
    d_flen = f.scratch<int32_t>(flanks ? chunk : 0);
    d_fshift = f.scratch<int32_t>(flanks ? chunk : 0);
  }
  if (const int st = f.begin()) return st;
  for (size_t a = 0; a < n; a += chunk) {                // a read's rows depend on the read alone: chunks change nothing
    const int32_t c = (int32_t)std::min(chunk, n - a);
    const Windows::Chunk x = w.from(a);
    // the windows (off, len) of the chunk mapped into rows; shift: what a window's start adds to the start it reports
    const auto map_windows = [&](const int32_t* off, const int32_t* len, const int32_t* shift, int32_t* rows) {
      int e = launch_mp_vote(x.bases, off, len, c, t.offsets, t.lists, idx->k, idx->n_refs, min_votes, cands, d_cand, f.stream());
      if (pooled) {
        if (!e) e = launch_mq_verify(x.bases, off, len, c, d_cand, t.masks, t.lens, idx->ref_len, cands, d_max, rows, f.stream());
        if (!e) e = launch_mq_start(x.bases, off, len, c, t.masks, t.lens, idx->ref_len, shift, rows, f.stream());
      } else {
        if (!e) e = launch_mp_verify(x.bases, off, len, c, d_cand, t.masks, idx->ref_len, cands, max_dist[0], rows, f.stream());
        if (!e) e = launch_mp_start(x.bases, off, len, c, t.masks, idx->ref_len, rows, f.stream());
      }
      return e;
    };
    int e = map_windows(x.off, x.len, nullptr, d_out.ptr() + 8 * a);
    if (!e && flanks) {
      e = launch_mq_flank(x.off, x.len, c, d_out.ptr() + 8 * a, min_flank, d_foff, d_flen, d_fshift, f.stream());
      if (!e) e = map_windows(d_foff, d_flen, d_fshift, d_supp.ptr() + 8 * a);
    }
    if (e) return launch_status(e);
  }
  return f.finish();
}

}  // namespace

extern "C" {

int lva_map_index_create_device(int32_t device, const uint8_t* refs, const int64_t* ref_off, int32_t n_refs, int32_t k, int32_t max_occ,
                                lva_map_index** out) {
  if (!refs || !ref_off || !out || n_refs < 1 || k < kMpMinK || k > kMpMaxK || max_occ < 1 || max_occ > 65535) return LVA_ERR_ARG;
  if (index_offsets_args(ref_off, n_refs) != LVA_OK) return LVA_ERR_ARG;
  return build_map_index_device(device, refs, ref_off, n_refs, k, max_occ, out);
}

int lva_map_index_tables(const lva_map_index* idx, uint32_t* offsets, int32_t* lists, uint64_t* masks) {
  if (!idx) return LVA_ERR_ARG;
  const size_t n_off = mi_table(idx->k) + 1, n_lists = (size_t)idx->pairs, n_masks = mp_mask_words(idx->n_refs, idx->ref_len);
  if (idx->device < 0) {
    if (offsets) std::memcpy(offsets, idx->offsets.data(), n_off * sizeof(uint32_t));
    if (lists && n_lists) std::memcpy(lists, idx->lists.data(), n_lists * sizeof(int32_t));
    if (masks) std::memcpy(masks, idx->masks.data(), n_masks * sizeof(uint64_t));
    return LVA_OK;
  }
  if (hipSetDevice(idx->device) != hipSuccess) return LVA_ERR_NO_DEVICE;   // the tables' device, like every call that works on one
  if (offsets) HIP_TRY(hipMemcpy(offsets, idx->d_offsets, n_off * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (lists && n_lists) HIP_TRY(hipMemcpy(lists, idx->d_lists, n_lists * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (masks) HIP_TRY(hipMemcpy(masks, idx->d_masks, n_masks * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return LVA_OK;
}

int lva_map_index_create(const uint8_t* refs, int32_t n_refs, int32_t ref_len, int32_t k, int32_t max_occ, lva_map_index** out) {
  if (!refs || !out || n_refs < 1 || ref_len < 1 || ref_len > kMaxRef || k < kMpMinK || k > kMpMaxK) return LVA_ERR_ARG;
  if (max_occ < 1 || max_occ > 65535 || (uint64_t)n_refs * (uint64_t)ref_len >= (1ull << 31)) return LVA_ERR_ARG;
  try {                                  // the equal-length case of the pooled index
    std::vector<int64_t> ref_off((size_t)n_refs + 1);
    for (int32_t o = 0; o <= n_refs; ++o) ref_off[o] = (int64_t)o * ref_len;
    return build_map_index(refs, ref_off.data(), n_refs, k, max_occ, out);
  } catch (const std::bad_alloc&) {
    return LVA_ERR_NOMEM;
  }
}

int lva_map_index_create_pooled(const uint8_t* refs, const int64_t* ref_off, int32_t n_refs, int32_t k, int32_t max_occ,
                                lva_map_index** out) {
  if (!refs || !ref_off || !out || n_refs < 1 || k < kMpMinK || k > kMpMaxK || max_occ < 1 || max_occ > 65535) return LVA_ERR_ARG;
  if (index_offsets_args(ref_off, n_refs) != LVA_OK) return LVA_ERR_ARG;
  return build_map_index(refs, ref_off, n_refs, k, max_occ, out);
}

void lva_map_index_destroy(lva_map_index* idx) { delete idx; }

int lva_map_index_info(const lva_map_index* idx, int64_t* kmers, int64_t* pairs, int64_t* dropped_kmers) {
  if (!idx) return LVA_ERR_ARG;
  if (kmers) *kmers = idx->kmers;
  if (pairs) *pairs = idx->pairs;
  if (dropped_kmers) *dropped_kmers = idx->dropped;
  return LVA_OK;
}

int lva_map_reads(int32_t device, const lva_map_index* idx, const uint8_t* bases, const int64_t* first_base, const int32_t* n_bases,
                  int32_t n_reads, int32_t cands, int32_t min_votes, int32_t max_dist, int32_t chunk_reads, int32_t* out) {
  if (map_args(idx, bases, first_base, n_bases, n_reads, cands, min_votes, chunk_reads, out) != LVA_OK || max_dist < 0) return LVA_ERR_ARG;
  if (idx->ragged) return LVA_ERR_ARG;                    // one ref_len for all: lva_map_reads_pooled takes the others
  return map_stage(device, idx, bases, first_base, n_bases, n_reads, cands, min_votes, false, &max_dist, 0, chunk_reads, out, nullptr);
}

int lva_map_reads_pooled(int32_t device, const lva_map_index* idx, const uint8_t* bases, const int64_t* first_base, const int32_t* n_bases,
                         int32_t n_reads, int32_t cands, int32_t min_votes, const int32_t* max_dist, int32_t min_flank,
                         int32_t chunk_reads, int32_t* out, int32_t* supp) {
  if (map_args(idx, bases, first_base, n_bases, n_reads, cands, min_votes, chunk_reads, out) != LVA_OK) return LVA_ERR_ARG;
  if (!max_dist || min_flank < 0 || (n_reads > 0 && min_flank > 0 && !supp)) return LVA_ERR_ARG;
  for (int32_t o = 0; o < idx->n_refs; ++o)
    if (max_dist[o] < 0) return LVA_ERR_ARG;
  return map_stage(device, idx, bases, first_base, n_bases, n_reads, cands, min_votes, true, max_dist, min_flank, chunk_reads, out, supp);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// what a given base sequence scores on a read -- the reference trellis restricted to one
// message (csrc/sc_kernels.hip; the definition is trellis_score.py).  Bound to a decoder: its stream, its max_deviation
// by default, posteriors where the decode calls read them.  The code's npos does not constrain a sequence; the band of a
// pair is the band formula's for (the read's blocks, the sequence's positions), evaluated on the host as the decode
// path evaluates its own (band_of, lva_code.cpp) and shared by the pairs that agree in both.
// ---------------------------------------------------------------------------------------------
namespace {

// Band words of one call at most (256 MiB on the host and on the device): one table per distinct (blocks, positions) among
// the pairs.  A run of 2 000 reads scored against its own lists needs 2 M words; 2^26 is 64 reads of 2^20 blocks each.
constexpr size_t kScMaxBandWords = (size_t)1 << 26;

// everything that can be refused without the device, in the order of include/lva_decoder.h
int score_args(const int64_t* first_block, const int64_t* n_blocks, int32_t n_reads, const uint8_t* bases, const int64_t* first_base,
               const int32_t* n_bases, int32_t n_seqs, const int32_t* pairs, int32_t n_pairs, const float* post, const float* out) {
  if (n_reads < 0 || n_seqs < 0 || n_pairs < 0) return LVA_ERR_ARG;
  if (n_reads > 0 && (!post || !first_block || !n_blocks)) return LVA_ERR_ARG;
  if (n_seqs > 0 && (!bases || !first_base || !n_bases)) return LVA_ERR_ARG;
  if (n_pairs > 0 && (!pairs || !out)) return LVA_ERR_ARG;
  for (int32_t i = 0; i < n_reads; ++i)                  // 32-bit block offsets inside the kernel, as everywhere
    if (first_block[i] < 0 || n_blocks[i] < 0 || n_blocks[i] > kBcMaxBlocks || first_block[i] + n_blocks[i] >= ((int64_t)1 << 31))
      return LVA_ERR_ARG;
  if (Windows::check(first_base, n_bases, n_seqs, kMaxRef) != LVA_OK) return LVA_ERR_ARG;        // a sequence longer than kMaxRef
  for (int32_t s = 0; s < n_seqs; ++s) {
    if (n_bases[s] < 1) return LVA_ERR_ARG;
    for (int32_t j = 0; j < n_bases[s]; ++j)
      if (base_code(bases[first_base[s] + j]) >= kBaseN) return LVA_ERR_ARG;                      // a base code above 3
  }
  for (int32_t k = 0; k < n_pairs; ++k)
    if (pairs[2 * k] < 0 || pairs[2 * k] >= n_reads || pairs[2 * k + 1] < 0 || pairs[2 * k + 1] >= n_seqs) return LVA_ERR_ARG;
  for (int32_t k = 0; k < n_pairs; ++k)                  // nblk < npos + 1: "Too small post matrix" (:600-601)
    if (n_blocks[pairs[2 * k]] < (int64_t)n_bases[pairs[2 * k + 1]] + 2) return LVA_ERR_POST_TOO_SHORT;
  return LVA_OK;
}

// What a trace asks for beside the scores (lva_trace_bases*); a score call has none
struct TraceOut {
  int32_t end;                 // 0 flip, 1 flop, -1 the larger
  uint64_t scratch_limit;      // bytes of back-pointers on the device at a time; 0: kStScratchDefault
  int32_t stride;
  int32_t* enter;
  uint8_t* kind;
  int32_t* info;
};
constexpr uint64_t kStScratchDefault = (uint64_t)1 << 30;

// back-pointer bytes of one pair: [nblk][min(2 * max_deviation, positions)], padded to the 16 bytes a pair's rows start at
uint32_t trace_width(uint32_t max_dev, int32_t n_bases) { return (uint32_t)std::min<uint64_t>(2 * (uint64_t)max_dev, (uint64_t)n_bases + 1); }
uint64_t trace_bytes(uint32_t max_dev, int64_t nblk, int32_t n_bases) {
  return ((uint64_t)nblk * trace_width(max_dev, n_bases) + 15) & ~(uint64_t)15;
}

// which of the three answers of the one-message trellis a call asks for
enum class ScoreKind { kScore, kForward, kTrace };

// lva_score_bases (post on the host, read i = blocks [first_block[i], + n_blocks[i]) of it, T blocks in all: uploaded) and
// lva_score_bases_device (post the caller's device buffer); kForward, lva_forward_bases*: the same pairs, band tables, frame
// and refusals, fw_forward in place of sc_score; kTrace (with tr), lva_trace_bases and lva_trace_bases_device: the same
// pairs and band tables, st_fill and st_walk in place of sc_score, chunk by chunk of what the back-pointers may occupy
int score_stage(lva_decoder* d, const float* post, size_t host_blocks, bool post_on_host, const int64_t* first_block,
                const int64_t* n_blocks, int32_t n_reads, const uint8_t* bases, const int64_t* first_base, const int32_t* n_bases,
                int32_t n_seqs, const int32_t* pairs, int32_t n_pairs, uint32_t max_deviation, float* out,
                ScoreKind kind = ScoreKind::kScore, const TraceOut* tr = nullptr) {
  if (!d || (kind == ScoreKind::kTrace) != (tr != nullptr)) return LVA_ERR_ARG;
  int st = score_args(first_block, n_blocks, n_reads, bases, first_base, n_bases, n_seqs, pairs, n_pairs, post, out);
  if (st != LVA_OK) return st;
  const uint32_t max_dev = max_deviation == LVA_MAX_DEVIATION_DEFAULT ? d->max_dev : max_deviation;
  if (tr) {                                              // the trace's own refusals, after the score's
    const uint64_t limit = tr->scratch_limit ? tr->scratch_limit : kStScratchDefault;
    if (tr->end < -1 || tr->end > 1 || tr->stride < 0) return LVA_ERR_ARG;
    if (n_pairs > 0 && (!tr->enter || !tr->kind || !tr->info)) return LVA_ERR_ARG;
    for (int32_t k = 0; k < n_pairs; ++k) {
      if (n_bases[pairs[2 * k + 1]] > tr->stride) return LVA_ERR_ARG;
      if (trace_bytes(max_dev, n_blocks[pairs[2 * k]], n_bases[pairs[2 * k + 1]]) > limit) return LVA_ERR_ARG;   // one pair alone
    }
  }
  st = stage_enter(d, n_pairs == 0);
  if (st != kRun) return st;
  // the pairs as the kernel reads them; one band table per (blocks, positions) that occurs
  Windows w;                                             // (these outlive the call's frame)
  std::vector<ScPair> sp((size_t)n_pairs);
  std::vector<uint32_t> band;
  std::vector<std::pair<uint64_t, uint32_t>> keys((size_t)n_pairs);          // (blocks << 32 | positions, pair)
  int32_t max_len = 1;
  for (int32_t k = 0; k < n_pairs; ++k) {
    const int32_t r = pairs[2 * k], s = pairs[2 * k + 1];
    keys[k] = {(uint64_t)n_blocks[r] << 32 | (uint32_t)(n_bases[s] + 1), (uint32_t)k};
    max_len = std::max(max_len, n_bases[s]);
  }
  std::sort(keys.begin(), keys.end());
  size_t band_words = 0;                                 // refused before anything is allocated: kScMaxBandWords
  for (size_t i = 0; i < keys.size(); ++i)
    if (i == 0 || keys[i].first != keys[i - 1].first) band_words += (size_t)(keys[i].first >> 32);
  if (band_words > kScMaxBandWords) return LVA_ERR_ARG;
  band.reserve(band_words);
  // a trace: where each pair's back-pointers lie in its chunk's scratch, and the chunks, pairs [cuts[c], cuts[c + 1])
  std::vector<StBp> sb;
  std::vector<size_t> cuts;
  uint64_t scratch_bytes = 0;
  if (tr) {
    const uint64_t limit = tr->scratch_limit ? tr->scratch_limit : kStScratchDefault;
    sb.resize((size_t)n_pairs);
    cuts.push_back(0);
    uint64_t in_chunk = 0;
    for (int32_t k = 0; k < n_pairs; ++k) {
      const int32_t r = pairs[2 * k], s = pairs[2 * k + 1];
      const uint64_t need = trace_bytes(max_dev, n_blocks[r], n_bases[s]);
      if (in_chunk + need > limit) {                     // (need <= limit: checked above)
        cuts.push_back((size_t)k);
        in_chunk = 0;
      }
      sb[k] = StBp{in_chunk, trace_width(max_dev, n_bases[s]), 0};
      in_chunk += need;
      scratch_bytes = std::max(scratch_bytes, in_chunk);
    }
    cuts.push_back((size_t)n_pairs);
  }
  Frame f(d->stream);
  w.pack(f, bases, first_base, n_bases, (size_t)n_seqs);
  for (size_t i = 0; i < keys.size(); ++i) {
    const uint32_t k = keys[i].second, nblk = (uint32_t)(keys[i].first >> 32), npos = (uint32_t)keys[i].first;
    if (i == 0 || keys[i].first != keys[i - 1].first)
      for (uint32_t t = 0; t < nblk; ++t) {
        uint32_t lo, hi;
        band_of(npos, t, nblk, max_dev, &lo, &hi);
        band.push_back(lo | hi << 16);                   // hi <= npos <= kMaxRef + 1
      }
    sp[k] = ScPair{(uint32_t)first_block[pairs[2 * k]], nblk, (uint32_t)w.win_off[(size_t)pairs[2 * k + 1]], npos - 1,
                   (uint32_t)(band.size() - nblk)};
  }
  const Piece<float> up = post_on_host ? f.in(post, kPostRow * host_blocks) : Piece<float>{};
  const auto d_pairs = f.in(sp.data(), sp.size());
  const auto d_band = f.in(band.data(), band.size());
  const auto d_out = f.out(out, 2 * (size_t)n_pairs);
  if (!tr) {
    if ((st = f.begin()) != LVA_OK) return st;
    const auto launch = kind == ScoreKind::kForward ? launch_fw_forward : launch_sc_score;
    const int e = launch(post_on_host ? up.ptr() : post, w.bases, d_pairs, d_band, n_pairs, max_len, d_out, f.stream());
    if (e) return launch_status(e);
    return f.finish();
  }
  const size_t rows = (size_t)n_pairs * (size_t)tr->stride;
  const auto d_bp = f.in(sb.data(), sb.size());
  const auto d_enter = f.out(tr->enter, rows);
  const auto d_kind = f.out(tr->kind, rows);
  const auto d_info = f.out(tr->info, 4 * (size_t)n_pairs);
  const auto d_scratch = f.scratch<uint8_t>((size_t)scratch_bytes);
  if ((st = f.begin()) != LVA_OK) return st;
  const float* d_post = post_on_host ? up.ptr() : post;
  for (size_t c = 0; c + 1 < cuts.size(); ++c) {         // a pair's outputs depend on the pair alone: chunks change nothing
    const size_t a = cuts[c];
    const int32_t n = (int32_t)(cuts[c + 1] - a);
    int e = launch_st_fill(d_post, w.bases, d_pairs.ptr() + a, d_bp.ptr() + a, d_band, n, max_len, d_scratch, d_out.ptr() + 2 * a,
                           f.stream());
    if (!e) e = launch_st_walk(w.bases, d_pairs.ptr() + a, d_bp.ptr() + a, d_band, n, d_scratch, d_out.ptr() + 2 * a, tr->end, tr->stride,
                               d_enter.ptr() + a * (size_t)tr->stride, d_kind.ptr() + a * (size_t)tr->stride, d_info.ptr() + 4 * a,
                               f.stream());
    if (e) return launch_status(e);
  }
  return f.finish();
}

}  // namespace

extern "C" {

int lva_score_bases_device(lva_decoder* d, const float* post_dev, const int64_t* first_block, const int64_t* n_blocks, int32_t n_reads,
                           const uint8_t* bases, const int64_t* first_base, const int32_t* n_bases, int32_t n_seqs,
                           const int32_t* pairs, int32_t n_pairs, uint32_t max_deviation, float* out) {
  return score_stage(d, post_dev, 0, false, first_block, n_blocks, n_reads, bases, first_base, n_bases, n_seqs, pairs, n_pairs,
                     max_deviation, out);
}

int lva_score_bases(lva_decoder* d, const float* post, const int64_t* row_offsets, int32_t n_reads, const uint8_t* bases,
                    const int64_t* first_base, const int32_t* n_bases, int32_t n_seqs, const int32_t* pairs, int32_t n_pairs,
                    uint32_t max_deviation, float* out) {
  if (!d || n_reads < 0 || !row_offsets) return LVA_ERR_ARG;
  size_t T = 0;
  if (check_offsets(row_offsets, n_reads, &T) != LVA_OK) return LVA_ERR_ARG;
  const std::vector<int32_t> len = read_lengths(row_offsets, n_reads);
  const std::vector<int64_t> nb(len.begin(), len.end());
  return score_stage(d, post, T, true, row_offsets, nb.data(), n_reads, bases, first_base, n_bases, n_seqs, pairs, n_pairs,
                     max_deviation, out);
}

int lva_forward_bases_device(lva_decoder* d, const float* post_dev, const int64_t* first_block, const int64_t* n_blocks, int32_t n_reads,
                             const uint8_t* bases, const int64_t* first_base, const int32_t* n_bases, int32_t n_seqs,
                             const int32_t* pairs, int32_t n_pairs, uint32_t max_deviation, float* out) {
  return score_stage(d, post_dev, 0, false, first_block, n_blocks, n_reads, bases, first_base, n_bases, n_seqs, pairs, n_pairs,
                     max_deviation, out, ScoreKind::kForward);
}

int lva_forward_bases(lva_decoder* d, const float* post, const int64_t* row_offsets, int32_t n_reads, const uint8_t* bases,
                      const int64_t* first_base, const int32_t* n_bases, int32_t n_seqs, const int32_t* pairs, int32_t n_pairs,
                      uint32_t max_deviation, float* out) {
  if (!d || n_reads < 0 || !row_offsets) return LVA_ERR_ARG;
  size_t T = 0;
  if (check_offsets(row_offsets, n_reads, &T) != LVA_OK) return LVA_ERR_ARG;
  const std::vector<int32_t> len = read_lengths(row_offsets, n_reads);
  const std::vector<int64_t> nb(len.begin(), len.end());
  return score_stage(d, post, T, true, row_offsets, nb.data(), n_reads, bases, first_base, n_bases, n_seqs, pairs, n_pairs,
                     max_deviation, out, ScoreKind::kForward);
}

int lva_trace_bases_device(lva_decoder* d, const float* post_dev, const int64_t* first_block, const int64_t* n_blocks, int32_t n_reads,
                           const uint8_t* bases, const int64_t* first_base, const int32_t* n_bases, int32_t n_seqs,
                           const int32_t* pairs, int32_t n_pairs, uint32_t max_deviation, int32_t end, uint64_t scratch_limit,
                           int32_t stride, float* out_score, int32_t* out_enter, uint8_t* out_kind, int32_t* out_info) {
  const TraceOut tr{end, scratch_limit, stride, out_enter, out_kind, out_info};
  return score_stage(d, post_dev, 0, false, first_block, n_blocks, n_reads, bases, first_base, n_bases, n_seqs, pairs, n_pairs,
                     max_deviation, out_score, ScoreKind::kTrace, &tr);
}

int lva_trace_bases(lva_decoder* d, const float* post, const int64_t* row_offsets, int32_t n_reads, const uint8_t* bases,
                    const int64_t* first_base, const int32_t* n_bases, int32_t n_seqs, const int32_t* pairs, int32_t n_pairs,
                    uint32_t max_deviation, int32_t end, uint64_t scratch_limit, int32_t stride, float* out_score,
                    int32_t* out_enter, uint8_t* out_kind, int32_t* out_info) {
  if (!d || n_reads < 0 || !row_offsets) return LVA_ERR_ARG;
  size_t T = 0;
  if (check_offsets(row_offsets, n_reads, &T) != LVA_OK) return LVA_ERR_ARG;
  const std::vector<int32_t> len = read_lengths(row_offsets, n_reads);
  const std::vector<int64_t> nb(len.begin(), len.end());
  const TraceOut tr{end, scratch_limit, stride, out_enter, out_kind, out_info};
  return score_stage(d, post, T, true, row_offsets, nb.data(), n_reads, bases, first_base, n_bases, n_seqs, pairs, n_pairs,
                     max_deviation, out_score, ScoreKind::kTrace, &tr);
}

}  // extern "C"
