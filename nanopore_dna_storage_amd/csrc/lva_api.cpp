// lva_api.cpp -- C ABI (include/lva_decoder.h) and the host driver of the trellis kernels: the decoder, its schedule,
// the decode stream, lva_decode_* and lva_device_*.  The stages beside the decoder are in lva_stages.cpp.
//
// Scheduling: reads are independent.  The decoder keeps S read slots resident in
// HBM; one trellis-step launch advances every active slot by one time step of its own read,
// so reads of different lengths overlap freely: a slot whose read finishes is gathered and
// re-initialised for the next read while the others continue ("continuous batching" of the
// reference's sequential time loop :667).  Everything is enqueued on one HIP stream without
// host synchronisation until the results are copied back.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <limits>
#include <numeric>
#include <utility>

#include "lva_host.h"
#include "lva_kernels.h"

using namespace lva;

static thread_local std::string g_hip_error;

void lva::set_hip_error(const std::string& text) { g_hip_error = text; }

extern "C" {

#ifndef LVA_BUILD_ID
#define LVA_BUILD_ID "unknown"
#endif
const char* lva_version(void) { return "lva_hip 5.0 (gfx950) build " LVA_BUILD_ID; }

int lva_abi_version(void) { return LVA_ABI_VERSION; }

const char* lva_last_hip_error(void) { return g_hip_error.c_str(); }

const char* lva_strerror(int code) {
  switch (code) {
    case LVA_OK: return "ok";
    case LVA_ERR_MEM_CONV: return "Invalid mem_conv (allowed: 6, 8, 11, 14)";
    case LVA_ERR_RATE: return "Invalid rate parameter (allowed: 1, 2, 3, 4, 5, 7)";
    case LVA_ERR_MSG_LEN: return "Output length not even. Try padding with a single 0 at end.";
    case LVA_ERR_SYNC: return "Invalid sync marker / sync period";
    case LVA_ERR_TOO_MANY_STATES: return "Too many states, can't fit in 32 bits";
    case LVA_ERR_POST_TOO_SHORT: return "Too small post matrix";
    case LVA_ERR_MSG_TOO_LONG: return "msg_len too large (message + memory must fit 256 bits, msg_len <= 255)";
    case LVA_ERR_NOMEM: return "out of memory";
    case LVA_ERR_HIP: return "HIP runtime error";
    case LVA_ERR_ARG: return "invalid argument";
    case LVA_ERR_NO_DEVICE: return "no usable HIP device (the decoder has no CPU fallback)";
    case LVA_ERR_UNSUPPORTED: return "unsupported code structure";
    case LVA_ERR_BUSY: return "busy: the stream's queue is full, or the decoder has a stream open";
    default: return "unknown error";
  }
}

int lva_code_describe(int32_t mem_conv, int32_t rate, uint32_t msg_len, int32_t rc, const char* sync_marker,
                      uint32_t sync_period, lva_code_info* out) {
  Code c;
  const int st = build_code(&c, mem_conv, rate, msg_len, rc, sync_marker, sync_period);
  if (st != LVA_OK) return st;
  if (!out) return LVA_OK;
  std::memset(out, 0, sizeof *out);
  out->nstate_pos = c.npos; out->nstate_conv = c.nconv; out->oligo_len = c.oligo_len();
  out->msg_words = c.msg_words(); out->initial_state = c.init; out->final_state = c.fin;
  out->g0 = c.g[0]; out->g1 = c.g[1]; out->pattern_len = c.plen;
  std::memcpy(out->pattern, c.pattern, 16);
  return LVA_OK;
}

int lva_code_tables(int32_t mem_conv, int32_t rate, uint32_t msg_len, int32_t rc, const char* sync_marker,
                    uint32_t sync_period, uint32_t* pos2msg, uint8_t* ptype, uint32_t* vmask, uint32_t* vval,
                    uint16_t* predtab) {
  Code c;
  const int st = build_code(&c, mem_conv, rate, msg_len, rc, sync_marker, sync_period);
  if (st != LVA_OK) return st;
  if (pos2msg) std::memcpy(pos2msg, c.pos2msg, c.npos * sizeof(uint32_t));
  if (ptype) std::memcpy(ptype, c.ptype, c.npos);
  if (vmask) std::memcpy(vmask, c.vmask, c.npos * sizeof(uint32_t));
  if (vval) std::memcpy(vval, c.vval, c.npos * sizeof(uint32_t));
  if (predtab)
    for (int T = 0; T < 4; ++T) {
      uint16_t* dst = predtab + (size_t)T * c.nconv;
      if (c.predtab[T].empty()) std::memset(dst, 0, c.nconv * sizeof(uint16_t));
      else std::memcpy(dst, c.predtab[T].data(), c.nconv * sizeof(uint16_t));
    }
  return LVA_OK;
}

int lva_code_fingerprint(int32_t mem_conv, int32_t rate, uint32_t msg_len, int32_t rc, const char* sync_marker,
                         uint32_t sync_period, const uint8_t* msg_bits, uint32_t n_bits, uint32_t* out) {
  Code c;
  const int st = build_code(&c, mem_conv, rate, msg_len, rc, sync_marker, sync_period);
  if (st != LVA_OK) return st;
  return c.fingerprint(msg_bits, n_bits, out);
}

int lva_encode(int32_t mem_conv, int32_t rate, uint32_t msg_len, const uint8_t* msgs, int32_t n_msgs,
               uint8_t* out_bases) {
  if (n_msgs < 0 || (n_msgs > 0 && (!msgs || !out_bases))) return LVA_ERR_ARG;
  Code c;
  const int st = build_code(&c, mem_conv, rate, msg_len, 0, nullptr, 0);
  if (st != LVA_OK) return st;
  for (int32_t i = 0; i < n_msgs; ++i) {
    const int e = c.encode(msgs + (size_t)i * msg_len, out_bases + (size_t)i * c.oligo_len());
    if (e != LVA_OK) return e;
  }
  return LVA_OK;
}

// the band of time step t the kernels work on: Code::working_band (lva_code.cpp)
static void working_band(const Code& c, uint32_t t, uint32_t nblk, uint32_t max_dev, uint32_t* lo_out, uint32_t* hi_out) {
  c.working_band(t, nblk, max_dev, lo_out, hi_out);
}

int lva_band_table(int32_t mem_conv, int32_t rate, uint32_t msg_len, int32_t rc, const char* sync_marker, uint32_t sync_period,
                   uint32_t nblk, uint32_t max_deviation, uint32_t* reference_lo_hi, uint32_t* working_lo_hi) {
  Code c;
  const int st = build_code(&c, mem_conv, rate, msg_len, rc, sync_marker, sync_period);
  if (st != LVA_OK) return st;
  if (max_deviation == LVA_MAX_DEVIATION_DEFAULT) max_deviation = msg_len + (uint32_t)mem_conv + 1;
  for (uint32_t t = 0; t < nblk; ++t) {
    uint32_t lo, hi;
    if (reference_lo_hi) { c.band(t, nblk, max_deviation, &lo, &hi); reference_lo_hi[2 * t] = lo; reference_lo_hi[2 * t + 1] = hi; }
    if (working_lo_hi) { working_band(c, t, nblk, max_deviation, &lo, &hi); working_lo_hi[2 * t] = lo; working_lo_hi[2 * t + 1] = hi; }
  }
  return LVA_OK;
}

int lva_algorithmic_bytes(int32_t mem_conv, int32_t rate, uint32_t msg_len, int32_t rc, const char* sync_marker,
                          uint32_t sync_period, uint32_t nblk, uint32_t list_size, uint32_t max_deviation,
                          double* out) {
  Code c;
  const int st = build_code(&c, mem_conv, rate, msg_len, rc, sync_marker, sync_period);
  if (st != LVA_OK) return st;
  if (max_deviation == LVA_MAX_DEVIATION_DEFAULT) max_deviation = msg_len + (uint32_t)mem_conv + 1;
  if (out) *out = c.algorithmic_bytes(nblk, list_size, max_deviation);
  return LVA_OK;
}

// ------------------------------------------------------------------------------------------

static int upload_codes(lva_decoder* d) {
  // predecessor tables of both orientations in one allocation: [orient 2][type 4][nconv]
  const uint32_t N = d->code[0].nconv;
  std::vector<uint16_t> host((size_t)2 * 4 * N, 0);
  for (int o = 0; o < 2; ++o)
    for (int T = 0; T < 4; ++T)
      if (!d->code[o].predtab[T].empty())
        std::memcpy(host.data() + ((size_t)o * 4 + T) * N, d->code[o].predtab[T].data(), N * sizeof(uint16_t));
  HIP_TRY(hipMalloc(&d->d_predtab, host.size() * sizeof(uint16_t)));
  HIP_TRY(hipMemcpy(d->d_predtab, host.data(), host.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  DevCode dc[2];
  std::memset(dc, 0, sizeof dc);
  for (int o = 0; o < 2; ++o) {
    const Code& c = d->code[o];
    dc[o].m = (uint32_t)c.mem_conv; dc[o].nconv = c.nconv; dc[o].npos = c.npos; dc[o].init = c.init; dc[o].fin = c.fin;
    std::memcpy(dc[o].ptype, c.ptype, sizeof dc[o].ptype);
    std::memcpy(dc[o].vmask, c.vmask, sizeof dc[o].vmask);
    std::memcpy(dc[o].vval, c.vval, sizeof dc[o].vval);
    std::memcpy(dc[o].fpc, c.fpc, sizeof dc[o].fpc);
    for (uint32_t p = 0; p < c.npos; ++p) dc[o].npair[p] = (uint8_t)std::max<uint32_t>(1, (c.nbits[p] + 63) / 64);
    for (int T = 0; T < 4; ++T)
      dc[o].predtab[T] = c.predtab[T].empty() ? nullptr : d->d_predtab + ((size_t)o * 4 + T) * N;
    for (uint32_t p = 0; p < c.npos; ++p) {
      const uint32_t q = p ? p - 1 : 0;
      PosRec& r = dc[o].rec[p];
      r.info = (uint32_t)dc[o].ptype[p] | (uint32_t)dc[o].ptype[q] << 8 | (uint32_t)dc[o].npair[p] << 16 | (uint32_t)dc[o].npair[q] << 24;
      r.vmask = c.vmask[p]; r.vval = c.vval[p]; r.vmask1 = c.vmask[q]; r.vval1 = c.vval[q];
      for (int nb = 0; nb < 4; ++nb) r.fpc[nb] = c.fpc[p][nb];
      r.np2 = p >= 2 ? dc[o].npair[p - 2] : 1u;
      auto one_bit = [&](int64_t at) -> uint32_t { return at >= 1 && dc[o].ptype[at] == 0 ? 1u : 0u; };   // compact lists there (Geometry::cmp)
      r.cmp3 = one_bit(p) | one_bit((int64_t)p - 1) << 1 | one_bit((int64_t)p - 2) << 2;
      r.xs = 0;
      r.pred = dc[o].predtab[dc[o].ptype[p] & 3]; r.pred1 = dc[o].predtab[dc[o].ptype[q] & 3];
    }
    // XCD-aware tile order (PosRec::xs; lva_kernels.hip xcd_tile).  A 128-byte line of position p's lists -- 16 consecutive conv
    // states, line index q = conv / 16 -- is read twice in the launch after the one that wrote it: as the own (stay) list of its
    // targets by the workgroup at p whose butterfly ends there (tile = q without the bits the step into p shifted in, sh = 1 or 2 of
    // them), and as a source list by the workgroup (tile q >> 2, p + 1).  With workgroups dealt round-robin over the 8 XCDs
    // (MI355X_MICROARCH.md, workgroup dispatch: observed, a speed matter only) a workgroup (tile, p) runs on the XCD labelled by
    // bits xs[p] .. xs[p]+2 of its tile, and both readers share an XCD -- and its L2 -- when xs[p] = xs[p+1] + sh.  Greedy chain
    // from the largest shift the tile count allows; 0 = the plain order.  Used by the L = 1 kernel only: the list kernels
    // reach their stay lists too late for the staged rows to be still in L2 (measured: nothing at m=11, -1 % at m=14).
    auto chain = [&](int tile_bits) {
      if (tile_bits < 4) return;
      const uint32_t smax = std::min<uint32_t>((uint32_t)tile_bits - 3u, 2u);   // (larger shifts spread a launch's neighbours over the rows: m=14 -2 %)
      uint32_t s = smax;
      for (uint32_t p = 1; p < c.npos; ++p) {
        dc[o].rec[p].xs = s;
        const uint32_t sh = c.shift_of(c.ptype[p]);
        s = s >= sh ? s - sh : smax;
      }
    };
    // (measurements: LVA_NO_XCD_ORDER=1 together with LVA_TESTING=1 keeps the plain order)
    const char* plain = std::getenv("LVA_NO_XCD_ORDER"); const char* testing = std::getenv("LVA_TESTING");
    if (!(plain && plain[0] == '1' && testing && testing[0] == '1')) chain(c.mem_conv - 6);
  }
  // Compact lists (Geometry::cmp) store crf state k's list as list k >> 1 at a one-bit position: that needs the reachable bases
  // of every valid conv state there to be a complementary pair ({A,T} or {C,G}).  True of the four built-in generator pairs
  // (tests/test_code_tables.py); checked here so that a code added later cannot alias two lists silently.
  if (d->g.cmp)
    for (int o = 0; o < 2; ++o) {
      const Code& c = d->code[o];
      for (uint32_t p = 1; p < c.npos; ++p) {
        if (c.ptype[p] != 0 || c.predtab[0].empty()) continue;
        for (uint32_t cv = 0; cv < N; ++cv) {
          if ((cv & c.vmask[p]) != c.vval[p]) continue;
          const uint32_t pk = c.predtab[0][cv];
          const uint32_t has = ((pk >> 3) & 1u) | (((pk >> 7) & 1u) << 1) | (((pk >> 11) & 1u) << 2) | (((pk >> 15) & 1u) << 3);
          if (has != 0x9u && has != 0x6u && has != 0u) return LVA_ERR_UNSUPPORTED;
        }
      }
    }
  HIP_TRY(hipMalloc(&d->d_codes, sizeof dc));
  HIP_TRY(hipMemcpy(d->d_codes, dc, sizeof dc, hipMemcpyHostToDevice));
  return LVA_OK;
}

// Positions at which every tile of 64 source conv states feeds at least one valid target conv state, in both orientations:
// the longest run [full_lo, full_hi].  A target conv state of tile x at position p is  x*Tn + low + leg*(N >> sh)  (low < Tn =
// 64 >> sh, leg < 2^sh): its middle bits are the tile's, so the tile has a valid target iff those bits agree with the mask.
static void full_tile_positions(lva_decoder* d) {
  const Code& c = d->code[0];
  const uint32_t N = c.nconv;
  std::vector<uint8_t> full(c.npos, 0);
  for (uint32_t p = 1; p < c.npos; ++p) {
    bool ok = N >= 64;
    for (int o = 0; o < 2 && ok; ++o) {
      const Code& co = d->code[o];
      const uint32_t sh = co.ptype[p] == 0 ? 1u : 2u, Tn = 64u >> sh;
      const uint32_t mid = (N - 1) & ~(Tn - 1) & ~(((1u << sh) - 1u) << ((uint32_t)co.mem_conv - sh));
      for (uint32_t x = 0; x < N / 64 && ok; ++x) ok = ((x * Tn) & co.vmask[p] & mid) == (co.vval[p] & mid);
    }
    full[p] = ok ? 1 : 0;
  }
  uint32_t best = 0, run = 0;
  for (uint32_t p = 1; p < c.npos; ++p) {
    run = full[p] ? run + 1 : 0;
    if (run > best) { best = run; d->full_hi = p; d->full_lo = p + 1 - run; }
  }
}

// What a configuration decides before its trellis is laid out, in the order its refusals are reported: the codes of both
// orientations, the limits of the message and the state index, the band half-width, the kernel plan and the ring length.
static int plan_config(const lva_config* cfg, Code* code, uint32_t* max_dev, Plan* plan, uint32_t* ring) {
  if (cfg->list_size == 0 || cfg->list_size > 65535) return LVA_ERR_ARG;
  for (int o = 0; o < 2; ++o) {
    const int st = build_code(&code[o], cfg->mem_conv, cfg->rate, cfg->msg_len, o, cfg->sync_marker ? cfg->sync_marker : "", cfg->sync_period);
    if (st != LVA_OK) return st;
  }
  const Code& c = code[0];
  if (c.msg_len > 255 || c.msg_len + (uint32_t)c.mem_conv > 256) return LVA_ERR_MSG_TOO_LONG;
  if ((uint64_t)c.npos * kCrf * c.nconv >= ((uint64_t)1 << 32)) return LVA_ERR_TOO_MANY_STATES;
  *max_dev = cfg->max_deviation == LVA_MAX_DEVIATION_DEFAULT ? c.msg_len + (uint32_t)c.mem_conv + 1 : cfg->max_deviation;
  const int st = plan_kernels(cfg->kernel, cfg->list_size, c.msg_bits(), plan);
  if (st != LVA_OK) return st;
  *ring = (uint32_t)std::max<uint64_t>(std::min<uint64_t>(c.npos, 2ull * *max_dev + plan->ring_extra), 1);
  return LVA_OK;
}

int lva_kernel_plan(const lva_config* cfg, lva_kernel_plan_info* out) {
  if (!cfg || !out) return LVA_ERR_ARG;
  Code code[2];
  uint32_t max_dev, ring;
  Plan plan;
  const int st = plan_config(cfg, code, &max_dev, &plan, &ring);
  if (st != LVA_OK) return st;
  out->mode = plan.mode; out->dominant = (int32_t)plan.dominant; out->fixup = (int32_t)plan.fixup;
  out->lazy = plan.lazy; out->rec = plan.rec; out->cmp = plan.cmp;
  out->ring_positions = ring; out->instance = plan.inst;
  return LVA_OK;
}

int lva_decoder_create(const lva_config* cfg, lva_decoder** out) {
  if (!cfg || !out) return LVA_ERR_ARG;
  *out = nullptr;
  Code code[2];
  uint32_t max_dev, ring;
  Plan plan;
  {
    const int st = plan_config(cfg, code, &max_dev, &plan, &ring);
    if (st != LVA_OK) return st;
  }
  const Geometry g = make_geometry(code[0].nconv, cfg->list_size, code[0].msg_bits(), ring, plan.lazy, plan.rec, plan.cmp);
  if (g.sPar >= ((uint64_t)1 << 32)) return LVA_ERR_TOO_MANY_STATES;
  lva_decoder* d = new (std::nothrow) lva_decoder();
  if (!d) return LVA_ERR_NOMEM;
  auto fail = [&](int code) { lva_decoder_destroy(d); return code; };
  d->cfg = *cfg;
  d->sync_marker = cfg->sync_marker ? cfg->sync_marker : "";
  d->cfg.sync_marker = nullptr;
  d->code[0] = std::move(code[0]); d->code[1] = std::move(code[1]);
  d->max_dev = max_dev; d->plan = plan; d->g = g;
  d->prof.kernel = plan.mode;
  full_tile_positions(d);
  const Code& c = d->code[0];
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) return fail(LVA_ERR_NO_DEVICE);
  d->device = cfg->device;
  if (hipSetDevice(d->device) != hipSuccess) return fail(LVA_ERR_NO_DEVICE);
  if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) return fail(LVA_ERR_HIP);
  for (hipEvent_t* ev : {&d->ev_total0, &d->ev_total1, &d->ev_step0, &d->ev_step1, &d->ev_h2d})
    if (hipEventCreate(ev) != hipSuccess) return fail(LVA_ERR_HIP);
  {
    const int st = upload_codes(d);
    if (st != LVA_OK) return fail(st);
  }
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return fail(LVA_ERR_HIP);
  const uint64_t slot_bytes = d->g.sSlot * sizeof(uint32_t);
  uint64_t budget = cfg->mem_budget_bytes ? cfg->mem_budget_bytes : (uint64_t)(free_b * 0.6);
  // reads in flight: enough of them that one trellis-step launch fills the chip -- a launch has
  // (2^m / 64 tiles) x (<= 2 max_deviation positions) x slots workgroups, so small trellises take
  // proportionally more slots (128 at m >= 11, 256 at m = 8, 1024 at m = 6: measured), and four times as many at
  // L = 1, whose launches are that much shorter (m = 6: 0.11 ms at 1024 slots; 4096 slots +15 %, m = 11: 128 slots +5 %: round 5,
  // scripts/r5/slot_sweep_small.sh); bounded by the memory budget and by the work-list item format (21 - m bits of slot index)
  const uint64_t hard = std::min<uint64_t>(kMaxSlotsLimit, 1ull << (21 - std::min(c.mem_conv, 20)));
  int slots = (int)std::min<uint64_t>(budget / slot_bytes, hard);
  if (cfg->max_slots > 0) slots = std::min(slots, (int)cfg->max_slots);
  else {
    const uint64_t per_l = cfg->list_size == 1 ? 4 : 1;
    // (never fewer than 128: the tail of a launch -- 74 k workgroups over 1024 resident ones at 64 slots of m = 11 -- costs 1.8 %)
    slots = std::min<int>(slots, (int)std::max<uint64_t>(128, std::min<uint64_t>(1024 * per_l, per_l * 32ull * 2048 / c.nconv)));
  }
  if (slots < 1) return fail(LVA_ERR_NOMEM);
  d->slots = slots;
  if (hipMalloc(&d->d_trellis, (size_t)slots * slot_bytes) != hipSuccess) return fail(LVA_ERR_NOMEM);
  if (hipMalloc(&d->d_slots, (size_t)slots * sizeof(SlotDesc)) != hipSuccess) return fail(LVA_ERR_NOMEM);
  if (hipMemset(d->d_slots, 0, (size_t)slots * sizeof(SlotDesc)) != hipSuccess) return fail(LVA_ERR_HIP);
  if (hipMalloc(&d->d_steps, (size_t)slots * sizeof(SlotStep)) != hipSuccess) return fail(LVA_ERR_NOMEM);
  d->prof.slots = slots;
  // tests: force the work-list overflow path.  Honoured only together with LVA_TESTING=1 -- a stray LVA_WORK_CAP in a user's
  // environment would cost an order of magnitude silently (visible through lva_profile.overflow_steps only)
  if (const char* cap = std::getenv("LVA_WORK_CAP")) {
    const char* testing = std::getenv("LVA_TESTING");
    const long v = std::atol(cap);
    if (testing && testing[0] == '1' && v >= 1 && v <= (1l << 24)) d->work_cap = (uint32_t)v;
  }
  if (hipMalloc(&d->d_work, sizeof(WorkHdr) + (size_t)d->work_cap * sizeof(uint32_t)) != hipSuccess) return fail(LVA_ERR_NOMEM);
  *out = d;
  return LVA_OK;
}

void lva_decoder_destroy(lva_decoder* d) {
  if (!d) return;
  if (d->open_stream) (void)lva_stream_close(d->open_stream);
  (void)hipSetDevice(d->device);
  if (d->stream) (void)hipStreamSynchronize(d->stream);
  if (d->d_trellis) (void)hipFree(d->d_trellis);
  if (d->d_results) (void)hipFree(d->d_results);
  if (d->d_work) (void)hipFree(d->d_work);
  if (d->d_slots) (void)hipFree(d->d_slots);
  if (d->d_steps) (void)hipFree(d->d_steps);
  if (d->d_band) (void)hipFree(d->d_band);
  if (d->d_tp_fwd) (void)hipFree(d->d_tp_fwd);
  if (d->d_tp_off) (void)hipFree(d->d_tp_off);
  for (hipEvent_t e : d->ev_pool) (void)hipEventDestroy(e);
  if (d->ev_h2d) (void)hipEventDestroy(d->ev_h2d);
  if (d->d_codes) (void)hipFree(d->d_codes);
  if (d->d_predtab) (void)hipFree(d->d_predtab);
  if (d->ev_total0) (void)hipEventDestroy(d->ev_total0);
  if (d->ev_total1) (void)hipEventDestroy(d->ev_total1);
  if (d->ev_step0) (void)hipEventDestroy(d->ev_step0);
  if (d->ev_step1) (void)hipEventDestroy(d->ev_step1);
  if (d->stream) (void)hipStreamDestroy(d->stream);
  delete d;
}

int lva_decoder_set_launch_events(lva_decoder* d, int32_t on) {
  if (!d) return LVA_ERR_ARG;
  d->launch_events = on ? 1 : 0;
  return LVA_OK;
}

int lva_decoder_profile(const lva_decoder* d, lva_profile* out) {
  if (!d || !out) return LVA_ERR_ARG;
  *out = d->prof;
  return LVA_OK;
}

// final selection (:806-844) on the host: gather finite entries crf-major, std::sort by score
// descending (the same libstdc++ algorithm the reference calls), keep list_size, unpack bits
static void finish_read(const lva_decoder* d, int orient, const uint32_t* rec, uint8_t* out_msgs, float* out_scores,
                        int32_t* out_count) {
  struct Path { float score; const uint32_t* words; };
  const uint32_t L = d->g.L, F = d->g.F;
  const Code& c = d->code[orient];
  std::vector<Path> paths;
  paths.reserve((size_t)8 * L);
  const float NEG = -std::numeric_limits<float>::infinity();
  for (uint32_t k = 0; k < 8; ++k)
    for (uint32_t l = 0; l < L; ++l) {
      const uint32_t* e = rec + ((size_t)k * L + l) * F;
      float s;
      std::memcpy(&s, e, sizeof s);
      if (s != NEG) paths.push_back({s, e + 2});
    }
  std::sort(paths.begin(), paths.end(), [](const Path& a, const Path& b) -> bool { return a.score > b.score; });
  if (paths.size() > L) paths.resize(L);
  const uint32_t total = c.msg_len + (uint32_t)c.mem_conv;
  for (size_t i = 0; i < paths.size(); ++i) {
    uint8_t* o = out_msgs + i * c.msg_len;
    for (uint32_t b = 0; b < c.msg_len; ++b) {
      const uint32_t bit = total - 1 - b;                              // :831-834
      const uint8_t v = (uint8_t)((paths[i].words[bit >> 5] >> (bit & 31)) & 1u);
      o[c.rc ? c.msg_len - 1 - b : b] = v;                             // :835
    }
    if (out_scores) out_scores[i] = paths[i].score;
  }
  *out_count = (int32_t)paths.size();
}

}  // extern "C"

// band of every time step of one read (:677-679), evaluated here as the reference binary does: out[nb] = lo | hi << 16 (| lazy flags)
static void read_band_table(const lva_decoder* d, const Code& c, uint32_t nb, uint32_t* out) {
  // lazy mode: when was each position's row of either parity buffer last written?  Step t reads the buffer written
  // by steps of t-1's parity; only the row of position lo-1 can be older than t-1 ("stale"), and at odd t
  // its entries' messages live in the message buffer of the (even) step that wrote it
  std::vector<int64_t> last_w[2];
  if (d->g.lazy) { last_w[0].assign(c.npos + 1, -1); last_w[1].assign(c.npos + 1, -1); if (c.npos) last_w[1][0] = -1; }
  for (uint32_t t = 0; t < nb; ++t) {
    uint32_t lo, hi;
    working_band(c, t, nb, d->max_dev, &lo, &hi);
    uint32_t w = lo | (hi << 16);
    if (d->g.lazy) {
      const int pc = (int)((t + 1) & 1u);                // parity class of the steps that wrote step t's "prev" buffer: t-1
      if (t >= 1 && lo >= 1) {
        const int64_t lw = last_w[pc][lo - 1];
        if (lw >= 0 && lw != (int64_t)t - 1) w |= 1u << 30 | (uint32_t)((lw >> 1) & 1) << 31;
      }
      for (uint32_t p = lo; p < hi; ++p) last_w[t & 1u][p] = t;
    }
    out[t] = w;
  }
}

namespace {
// The host schedule, written once for a batch call (decode_impl) and for a decode stream (lva_stream_poll): reads enter slots
// (fill), one launch group advances every active slot by one time step (launch), finished reads leave through the gather
// (retire).  Which read goes into which slot, and when, is the caller's: longest first for a batch, first in first served
// for a stream.  A read's result depends on neither.
struct Schedule {
  struct Slot {
    int32_t read = -1;         // the caller's name of the read in the slot
    uint32_t end = 0;          // launch number after the read's last step
    uint32_t nblk = 0, orient = 0;
    uint32_t last_band = 0;    // band word of the last time step: was the final state ever written?
    uint32_t rec = 0;          // result record the gather writes
  };
  lva_decoder* d;
  std::vector<Slot> slot;
  uint32_t* results;           // device, [records][8 L F words]
  bool launch_events;
  size_t active = 0;
  size_t waiting = 0;          // slots whose read starts with the launch after next (lazy mode's phase alignment)
  size_t ev_used = 0;
  bool first_step = true;
  InitBatch ib;
  GatherBatch gb;

  Schedule(lva_decoder* dec, size_t nslots, uint32_t* res, bool events) : d(dec), slot(nslots), results(res), launch_events(events) {
    ib.n = 0; ib.pad = 0; gb.n = 0;
  }
  void reset_profile() {
    lva_profile& p = d->prof;
    p.step_launches = 0; p.read_steps = 0; p.algorithmic_bytes = 0; p.working_bytes = 0; p.fixup_states = 0; p.overflow_steps = 0;
    p.dominant_kernel_ms = 0; p.step_pair_ms = 0; p.timed_launches = 0;
  }
  int next_event(hipEvent_t* out) {
    if (ev_used == d->ev_pool.size()) {
      hipEvent_t e;
      HIP_TRY(hipEventCreate(&e));
      d->ev_pool.push_back(e);
    }
    *out = d->ev_pool[ev_used++];
    return LVA_OK;
  }
  int flush_inits() {
    const int e = launch_init_slots(d->g, d->d_codes, d->d_trellis, ib, d->d_slots, d->stream);
    ib.n = 0;
    return launch_status(e);
  }
  int flush_gathers() {
    const int e = launch_gather_finals(d->g, d->d_codes, d->d_trellis, gb, results, d->stream);
    gb.n = 0;
    return launch_status(e);
  }
  // a read enters idle slot s: its descriptor and initial scores (:657-663) go in stream order, a batch of slots per launch
  // (behind the gathers of the reads that left them: retire runs before the next fill)
  int fill(size_t s, int32_t read, const float* post_dev, const uint32_t* band_dev, uint32_t nblk, uint32_t orient, uint32_t last_band,
           uint32_t rec) {
    SlotDesc sd;
    sd.post = post_dev;
    sd.band = band_dev;
    sd.nblk = nblk; sd.orient = orient;
    // Lazy mode: every read starts on an EVEN launch (a read that arrives on an odd one idles for one launch: 1 in ~500),
    // so all slots are at an even time step on even launches and at an odd one on odd launches -- a launch then runs ONE
    // instance of lva_step_lazy over a grid without workgroups of the wrong kind (launch_step, phase_aligned)
    sd.start = d->launch_no + (d->plan.lazy ? (d->launch_no & 1u) : 0u); sd.pad = 0;
    Slot& sl = slot[s];
    sl.read = read; sl.end = sd.start + sd.nblk; sl.nblk = nblk; sl.orient = orient; sl.last_band = last_band; sl.rec = rec;
    if (sd.start != d->launch_no) ++waiting;
    ib.slot[ib.n] = (uint32_t)s; ib.desc[ib.n] = sd;
    if (++ib.n == (uint32_t)kTurnoverBatch) { const int st = flush_inits(); if (st) return st; }
    d->prof.algorithmic_bytes += d->code[orient].algorithmic_bytes(nblk, d->g.L, d->max_dev);
    d->prof.working_bytes += d->code[orient].working_bytes(nblk, d->g.L, d->max_dev);
    ++active;
    return LVA_OK;
  }
  // one launch group over slots [0, nslots): prepare, dominant kernel, fix-up
  int launch(uint32_t nslots) {
    const uint32_t npos = d->code[0].npos;
    StepArgs a;
    a.slots = d->d_slots; a.steps = d->d_steps; a.nslots = nslots; a.band_max = std::min<uint32_t>(npos, 2 * d->max_dev);
    a.launch_no = d->launch_no; a.step_parity = d->launch_no & 1u;
    a.phase_aligned = d->plan.lazy;
    a.full_lo = d->full_lo; a.full_hi = d->full_hi; a.pad = 0;
    {
      const int e = launch_prepare_step(a, d->d_codes, d->d_steps, d->stream);
      if (e) return launch_status(e);
    }
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    if (launch_events) {
      int st;
      if ((st = next_event(&e0)) || (st = next_event(&e1)) || (st = next_event(&e2))) return st;
      HIP_TRY(hipEventRecord(e0, d->stream));
      if (first_step) HIP_TRY(hipEventRecord(d->ev_step0, d->stream));
    } else if (first_step) {
      HIP_TRY(hipEventRecord(d->ev_step0, d->stream));
    }
    first_step = false;
    {
      const int e = launch_step(d->plan, a, d->g, d->d_codes, d->d_trellis, d->d_work, reinterpret_cast<uint32_t*>(d->d_work + 1), d->stream, e1);
      if (e) return launch_status(e);
    }
    if (e2) HIP_TRY(hipEventRecord(e2, d->stream));
    ++d->launch_no;
    d->prof.step_launches += 1;
    d->prof.read_steps += active - waiting;
    waiting = 0;
    return LVA_OK;
  }
  // reads whose last step was the launch just enqueued leave their slots: left(slot, gathered) for each; gathered = false
  // when the final state was never written (an empty list, no record)
  template <class F>
  int retire(F&& left) {
    const uint32_t npos = d->code[0].npos;
    for (size_t s = 0; s < slot.size(); ++s) {
      Slot& sl = slot[s];
      if (sl.read < 0 || sl.end != d->launch_no) continue;
      const bool got = (sl.last_band & 0xFFFFu) <= npos - 1 && npos - 1 < ((sl.last_band >> 16) & 0x3FFFu);
      if (got) {
        gb.a[gb.n] = GatherArgs{(uint32_t)s, (uint32_t)(sl.nblk & 1u), sl.orient, sl.rec, sl.nblk};
        if (++gb.n == (uint32_t)kTurnoverBatch) { const int st = flush_gathers(); if (st) return st; }
      }
      left(sl, got);
      sl.read = -1;
      --active;
    }
    return flush_gathers();
  }
  // the totals a call or a stream leaves in the profile once the device is idle
  int close_profile(const WorkHdr& h1) {
    d->prof.fixup_states = h1.total;
    d->prof.overflow_steps = h1.overflow_steps;
    for (int i = 0; i < 4; ++i) d->prof.fixup_reason[i] = h1.reason[i];
    float ms = 0;
    if (!first_step) { HIP_TRY(hipEventElapsedTime(&ms, d->ev_step0, d->ev_step1)); }
    d->prof.step_kernel_ms = ms;
    HIP_TRY(hipEventElapsedTime(&ms, d->ev_total0, d->ev_total1));
    d->prof.total_ms = ms;
    for (size_t i = 0; i + 3 <= ev_used; i += 3) {
      float a_ms = 0, b_ms = 0;
      HIP_TRY(hipEventElapsedTime(&a_ms, d->ev_pool[i], d->ev_pool[i + 1]));
      HIP_TRY(hipEventElapsedTime(&b_ms, d->ev_pool[i], d->ev_pool[i + 2]));
      d->prof.dominant_kernel_ms += a_ms;
      d->prof.step_pair_ms += b_ms;
      d->prof.timed_launches += 1;
    }
    return LVA_OK;
  }
};
}  // namespace

extern "C" {

static int decode_impl(lva_decoder* d, const float* post_dev, const int64_t* beg, const int64_t* len, int32_t n, const uint8_t* rc_flags,
                       uint8_t* out_msgs, float* out_scores, int32_t* out_counts, bool timed_total_started) {
  const Geometry& g = d->g;
  const uint32_t npos = d->code[0].npos, L = g.L;
  const size_t rec_words = (size_t)8 * L * g.F;
  // host buffers that asynchronous copies read or write: declared BEFORE the drain, so that on every error exit the
  // drain's hipStreamSynchronize runs first and these die afterwards (locals are destroyed in reverse order)
  std::vector<uint32_t> band, host;
  std::vector<uint8_t> gathered;
  WorkHdr h0, h1;
  StreamDrain drain(d->stream);
  // reads the reference would refuse (:600-601)
  std::vector<int32_t> order;
  size_t band_words = 0;
  for (int32_t i = 0; i < n; ++i) {
    const int64_t nb = len[i];
    if (nb < 0 || nb > 0xFFFFFFFFll || beg[i] < 0) return LVA_ERR_ARG;
    if ((uint64_t)nb < (uint64_t)npos + 1) out_counts[i] = LVA_ERR_POST_TOO_SHORT;
    else { out_counts[i] = 0; order.push_back(i); band_words += (size_t)nb; }
  }
  // longest first: the tail of the schedule is then made of short reads
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return len[a] > len[b]; });

  if ((size_t)n > d->results_cap) {
    if (d->d_results) (void)hipFree(d->d_results);
    d->d_results = nullptr; d->results_cap = 0;
    HIP_TRY(hipMalloc(&d->d_results, (size_t)n * rec_words * sizeof(uint32_t)));
    d->results_cap = (size_t)n;
  }
  if (!timed_total_started) HIP_TRY(hipEventRecord(d->ev_total0, d->stream));

  band.assign(std::max<size_t>(band_words, 1), 0u);
  std::vector<size_t> band_at((size_t)n, 0);
  {
    size_t at = 0;
    for (int32_t r : order) {
      band_at[(size_t)r] = at;
      read_band_table(d, d->code[rc_flags && rc_flags[r] ? 1 : 0], (uint32_t)len[r], band.data() + at);
      at += (size_t)len[r];
    }
  }
  if (band.size() > d->band_cap) {
    if (d->d_band) (void)hipFree(d->d_band);
    d->d_band = nullptr; d->band_cap = 0;
    HIP_TRY(hipMalloc(&d->d_band, band.size() * sizeof(uint32_t)));
    d->band_cap = band.size();
  }
  HIP_TRY(hipMemcpyAsync(d->d_band, band.data(), band.size() * sizeof(uint32_t), hipMemcpyHostToDevice, d->stream));
  std::memset(&h0, 0, sizeof h0);
  h0.cap = d->work_cap;
  HIP_TRY(hipMemcpyAsync(d->d_work, &h0, sizeof h0, hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipMemsetAsync(d->d_slots, 0, (size_t)d->slots * sizeof(SlotDesc), d->stream));   // nblk = 0: no slot takes part yet

  Schedule sc(d, std::min<size_t>((size_t)d->slots, std::max<size_t>(order.size(), 1)), d->d_results, d->launch_events != 0);
  sc.reset_profile();
  size_t next = 0;
  gathered.assign((size_t)n, 0);
  for (;;) {
    // (re)fill idle slots in the batch's order; a read's result record is the read's index
    for (size_t s = 0; s < sc.slot.size(); ++s) {
      if (sc.slot[s].read >= 0 || next >= order.size()) continue;
      const int32_t r = order[next++];
      const uint32_t nb = (uint32_t)len[r];
      const int st = sc.fill(s, r, post_dev + (size_t)beg[r] * 40, d->d_band + band_at[(size_t)r], nb, rc_flags && rc_flags[r] ? 1u : 0u,
                             band[band_at[(size_t)r] + nb - 1], (uint32_t)r);
      if (st) return st;
    }
    { const int st = sc.flush_inits(); if (st) return st; }
    if (sc.active == 0) break;
    { const int st = sc.launch((uint32_t)sc.slot.size()); if (st) return st; }
    { const int st = sc.retire([&](const Schedule::Slot& sl, bool got) { if (got) gathered[(size_t)sl.read] = 1; }); if (st) return st; }
  }
  if (!sc.first_step) HIP_TRY(hipEventRecord(d->ev_step1, d->stream));
  host.assign((size_t)n * rec_words, 0u);
  if (n > 0) HIP_TRY(hipMemcpyAsync(host.data(), d->d_results, host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipMemcpyAsync(&h1, d->d_work, sizeof h1, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipEventRecord(d->ev_total1, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  drain.armed = false;
  { const int st = sc.close_profile(h1); if (st) return st; }

  for (int32_t i = 0; i < n; ++i) {
    if (out_counts[i] < 0) continue;
    if (!gathered[(size_t)i]) { out_counts[i] = 0; continue; }
    finish_read(d, rc_flags && rc_flags[i] ? 1 : 0, host.data() + (size_t)i * rec_words,
                out_msgs + (size_t)i * L * d->code[0].msg_len, out_scores ? out_scores + (size_t)i * L : nullptr,
                &out_counts[i]);
  }
  return LVA_OK;
}

// ---------------------------------------------------------------------------------------------
// Decode stream: the same schedule, fed while it runs.  No thread of its own: lva_stream_poll drives it.
// ---------------------------------------------------------------------------------------------
struct lva_stream {
  lva_decoder* d = nullptr;
  uint32_t queue_cap = 0;
  Schedule* sch = nullptr;
  size_t rec_words = 0;
  // one pinned host buffer + one device buffer per read in flight: 40 floats per block, then one band word per block.  A buffer
  // returns to the free list when its read's result has been seen on the host (so no copy from it can still be pending)
  struct PostBuf { uint32_t* host = nullptr; uint32_t* dev = nullptr; size_t cap = 0; };
  std::vector<PostBuf> bufs;
  std::vector<int32_t> free_bufs;
  struct Read { uint64_t tag = 0; int32_t buf = -1; uint32_t nblk = 0, orient = 0, rec = 0; bool gathered = false; };
  std::vector<Read> reads;             // indexed by the read's id (Schedule::Slot::read)
  std::vector<int32_t> free_reads;
  std::deque<int32_t> queue;           // waiting for a slot, in submission order
  // a mark = an event behind a launch group: the reads that retired with that group are finished when it has passed
  struct Mark { hipEvent_t ev = nullptr; uint32_t launch_no = 0; std::vector<int32_t> reads; };
  std::deque<Mark> marks;
  std::vector<hipEvent_t> free_ev;
  struct Finished { uint64_t tag; int32_t count; std::vector<uint8_t> msgs; std::vector<float> scores; };
  std::deque<Finished> finished;
  uint32_t* d_res = nullptr;           // result records on the device ...
  uint32_t* h_res = nullptr;           // ... and their pinned host copies, one per read between fill and hand-out
  std::vector<uint32_t> free_rec;
  uint32_t done_launch = 0;            // launches the device is known to have passed
  size_t in_marks = 0;                 // reads retired on the host whose records are still on their way
  WorkHdr h0, h1;
};

namespace {
constexpr uint32_t kStreamAhead = 32;  // launches the host may be ahead of the device: what a new read waits at most before it
                                       // can join, and what poll(wait = 0) enqueues at most in one call
constexpr uint32_t kStreamMarkEvery = 4;

int stream_take_buf(lva_stream* s, size_t nblk, int32_t* out) {
  for (size_t k = 0; k < s->free_bufs.size(); ++k) {
    const int32_t b = s->free_bufs[k];
    if (s->bufs[(size_t)b].cap >= nblk) {
      s->free_bufs[k] = s->free_bufs.back();
      s->free_bufs.pop_back();
      *out = b;
      return LVA_OK;
    }
  }
  lva_stream::PostBuf pb;
  pb.cap = (std::max<size_t>(nblk, 256) + 63) / 64 * 64;
  if (hipHostMalloc(reinterpret_cast<void**>(&pb.host), pb.cap * 41 * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) return LVA_ERR_NOMEM;
  if (hipMalloc(reinterpret_cast<void**>(&pb.dev), pb.cap * 41 * sizeof(uint32_t)) != hipSuccess) { (void)hipHostFree(pb.host); return LVA_ERR_NOMEM; }
  s->bufs.push_back(pb);
  *out = (int32_t)s->bufs.size() - 1;
  return LVA_OK;
}

void stream_release_read(lva_stream* s, int32_t id) {
  lva_stream::Read& r = s->reads[(size_t)id];
  if (r.buf >= 0) s->free_bufs.push_back(r.buf);
  r.buf = -1;
  s->free_reads.push_back(id);
}

// marks the device has passed: their reads' records are on the host -> final selection, hand-out queue
int stream_reap(lva_stream* s, bool block_on_first) {
  lva_decoder* d = s->d;
  const uint32_t L = d->g.L, msg_len = d->code[0].msg_len;
  while (!s->marks.empty()) {
    lva_stream::Mark& m = s->marks.front();
    if (block_on_first) {
      HIP_TRY(hipEventSynchronize(m.ev));
      block_on_first = false;
    } else {
      const hipError_t e = hipEventQuery(m.ev);
      if (e == hipErrorNotReady) break;
      if (e != hipSuccess) { g_hip_error = std::string("hipEventQuery: ") + hipGetErrorString(e); return LVA_ERR_HIP; }
    }
    s->done_launch = m.launch_no;
    for (int32_t id : m.reads) {
      const lva_stream::Read& r = s->reads[(size_t)id];
      lva_stream::Finished f{r.tag, 0, {}, {}};
      if (r.gathered) {
        f.msgs.assign((size_t)L * msg_len, 0);
        f.scores.assign(L, 0.f);
        finish_read(d, (int)r.orient, s->h_res + (size_t)r.rec * s->rec_words, f.msgs.data(), f.scores.data(), &f.count);
      }
      s->finished.push_back(std::move(f));
      s->free_rec.push_back(r.rec);
      stream_release_read(s, id);
      --s->in_marks;
    }
    s->free_ev.push_back(m.ev);
    s->marks.pop_front();
  }
  return LVA_OK;
}

// enqueue launch groups while there is work and the host is less than kStreamAhead launches ahead of the device
int stream_pump(lva_stream* s) {
  lva_decoder* d = s->d;
  Schedule& sc = *s->sch;
  while ((sc.active > 0 || !s->queue.empty()) && d->launch_no - s->done_launch < kStreamAhead) {
    // free slots take the queue's reads in submission order, lowest slot first; a read takes its result record with it
    for (size_t k = 0; k < sc.slot.size() && !s->queue.empty() && !s->free_rec.empty() && sc.active < sc.slot.size(); ++k) {
      if (sc.slot[k].read >= 0) continue;
      const int32_t id = s->queue.front();
      s->queue.pop_front();
      lva_stream::Read& r = s->reads[(size_t)id];
      r.rec = s->free_rec.back();
      s->free_rec.pop_back();
      const lva_stream::PostBuf& pb = s->bufs[(size_t)r.buf];
      const int st = sc.fill(k, id, reinterpret_cast<const float*>(pb.dev), pb.dev + (size_t)r.nblk * 40, r.nblk, r.orient,
                             pb.host[(size_t)r.nblk * 40 + r.nblk - 1], r.rec);
      if (st) return st;
    }
    { const int st = sc.flush_inits(); if (st) return st; }
    if (sc.active == 0) break;
    uint32_t nslots = 0;
    for (size_t k = sc.slot.size(); k > 0; --k)
      if (sc.slot[k - 1].read >= 0) { nslots = (uint32_t)k; break; }
    { const int st = sc.launch(nslots); if (st) return st; }
    lva_stream::Mark m;
    {
      const int st = sc.retire([&](const Schedule::Slot& sl, bool got) {
        s->reads[(size_t)sl.read].gathered = got;
        m.reads.push_back(sl.read);
      });
      if (st) return st;
    }
    if (m.reads.empty() && d->launch_no % kStreamMarkEvery != 0) continue;
    // from here on the retired reads belong to the mark: on an error they are dropped with the stream (close drains)
    for (int32_t id : m.reads) {
      const lva_stream::Read& r = s->reads[(size_t)id];
      if (r.gathered)
        HIP_TRY(hipMemcpyAsync(s->h_res + (size_t)r.rec * s->rec_words, s->d_res + (size_t)r.rec * s->rec_words,
                               s->rec_words * sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    }
    if (s->free_ev.empty()) {
      hipEvent_t e;
      HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      s->free_ev.push_back(e);
    }
    m.ev = s->free_ev.back();
    s->free_ev.pop_back();
    m.launch_no = d->launch_no;
    s->in_marks += m.reads.size();
    const hipError_t e = hipEventRecord(m.ev, d->stream);
    s->marks.push_back(std::move(m));
    if (e != hipSuccess) { g_hip_error = std::string("hipEventRecord: ") + hipGetErrorString(e); return LVA_ERR_HIP; }
  }
  return LVA_OK;
}
}  // namespace

int lva_stream_open(lva_decoder* d, int32_t queue_cap, lva_stream** out) {
  if (!d || !out || queue_cap < 1) return LVA_ERR_ARG;
  *out = nullptr;
  if (d->open_stream) return LVA_ERR_BUSY;
  if (hipSetDevice(d->device) != hipSuccess) return LVA_ERR_NO_DEVICE;
  lva_stream* s = new (std::nothrow) lva_stream();
  if (!s) return LVA_ERR_NOMEM;
  s->d = d;
  s->queue_cap = (uint32_t)queue_cap;
  s->rec_words = (size_t)8 * d->g.L * d->g.F;
  const size_t nrec = 2 * (size_t)d->slots + kTurnoverBatch;
  auto fail = [&](int code) {
    (void)hipStreamSynchronize(d->stream);
    if (s->d_res) (void)hipFree(s->d_res);
    if (s->h_res) (void)hipHostFree(s->h_res);
    delete s->sch;
    delete s;
    return code;
  };
  if (hipMalloc(reinterpret_cast<void**>(&s->d_res), nrec * s->rec_words * sizeof(uint32_t)) != hipSuccess) return fail(LVA_ERR_NOMEM);
  if (hipHostMalloc(reinterpret_cast<void**>(&s->h_res), nrec * s->rec_words * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
    return fail(LVA_ERR_NOMEM);
  for (size_t i = nrec; i > 0; --i) s->free_rec.push_back((uint32_t)(i - 1));
  s->sch = new (std::nothrow) Schedule(d, (size_t)d->slots, s->d_res, false);   // (per-launch events are a batch call's: a stream has no last launch to sum at)
  if (!s->sch) return fail(LVA_ERR_NOMEM);
  s->sch->reset_profile();
  d->prof.h2d_ms = 0; d->prof.h2d_bytes = 0;
  std::memset(&s->h0, 0, sizeof s->h0);
  s->h0.cap = d->work_cap;
  hipError_t e = hipEventRecord(d->ev_total0, d->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d->d_work, &s->h0, sizeof s->h0, hipMemcpyHostToDevice, d->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d->d_slots, 0, (size_t)d->slots * sizeof(SlotDesc), d->stream);   // nblk = 0: no slot takes part yet
  if (e != hipSuccess) { g_hip_error = hipGetErrorString(e); return fail(LVA_ERR_HIP); }
  s->done_launch = d->launch_no;
  d->open_stream = s;
  *out = s;
  return LVA_OK;
}

int lva_stream_close(lva_stream* s) {
  if (!s) return LVA_ERR_ARG;
  lva_decoder* d = s->d;
  (void)hipSetDevice(d->device);
  // what is enqueued runs to its end (the pinned buffers below are targets and sources of its copies); reads that have not
  // finished are dropped: a later call re-initialises the slots it uses
  int st = LVA_OK;
  hipError_t e = hipSuccess;
  if (!s->sch->first_step) e = hipEventRecord(d->ev_step1, d->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&s->h1, d->d_work, sizeof s->h1, hipMemcpyDeviceToHost, d->stream);
  if (e == hipSuccess) e = hipEventRecord(d->ev_total1, d->stream);
  const hipError_t e_sync = hipStreamSynchronize(d->stream);
  if (e == hipSuccess) e = e_sync;
  if (e != hipSuccess) { g_hip_error = hipGetErrorString(e); st = LVA_ERR_HIP; }
  else st = s->sch->close_profile(s->h1);
  for (lva_stream::Mark& m : s->marks) (void)hipEventDestroy(m.ev);
  for (hipEvent_t ev : s->free_ev) (void)hipEventDestroy(ev);
  for (lva_stream::PostBuf& pb : s->bufs) { (void)hipFree(pb.dev); (void)hipHostFree(pb.host); }
  (void)hipFree(s->d_res);
  (void)hipHostFree(s->h_res);
  d->open_stream = nullptr;
  delete s->sch;
  delete s;
  return st;
}

int lva_stream_submit(lva_stream* s, const float* post, int64_t n_blocks, int32_t rc, uint64_t tag) {
  if (!s || n_blocks < 0 || n_blocks > 0xFFFFFFFFll || (n_blocks > 0 && !post)) return LVA_ERR_ARG;
  lva_decoder* d = s->d;
  const uint32_t npos = d->code[0].npos;
  if ((uint64_t)n_blocks < (uint64_t)npos + 1) {           // (:600-601) comes back from poll like every other read
    s->finished.push_back(lva_stream::Finished{tag, LVA_ERR_POST_TOO_SHORT, {}, {}});
    return LVA_OK;
  }
  if (s->queue.size() >= s->queue_cap) return LVA_ERR_BUSY;
  if (hipSetDevice(d->device) != hipSuccess) return LVA_ERR_NO_DEVICE;
  const uint32_t nb = (uint32_t)n_blocks, orient = rc ? 1u : 0u;
  int32_t buf = -1;
  { const int st = stream_take_buf(s, nb, &buf); if (st) return st; }
  const lva_stream::PostBuf& pb = s->bufs[(size_t)buf];
  std::memcpy(pb.host, post, (size_t)nb * 40 * sizeof(float));
  read_band_table(d, d->code[orient], nb, pb.host + (size_t)nb * 40);
  const hipError_t e = hipMemcpyAsync(pb.dev, pb.host, (size_t)nb * 41 * sizeof(uint32_t), hipMemcpyHostToDevice, d->stream);
  if (e != hipSuccess) {
    // (the buffer is not reused: whether the copy was enqueued is unknown; it is freed at close, behind the drain)
    g_hip_error = std::string("hipMemcpyAsync: ") + hipGetErrorString(e);
    return LVA_ERR_HIP;
  }
  d->prof.h2d_bytes += (uint64_t)nb * 40 * sizeof(float);
  int32_t id;
  if (!s->free_reads.empty()) { id = s->free_reads.back(); s->free_reads.pop_back(); }
  else { s->reads.emplace_back(); id = (int32_t)s->reads.size() - 1; }
  lva_stream::Read& r = s->reads[(size_t)id];
  r.tag = tag; r.buf = buf; r.nblk = nb; r.orient = orient; r.rec = 0; r.gathered = false;
  s->queue.push_back(id);
  return LVA_OK;
}

int lva_stream_poll(lva_stream* s, int32_t wait, int32_t max_reads, uint64_t* tags, uint8_t* out_msgs, float* out_scores,
                    int32_t* out_counts, int32_t* n_out) {
  if (!s || !n_out || max_reads < 0 || (max_reads > 0 && (!tags || !out_msgs || !out_counts))) return LVA_ERR_ARG;
  *n_out = 0;
  lva_decoder* d = s->d;
  if (hipSetDevice(d->device) != hipSuccess) return LVA_ERR_NO_DEVICE;
  const size_t row = (size_t)d->g.L * d->code[0].msg_len;
  bool block = false;
  for (;;) {
    { const int st = stream_reap(s, block); if (st) return st; }
    { const int st = stream_pump(s); if (st) return st; }
    if (!block) { const int st = stream_reap(s, false); if (st) return st; }   // (what finished while the launches were enqueued)
    if (!s->finished.empty() || !wait || max_reads == 0) break;
    if (s->marks.empty()) break;       // nothing pending: every read handed in has been handed out
    block = true;                      // wait = 1: sleep on the oldest mark, then look again
  }
  int32_t k = 0;
  while (k < max_reads && !s->finished.empty()) {
    lva_stream::Finished& f = s->finished.front();
    tags[k] = f.tag;
    out_counts[k] = f.count;
    if (f.count > 0) {
      std::memcpy(out_msgs + (size_t)k * row, f.msgs.data(), (size_t)f.count * d->code[0].msg_len);
      if (out_scores) std::memcpy(out_scores + (size_t)k * d->g.L, f.scores.data(), (size_t)f.count * sizeof(float));
    }
    s->finished.pop_front();
    ++k;
  }
  *n_out = k;
  return LVA_OK;
}

int lva_stream_pending(const lva_stream* s, int32_t* queued, int32_t* in_slots, int32_t* finished) {
  if (!s) return LVA_ERR_ARG;
  if (queued) *queued = (int32_t)s->queue.size();
  if (in_slots) *in_slots = (int32_t)(s->sch->active + s->in_marks);
  if (finished) *finished = (int32_t)s->finished.size();
  return LVA_OK;
}

int lva_decode_batch_device(lva_decoder* d, const float* post_dev, const int64_t* row_offsets, int32_t n_reads,
                            const uint8_t* rc_flags, uint8_t* out_msgs, float* out_scores, int32_t* out_counts) {
  if (!d || n_reads < 0 || !row_offsets || (n_reads > 0 && (!post_dev || !out_msgs || !out_counts))) return LVA_ERR_ARG;
  if (d->open_stream) return LVA_ERR_BUSY;   // a stream owns the slots, the work list and the profile
  if (hipSetDevice(d->device) != hipSuccess) return LVA_ERR_NO_DEVICE;
  std::vector<int64_t> len((size_t)n_reads);
  for (int32_t i = 0; i < n_reads; ++i) len[i] = row_offsets[i + 1] - row_offsets[i];
  return decode_impl(d, post_dev, row_offsets, len.data(), n_reads, rc_flags, out_msgs, out_scores, out_counts, false);
}

int lva_decode_windows_device(lva_decoder* d, const float* post_dev, const int64_t* first_block, const int64_t* n_blocks,
                              int32_t n_reads, const uint8_t* rc_flags, uint8_t* out_msgs, float* out_scores,
                              int32_t* out_counts) {
  if (!d || n_reads < 0 || (n_reads > 0 && (!post_dev || !first_block || !n_blocks || !out_msgs || !out_counts))) return LVA_ERR_ARG;
  if (d->open_stream) return LVA_ERR_BUSY;   // a stream owns the slots, the work list and the profile
  if (hipSetDevice(d->device) != hipSuccess) return LVA_ERR_NO_DEVICE;
  return decode_impl(d, post_dev, first_block, n_blocks, n_reads, rc_flags, out_msgs, out_scores, out_counts, false);
}

int lva_decode_batch(lva_decoder* d, const float* post, const int64_t* row_offsets, int32_t n_reads,
                     const uint8_t* rc_flags, uint8_t* out_msgs, float* out_scores, int32_t* out_counts) {
  if (!d || n_reads < 0 || !row_offsets || (n_reads > 0 && (!post || !out_msgs || !out_counts))) return LVA_ERR_ARG;
  if (d->open_stream) return LVA_ERR_BUSY;   // a stream owns the slots, the work list and the profile
  if (hipSetDevice(d->device) != hipSuccess) return LVA_ERR_NO_DEVICE;
  const int64_t blocks = n_reads > 0 ? row_offsets[n_reads] : 0;
  if (blocks < 0) return LVA_ERR_ARG;
  HostPost hp;                               // freed on every exit below, each behind a drained stream
  const size_t bytes = (size_t)std::max<int64_t>(blocks, 1) * 40 * sizeof(float);
  HIP_TRY(hipMalloc(&hp.dev, bytes));
  hipError_t e = hipEventRecord(d->ev_total0, d->stream);
  if (e == hipSuccess && blocks > 0)
    e = hipMemcpyAsync(hp.dev, post, (size_t)blocks * 40 * sizeof(float), hipMemcpyHostToDevice, d->stream);
  if (e == hipSuccess) e = hipEventRecord(d->ev_h2d, d->stream);
  if (e != hipSuccess) { g_hip_error = hipGetErrorString(e); (void)hipStreamSynchronize(d->stream); return LVA_ERR_HIP; }
  std::vector<int64_t> len((size_t)n_reads);
  for (int32_t i = 0; i < n_reads; ++i) len[i] = row_offsets[i + 1] - row_offsets[i];
  const int st = decode_impl(d, hp.dev, row_offsets, len.data(), n_reads, rc_flags, out_msgs, out_scores, out_counts, true);
  (void)hipStreamSynchronize(d->stream);
  float ms = 0;
  d->prof.h2d_ms = (st == LVA_OK && hipEventElapsedTime(&ms, d->ev_total0, d->ev_h2d) == hipSuccess) ? ms : 0.0;
  d->prof.h2d_bytes = (uint64_t)blocks * 40 * sizeof(float);
  return st;
}

int lva_device_alloc(lva_decoder* d, uint64_t bytes, void** out_dev_ptr) {
  if (!d || !out_dev_ptr) return LVA_ERR_ARG;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipMalloc(out_dev_ptr, (size_t)std::max<uint64_t>(bytes, 1)));
  return LVA_OK;
}

int lva_device_free(lva_decoder* d, void* dev_ptr) {
  if (!d) return LVA_ERR_ARG;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipFree(dev_ptr));
  return LVA_OK;
}

int lva_device_upload(lva_decoder* d, void* dev_dst, const void* host_src, uint64_t bytes) {
  if (!d || (bytes && (!dev_dst || !host_src))) return LVA_ERR_ARG;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipMemcpyAsync(dev_dst, host_src, (size_t)bytes, hipMemcpyHostToDevice, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return LVA_OK;
}

int lva_device_download(lva_decoder* d, void* host_dst, const void* dev_src, uint64_t bytes) {
  if (!d || (bytes && (!host_dst || !dev_src))) return LVA_ERR_ARG;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipMemcpyAsync(host_dst, dev_src, (size_t)bytes, hipMemcpyDeviceToHost, d->stream));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return LVA_OK;
}

int lva_device_synchronize(lva_decoder* d) {
  if (!d) return LVA_ERR_ARG;
  HIP_TRY(hipSetDevice(d->device));
  HIP_TRY(hipStreamSynchronize(d->stream));
  return LVA_OK;
}

}  // extern "C"
