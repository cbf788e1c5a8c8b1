// lva_host.h -- what the host files of the library share: lva_api.cpp (decoder, schedule, decode stream) and
// lva_stages.cpp (the stages beside the decoder).  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/lva_decoder.h"
#include "lva_code.h"
#include "lva_device.h"
#include "lva_plan.h"

namespace lva {
// the text lva_last_hip_error returns on the calling thread (lva_api.cpp owns it)
void set_hip_error(const std::string& text);

// a kernel launcher's return (0 or a hipError_t) as an LVA_* code
inline int launch_status(int e) {
  if (!e) return LVA_OK;
  set_hip_error(hipGetErrorString((hipError_t)e));
  return LVA_ERR_HIP;
}
}  // namespace lva

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e__ = (expr);                                                                   \
    if (e__ != hipSuccess) {                                                                   \
      ::lva::set_hip_error(std::string(#expr) + ": " + hipGetErrorString(e__));                \
      return LVA_ERR_HIP;                                                                      \
    }                                                                                          \
  } while (0)

struct lva_stream;

struct lva_decoder {
  lva_config cfg{};
  std::string sync_marker;
  lva::Code code[2];           // forward, reverse complement
  uint32_t max_dev = 0;
  lva::Plan plan{};           // which step kernel runs, on which layout (plan_kernels): decided in lva_decoder_create
  lva::Geometry g{};
  int slots = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_total0 = nullptr, ev_total1 = nullptr, ev_step0 = nullptr, ev_step1 = nullptr, ev_h2d = nullptr;
  lva::DevCode* d_codes = nullptr;
  uint16_t* d_predtab = nullptr;
  uint32_t* d_trellis = nullptr;
  uint32_t* d_results = nullptr;
  size_t results_cap = 0;      // reads
  lva::SlotDesc* d_slots = nullptr; // [slots]
  lva::SlotStep* d_steps = nullptr; // [slots] this launch's time step of every slot (lva_prepare_step)
  uint32_t* d_band = nullptr;  // band tables of the batch in flight: lo | hi << 16 per (read, time step)
  size_t band_cap = 0;         // words
  lva::WorkHdr* d_work = nullptr;   // header followed by the item array
  uint32_t work_cap = 1u << 20;
  uint32_t launch_no = 0;      // trellis-step launches since creation (the slots' clock)
  uint32_t full_lo = 1, full_hi = 0;   // positions at which every 64-source tile has a valid target (StepArgs::full_lo/hi)
  int launch_events = 0;       // lva_decoder_set_launch_events
  std::vector<hipEvent_t> ev_pool;
  lva_profile prof{};
  lva_stream* open_stream = nullptr;   // lva_stream_open .. lva_stream_close: the batch entry points refuse meanwhile
  float* d_tp_fwd = nullptr;   // lva_transpost_*: forward vectors, 8 floats per block; grows, never shrinks
  size_t tp_fwd_cap = 0;       // blocks
  int64_t* d_tp_off = nullptr; // lva_transpost_*: row offsets of the batch
  size_t tp_off_cap = 0;       // entries
};

namespace lva {
// The two below serve lva_api.cpp's decode path alone; a side stage owns its stream, allocation and drain through one
// Frame (lva_stages.cpp), whose destructor keeps the order that these two leave to their caller.
//
// From its construction on, every exit of a call leaves with the stream drained: pending copies read and write host buffers
// and device blocks that die with the call's frame.  Construct it before the first asynchronous call and AFTER every such
// buffer and block (locals are destroyed in reverse order).
struct StreamDrain {
  hipStream_t s;
  bool armed = true;
  explicit StreamDrain(hipStream_t st) : s(st) {}
  ~StreamDrain() { if (armed && s) (void)hipStreamSynchronize(s); }
  int finish() {               // the success exit: wait, and report what the wait reports
    armed = false;
    HIP_TRY(hipStreamSynchronize(s));
    return LVA_OK;
  }
};

// a device copy of the caller's host posteriors for the length of lva_decode_batch
struct HostPost {
  float* dev = nullptr;
  ~HostPost() { if (dev) (void)hipFree(dev); }
};
}  // namespace lva
