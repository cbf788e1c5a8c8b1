// lva_plan.h -- which step kernel runs for a configuration, and on which memory layout.  plan_kernels decides it once:
// lva_decoder_create builds the geometry from the plan, launch_step (lva_kernels.hip) switches on it, the schedule reads its
// flags.  No other place in the tree names a list-size class.  Host only, no HIP types.
#pragma once
#include <cstdint>

#include "../../include/lva_decoder.h"

namespace lva {

enum class StepKernel { Exact, Wave, WaveWide, Acs, Fast, Lazy, Big, BigRec };   // LVA_STEP_* of lva_kernel_plan_info, in order
enum class Fixup { None, Wave, Lazy };                                           // LVA_FIXUP_*

struct Plan {
  int mode;                  // the kernel mode of include/lva_decoder.h that runs (lva_profile.kernel): 1..4
  StepKernel dominant;
  Fixup fixup;               // the exact pass over the dominant kernel's work list
  uint32_t lazy, rec, cmp;   // Geometry's layout flags, taken as they are by make_geometry
  uint32_t ring_extra;       // ring positions = min(npos, 2 max_deviation + ring_extra), at least 1
  int inst;                  // template instance: LL of Big (16, 32, 64) and BigRec (32, 64), R = ceil(L / 64) of WaveWide, else 0
};

// request: lva_config.kernel; L: 1..65535 (the caller's check); msg_bits: msg_len + mem_conv.
// LVA_OK, LVA_ERR_UNSUPPORTED (a mode the list size has no kernel for) or LVA_ERR_ARG (no such mode).
inline int plan_kernels(int32_t request, uint32_t L, uint32_t msg_bits, Plan* out) {
  if (request < 0 || request > 4) return LVA_ERR_ARG;
  const bool small = L == 2 || L == 4 || L == 8;   // the list sizes lva_step_fast and lva_step_lazy are instantiated for
  Plan p{1, StepKernel::Exact, Fixup::None, 0, 0, 0, 1, 0};
  if (request == 1 || (request == 0 && L > 64)) {
    // one thread per target; the default above 64 entries (mode 3 there is on request only: DESIGN.md 4)
  } else if (request == 3) {
    if (L < 2 || L > 256) return LVA_ERR_UNSUPPORTED;
    p.mode = 3;
    p.dominant = L <= 64 ? StepKernel::Wave : StepKernel::WaveWide;
    p.inst = L <= 64 ? 0 : (int)((L + 63) / 64);   // register rows of 64 entries
  } else if (request == 4 || (request == 0 && small)) {
    // Lazy messages: materialised every second time step and carried as one-byte back-pointers in between; two-hop chains
    // reach one position further below the band, hence one more ring position.  The default at its list sizes (m = 11 L = 8:
    // +5 % over mode 2, m = 8: +9 %; m = 14 with four message planes: +8 % since the anchor instance keeps one entry in flight).
    if (!small) return LVA_ERR_UNSUPPORTED;
    p = Plan{4, StepKernel::Lazy, Fixup::Lazy, 1, 0, 1, 2, 0};
  } else {                                          // mode 2, asked for or the default: the fast kernels and their fix-up
    if (L > 64) return LVA_ERR_UNSUPPORTED;
    p.mode = 2;
    if (L == 1) {                                   // no ties to resolve, no work list
      p.dominant = StepKernel::Acs; p.cmp = 1;
    } else if (small) {
      p.dominant = StepKernel::Fast; p.fixup = Fixup::Wave;
    } else if ((msg_bits + 63) / 64 == 3 && L >= 32 && L % 4 == 0) {
      // record layout: three message planes, L a multiple of 4 (below 32 entries the plane layout is faster: measured).  It keeps
      // a list's entries together, so a compact list that does not exist would be a hole of whole lines: cmp stays 0
      p.dominant = StepKernel::BigRec; p.fixup = Fixup::Wave; p.rec = 1; p.inst = L <= 32 ? 32 : 64;
    } else {
      p.dominant = StepKernel::Big; p.fixup = Fixup::Wave; p.cmp = 1; p.inst = L <= 16 ? 16 : L <= 32 ? 32 : 64;
    }
  }
  *out = p;
  return LVA_OK;
}

}  // namespace lva
