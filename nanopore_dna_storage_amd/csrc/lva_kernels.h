// lva_kernels.h -- launchers of the HIP kernels in lva_kernels.hip (stream passed as void*).
#pragma once
#include "lva_device.h"
#include "lva_plan.h"

namespace lva {

// one whole step: the plan's dominant kernel, then its fix-up pass over the work list (hdr, items) where it has one.
// ev_mid (a hipEvent_t or nullptr) is recorded between the two
int launch_step(const Plan& plan, const StepArgs& a, const Geometry& g, const DevCode* codes, uint32_t* trellis, WorkHdr* hdr,
                uint32_t* items, void* stream, void* ev_mid);
// this launch's SlotStep records (a.steps), to be enqueued right before the step launch
int launch_prepare_step(const StepArgs& a, const DevCode* codes, SlotStep* steps, void* stream);
// initial scores of up to kTurnoverBatch slots + their descriptors (the reads enter their slots); no launch for an empty batch
int launch_init_slots(const Geometry& g, const DevCode* codes, uint32_t* trellis, const InitBatch& batch, SlotDesc* slots, void* stream);
// the final lists of up to kTurnoverBatch finished reads -> their result records
int launch_gather_finals(const Geometry& g, const DevCode* codes, const uint32_t* trellis, const GatherBatch& batch,
                         uint32_t* results, void* stream);

}  // namespace lva
