// sweepkernel.h -- launch interface of sweepkernel.hip (sphere sweep queries, pt_sweep.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_sweep.h"

namespace pt {

struct SweepArgs {
  SceneView scene;                      // nodes64 set = walk the 64-byte nodes
  const float* sweeps;                  // n x 8 floats ox oy oz dx dy dz radius tmax, 16-byte aligned (device)
  void* out;                            // closest: n x SweepHit, 16-byte aligned; any: n x int32 (device)
  int n;                                // sweeps of this launch (the host cuts longer batches: indices stay 32-bit)
  unsigned long long* stackOverflow;    // per-thread spill area (reference + entry time) for trees deeper than the LDS stack, or null
};
constexpr int kSweepMaxLaunch = 1 << 30;      // sweeps per launch

size_t sweepkernel_overflow_entries(int nBlocks, int stackBound);      // 0 = the tree fits the LDS stack
// mode: SWEEP_CLOSEST / SWEEP_ANY (pt_sweep.h).  Launches min(nBlocks, ceil(n / 256)) workgroups on `stream`.
hipError_t launch_sweepquery(hipStream_t stream, const SweepArgs& a, int nBlocks, int mode);

}  // namespace pt
