// aovkernel.h -- launch interface of aovkernel.hip (first-hit AOVs, pt_aov.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_types.h"

namespace pt {

struct AovArgs {
  SceneView scene;                  // whole frame (the AOVs ignore moptix_set_partition)
  const int* seeds; int nSeeds;     // launch seeds (device memory), added in this order
  int writeIds;                     // 1: first call after a clear -- primId / matId come from its first seed
  float* albedo; float* normal;     // float3 W*H, row 0 = bottom (the accumulation buffer's layout)
  float* depth; float* hits;        // float W*H
  int* primId; int* matId;          // int32 W*H
  int* stackOverflow;               // per-thread spill area for trees deeper than the LDS stack (or null)
};

int aovkernel_threads(int nCUs);    // threads of a launch (the overflow area holds aovkernel_overflow_ints of them)
size_t aovkernel_overflow_ints(int nCUs, int stackBound);
// node64: walk scene.nodes64 (must be non-null) instead of scene.nodes.  tileCounter: one int of device memory, the waves' tile
// counter (zeroed on the stream by the launch).  a.stackOverflow must hold aovkernel_overflow_ints(nCUs, stackBound) ints.
hipError_t launch_aovkernel(hipStream_t stream, const AovArgs& a, int nCUs, int* tileCounter, bool node64);

}  // namespace pt
