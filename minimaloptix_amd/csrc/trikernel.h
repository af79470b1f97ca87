// trikernel.h -- launch interface of trikernel.hip (triangle queries, pt_tri.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_tri.h"

namespace pt {

struct TriArgs {
  SceneView scene;                // nodes64 set = walk the 64-byte nodes
  const float* tris;              // n x 9 floats (pt_tri.h), 4-byte aligned (device)
  int* out;                       // any: n x int32 |S| > 0; count and list: n x int32 |S| (device)
  const long long* offsets;       // list: n + 1 entries of this launch into prims, 8-byte aligned (device); else null
  int* prims;                     // list: the caller's whole prims array (the offsets are absolute); else null
  int n;                          // queries of this launch (the host cuts longer batches: indices stay 32-bit)
  int* stackOverflow;             // per-thread spill area (one reference per entry) for trees deeper than the LDS stack, or null
};
constexpr int kTriMaxLaunch = 1 << 30;      // queries per launch

size_t trikernel_overflow_ints(int nBlocks, int stackBound);      // 0 = the tree fits the LDS stack
// mode: BOX_ANY / BOX_COUNT / BOX_LIST (pt_box.h).  Launches min(nBlocks, ceil(n / 256)) workgroups on `stream`.
hipError_t launch_triquery(hipStream_t stream, const TriArgs& a, int nBlocks, int mode);

}  // namespace pt
