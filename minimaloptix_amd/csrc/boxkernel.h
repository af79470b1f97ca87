// boxkernel.h -- launch interface of boxkernel.hip (box overlap queries, pt_box.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_box.h"

namespace pt {

struct BoxArgs {
  SceneView scene;                // nodes64 set = walk the 64-byte nodes
  const float* boxes;             // n x 6 floats lox loy loz hix hiy hiz, 8-byte aligned (device)
  int* out;                       // any: n x int32 |S| > 0; count and list: n x int32 |S| (device)
  const long long* offsets;       // list: n + 1 entries of this launch into prims, 8-byte aligned (device); else null
  int* prims;                     // list: the caller's whole prims array (the offsets are absolute); else null
  int n;                          // boxes of this launch (the host cuts longer batches: indices stay 32-bit)
  int* stackOverflow;             // per-thread spill area (one reference per entry) for trees deeper than the LDS stack, or null
};
constexpr int kBoxMaxLaunch = 1 << 30;      // boxes per launch

size_t boxkernel_overflow_ints(int nBlocks, int stackBound);      // 0 = the tree fits the LDS stack
// mode: BOX_ANY / BOX_COUNT / BOX_LIST (pt_box.h).  Launches min(nBlocks, ceil(n / 256)) workgroups on `stream`.
hipError_t launch_boxquery(hipStream_t stream, const BoxArgs& a, int nBlocks, int mode);

}  // namespace pt
