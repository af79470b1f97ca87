// windingkernel.h -- launch interface of windingkernel.hip (winding-number queries, pt_winding.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_winding.h"

namespace pt {

struct WindingArgs {
  SceneView scene;                // the references come from scene.nodes (Node128) whatever scene.nodes64 says: no box is read
  const WindingNode* table;       // the moments, one record per node (device); null in a scene without nodes
  const float* points;            // n x 4 floats x y z beta, 16-byte aligned (device)
  float* out;                     // n x float (device)
  int n;                          // queries of this launch (the host cuts longer batches: indices stay 32-bit)
  int* stackOverflow;             // per-thread spill area (one entry per int) for trees deeper than the LDS stack, or null
};
constexpr int kWindingMaxLaunch = 1 << 30;      // queries per launch, the point kernel's
constexpr int kWindingMaxNodes = 1 << 25;       // 4 * node + slot is a stack entry, and 32 x that a 32-bit byte offset into the table

size_t windingkernel_overflow_ints(int nBlocks, int stackBound);      // 0 = the tree fits the LDS stack
// Launches min(nBlocks, ceil(n / 256)) workgroups on `stream`.
hipError_t launch_windingquery(hipStream_t stream, const WindingArgs& a, int nBlocks);

// One level of the moments table: the nodes levelOrder[first .. first + count), whose node children must be finished already (deepest
// level first).  tris, nodes: the tree as it is now (after a refit: the refitted boxes).
struct WindingTableArgs {
  const Node128* nodes; const Tri48* tris; const int* levelOrder;
  WindingNode* table;
};
hipError_t launch_winding_level(hipStream_t stream, const WindingTableArgs& a, int first, int count);

}  // namespace pt
