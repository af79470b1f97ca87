// pointkernel.h -- launch interface of pointkernel.hip (closest-point queries, pt_point.h, their signed mode, pt_sign.h, and the K-nearest
// queries, pt_pointmulti.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_sign.h"

namespace pt {

struct PointArgs {
  SceneView scene;                // nodes64 set = walk the 64-byte nodes
  const float* points;            // n x 4 floats x y z maxDist, 16-byte aligned (device)
  void* out;                      // closest: n x PointHit (16-byte aligned); any: n x int32 (device)
  int n;                          // points of this launch (the host cuts longer batches: indices stay 32-bit)
  unsigned long long* stackOverflow;   // per-thread spill area (reference + box distance per entry) for trees deeper than the LDS stack, or null
};
struct PointSignedArgs {          // what the signed mode's kernel takes
  PointArgs p;                    // out: n x PointHit
  const SignRecord* table;        // one record per original face id; may be null in a scene without triangles
};
// K nearest (pt_pointmulti.h): a struct of its own, so that the kernels above keep their arguments
struct PointMultiArgs {
  SceneView scene;
  const float* points;            // n x 4 floats x y z maxDist, 16-byte aligned (device)
  void* hits;                     // n x maxNear PointHit, query-major, 16-byte aligned (device); null with maxNear 0
  int* counts;                    // n x int32 (device)
  int n;                          // points of this launch: n x max(maxNear, 1) <= kPointMaxLaunch
  int maxNear;                    // 0..64; 0 only with countAll
  unsigned long long* stackOverflow;   // the point queries' area, as PointArgs'
};
constexpr int kPointMaxLaunch = 1 << 30;      // points per launch; of the K-nearest queries: records per launch

size_t pointkernel_overflow_entries(int nBlocks, int stackBound);     // 8-byte entries; 0 = the tree fits the LDS stack
// mode: POINT_CLOSEST / POINT_ANY (pt_point.h) / POINT_SIGNED (pt_sign.h).  table: the signed mode's; null for the other two and for a
// scene without triangles.  Launches min(nBlocks, ceil(n / 256)) workgroups on `stream`.
hipError_t launch_pointquery(hipStream_t stream, const PointArgs& a, const SignRecord* table, int nBlocks, int mode);
// countAll: counts = |S| and the walk prunes at r2 alone; else counts = min(maxNear, |S|).  The same grid.
hipError_t launch_pointquery_multi(hipStream_t stream, const PointMultiArgs& a, int nBlocks, bool countAll);

}  // namespace pt
