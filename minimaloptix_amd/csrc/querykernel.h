// querykernel.h -- launch interface of querykernel.hip (batched ray queries, pt_query.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_types.h"

namespace pt {

struct QueryArgs {
  SceneView scene;                // nodes64 set = walk the 64-byte nodes
  const float* rays;              // n x 8 floats, 16-byte aligned (device)
  void* out;                      // closest: n x QueryHit (16-byte aligned); any: n x int32 (device)
  int n;                          // rays of this launch (the host cuts longer batches: indices stay 32-bit)
  int* stackOverflow;             // per-thread spill area for trees deeper than the LDS stack (or null), sized for the grid's cap
};
// multi-hit (pt_multihit.h): a struct of its own, so that the kernels above keep their arguments
struct MultiArgs {
  SceneView scene;
  const float* rays;              // n x 8 floats, 16-byte aligned (device)
  void* hits;                     // n x maxHits QueryHit, ray-major, 16-byte aligned (device); null with maxHits 0
  int* counts;                    // n x int32 (device)
  int n;                          // rays of this launch: n x max(maxHits, 1) <= kQueryMaxLaunch
  int maxHits;                    // 0..64; 0 only with countAll
  int* stackOverflow;             // as QueryArgs'
};
constexpr int kQueryMaxLaunch = 1 << 30;      // rays per launch

int querykernel_blocks(int nCUs, int blocksPerCU);      // the grid's cap, of the radiance and point queries too (api_core.hip fill_query_view)
size_t querykernel_overflow_ints(int nBlocks, int stackBound);     // 0 = the tree fits the LDS stack
// mode: QUERY_CLOSEST / QUERY_ANY (pt_query.h).  Launches min(nBlocks, ceil(n / 256)) workgroups on `stream`.
hipError_t launch_rayquery(hipStream_t stream, const QueryArgs& a, int nBlocks, int mode);
// countAll: counts = |H| and the walk does not prune; else counts = min(maxHits, |H|).  The same grid.
hipError_t launch_rayquery_multi(hipStream_t stream, const MultiArgs& a, int nBlocks, bool countAll);

}  // namespace pt
