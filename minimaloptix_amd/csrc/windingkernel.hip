// windingkernel.hip -- winding-number queries (pt_winding.h) for gfx950: the generalised winding number of the caller's points, and
// the table of cluster moments its far field reads.
//
// Its own translation unit, as the other query kernels': nothing of this pass is compiled into another kernel.
//
// pt_windingquery.  Execution model: the point queries' (pointkernel.hip).  One point per lane, walked to its end with the if-if step
// (pt_winding.h winding_step).  The grid is ceil(n / 256) workgroups up to a cap of CUs x blocksPerCU; past the cap a lane goes on to the
// point one grid further (grid-stride loop), so the stack overflow area is sized by the cap, not by n, and a result goes to its point's
// own index: nothing depends on the scheduling.  A point is read as one 16-byte load, a result written as one 4-byte store.  The
// traversal stack holds entries of four bytes (4 x node + slot): 16 per lane in LDS ([entry][lane], 16 KB per workgroup) with a
// global overflow column per thread.  The accumulator is one binary64 register pair per lane; no atomics, no cross-lane traffic.
//
// k_winding_level.  One thread per node of one level of the emitted tree, deepest level first (one launch per level, the refit's
// plan): a node child's sums read the records the launch before wrote.  Plain loads and stores: the table is written here, so
// nothing of it goes through load_const in this kernel.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_lanestack.h"
#include "pt_winding.h"
#include "windingkernel.h"

namespace pt {

namespace {

constexpr int kBlockThreads = 256;
constexpr int kWavesPerBlock = kBlockThreads / 64;
constexpr int kLdsStack = 16;          // entries per lane kept in LDS (4 bytes each: 16 KB per workgroup)

using WindingStack = LaneStack<kLdsStack, int>;

__global__ void __launch_bounds__(kBlockThreads) pt_windingquery(const WindingArgs a) {
  __shared__ int ldsStack[kWavesPerBlock * kLdsStack * 64];
  const SceneView& sc = a.scene;
  const int gthread = blockIdx.x * kBlockThreads + threadIdx.x, stride = gridDim.x * kBlockThreads;
  WindingStack st;
  st.init(ldsStack, a.stackOverflow, gthread, stride);
  const uint4* __restrict__ points = reinterpret_cast<const uint4*>(a.points);
  for (int i = gthread; i < a.n; i += stride) {           // n <= kWindingMaxLaunch = 2^30 and stride <= 2^22: no overflow
    const uint4 r = points[(size_t)i];
    const float p[4] = { i2f((int32_t)r.x), i2f((int32_t)r.y), i2f((int32_t)r.z), i2f((int32_t)r.w) };
    a.out[i] = winding_query(sc, a.table, p, st);
  }
}

__global__ void __launch_bounds__(kBlockThreads) k_winding_level(const WindingTableArgs a, int first, int count) {
  const int i = blockIdx.x * kBlockThreads + threadIdx.x;
  if (i >= count) return;
  const int n = a.levelOrder[first + i];
  a.table[n] = winding_node(a.nodes[n], a.nodes, a.tris, a.table);
}

}  // namespace

size_t windingkernel_overflow_ints(int nBlocks, int stackBound) { return lane_stack_overflow_entries((size_t)nBlocks * kBlockThreads, stackBound, kLdsStack); }

hipError_t launch_windingquery(hipStream_t stream, const WindingArgs& a, int nBlocks) {
  const int blocks = (int)std::min<long long>(nBlocks, ((long long)a.n + kBlockThreads - 1) / kBlockThreads);
  pt_windingquery<<<blocks, kBlockThreads, 0, stream>>>(a);
  return hipGetLastError();
}

hipError_t launch_winding_level(hipStream_t stream, const WindingTableArgs& a, int first, int count) {
  if (count <= 0) return hipSuccess;
  k_winding_level<<<(count + kBlockThreads - 1) / kBlockThreads, kBlockThreads, 0, stream>>>(a, first, count);
  return hipGetLastError();
}

}  // namespace pt
