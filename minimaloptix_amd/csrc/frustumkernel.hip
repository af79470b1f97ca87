// frustumkernel.hip -- frustum queries (pt_frustum.h) for gfx950: does anything meet the caller's six-plane region, how many primitives
// do, and which.
//
// Its own translation unit, as the box kernels': nothing of this pass is compiled into another kernel.
//
// Execution model: the box queries' (boxkernel.hip).  One query per lane, walked to its end with the if-if step (pt_frustum.h
// frustum_step).  The grid is ceil(n / 256) workgroups up to a cap of CUs x blocksPerCU; past the cap a lane goes on to the query one grid
// further (grid-stride loop), so the stack overflow area is sized by the cap, not by n, and a result goes to its query's own index:
// nothing depends on the scheduling.  A query is read as six 16-byte loads; the 24 plane floats and the six nb_j stay in registers (the
// absolute values are source modifiers, and the six len_j are dead once the spheres in front of the walk are done), so the lane's LDS
// row holds its stack alone.  The traversal stack holds child references alone, four bytes an entry: 16 entries per lane in LDS
// ([entry][lane], 16 KB per workgroup) with a global overflow column per thread.  The list is the box queries': appended to the query's
// own slice, heap-sorted there.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_lanestack.h"
#include "pt_frustum.h"
#include "frustumkernel.h"

namespace pt {

namespace {

constexpr int kBlockThreads = 256;
constexpr int kWavesPerBlock = kBlockThreads / 64;
constexpr int kLdsStack = 16;          // entries per lane kept in LDS (4 bytes each: 16 KB per workgroup)

using FrustumStack = LaneStack<kLdsStack, int>;

template <int MODE, bool N64>
__global__ void __launch_bounds__(kBlockThreads) pt_frustumquery(const FrustumArgs a) {
  __shared__ int ldsStack[kWavesPerBlock * kLdsStack * 64];
  const SceneView& sc = a.scene;
  const int gthread = blockIdx.x * kBlockThreads + threadIdx.x, stride = gridDim.x * kBlockThreads;
  FrustumStack st;
  st.init(ldsStack, a.stackOverflow, gthread, stride);
  const float4* frusta = reinterpret_cast<const float4*>(a.frusta);
  for (int i = gthread; i < a.n; i += stride) {           // n <= kFrustumMaxLaunch = 2^30 and stride <= 2^22: no overflow
    const float4* row = frusta + 6 * (size_t)i;
    const float4 f0 = row[0], f1 = row[1], f2 = row[2], f3 = row[3], f4 = row[4], f5 = row[5];
    const float f[24] = { f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w, f2.x, f2.y, f2.z, f2.w,
                          f3.x, f3.y, f3.z, f3.w, f4.x, f4.y, f4.z, f4.w, f5.x, f5.y, f5.z, f5.w };
    const Frustum q = frustum_make(f);
    BoxOut o;
    o.slice = nullptr; o.cap = 0; o.count = 0;
    if constexpr (MODE == BOX_LIST) {
      const long long first = a.offsets[i], cap = a.offsets[(size_t)i + 1] - first;
      o.slice = a.prims + first; o.cap = cap > 0 ? cap : 0;
    }
    BoxTrav tv;
    frustum_begin<MODE>(sc, q, frustum_valid(f), tv, o);
    while (tv.node != kTravDone) frustum_step<MODE, N64>(sc, q, tv, st, o);
    if constexpr (MODE == BOX_LIST) box_list_finish(o);
    a.out[i] = MODE == BOX_ANY ? (o.count > 0 ? 1 : 0) : o.count;
  }
}

template <int MODE>
void launch_mode(hipStream_t stream, const FrustumArgs& a, int blocks) {
  if (a.scene.nodes64 != nullptr) pt_frustumquery<MODE, true><<<blocks, kBlockThreads, 0, stream>>>(a);
  else                            pt_frustumquery<MODE, false><<<blocks, kBlockThreads, 0, stream>>>(a);
}

}  // namespace

size_t frustumkernel_overflow_ints(int nBlocks, int stackBound) { return lane_stack_overflow_entries((size_t)nBlocks * kBlockThreads, stackBound, kLdsStack); }

hipError_t launch_frustumquery(hipStream_t stream, const FrustumArgs& a, int nBlocks, int mode) {
  const int blocks = (int)std::min<long long>(nBlocks, ((long long)a.n + kBlockThreads - 1) / kBlockThreads);
  if (mode == BOX_LIST) launch_mode<BOX_LIST>(stream, a, blocks);
  else if (mode == BOX_COUNT) launch_mode<BOX_COUNT>(stream, a, blocks);
  else launch_mode<BOX_ANY>(stream, a, blocks);
  return hipGetLastError();
}

}  // namespace pt
