// trikernel.hip -- triangle queries (pt_tri.h) for gfx950: does anything meet the caller's triangle, how many primitives do, and which.
//
// Its own translation unit, as the box kernel's: nothing of this pass is compiled into another kernel.
//
// Execution model: the box queries' (boxkernel.hip).  One query per lane, walked to its end with the if-if step (pt_tri.h tri_step; the
// node step is pt_box.h's own against the query's box).  The grid is ceil(n / 256) workgroups up to a cap of CUs x blocksPerCU; past the
// cap a lane goes on to the query one grid further (grid-stride loop), so the stack overflow area is sized by the cap, not by n, and a
// result goes to its query's own index: nothing depends on the scheduling.  A query is read as nine dword loads (36 bytes a query: not
// float4-aligned); its box, its edges, its normal and the in-plane edge normals are computed once, in front of the walk.
// The traversal stack holds child references alone, four bytes an entry: 16 entries per lane in LDS ([entry][lane], 16 KB per workgroup)
// with a global overflow column per thread.  The list is the box queries': appended to the query's own slice, heap-sorted there.
// The leaf step holds one copy of the 23-axis test; its three groups of axes end early where a group has separated the pair, which
// changes no result (the predicate is the OR over all 23).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_lanestack.h"
#include "pt_tri.h"
#include "trikernel.h"

namespace pt {

namespace {

constexpr int kBlockThreads = 256;
constexpr int kWavesPerBlock = kBlockThreads / 64;
constexpr int kLdsStack = 16;          // entries per lane kept in LDS (4 bytes each: 16 KB per workgroup)

using TriStack = LaneStack<kLdsStack, int>;

template <int MODE, bool N64>
__global__ void __launch_bounds__(kBlockThreads) pt_triquery(const TriArgs a) {
  __shared__ int ldsStack[kWavesPerBlock * kLdsStack * 64];
  const SceneView& sc = a.scene;
  const int gthread = blockIdx.x * kBlockThreads + threadIdx.x, stride = gridDim.x * kBlockThreads;
  TriStack st;
  st.init(ldsStack, a.stackOverflow, gthread, stride);
  for (int i = gthread; i < a.n; i += stride) {           // n <= kTriMaxLaunch = 2^30 and stride <= 2^22: no overflow
    const float* t = a.tris + 9 * (size_t)i;
    const float f[9] = { t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8] };
    const TriQ q = tri_make(f);
    BoxOut o;
    o.slice = nullptr; o.cap = 0; o.count = 0;
    if constexpr (MODE == BOX_LIST) {
      const long long first = a.offsets[i], cap = a.offsets[(size_t)i + 1] - first;
      o.slice = a.prims + first; o.cap = cap > 0 ? cap : 0;
    }
    BoxTrav tv;
    tri_begin<MODE>(sc, q, tri_valid(f), tv, o);
    while (tv.node != kTravDone) tri_step<MODE, N64>(sc, q, tv, st, o);
    if constexpr (MODE == BOX_LIST) box_list_finish(o);
    a.out[i] = MODE == BOX_ANY ? (o.count > 0 ? 1 : 0) : o.count;
  }
}

template <int MODE>
void launch_mode(hipStream_t stream, const TriArgs& a, int blocks) {
  if (a.scene.nodes64 != nullptr) pt_triquery<MODE, true><<<blocks, kBlockThreads, 0, stream>>>(a);
  else                            pt_triquery<MODE, false><<<blocks, kBlockThreads, 0, stream>>>(a);
}

}  // namespace

size_t trikernel_overflow_ints(int nBlocks, int stackBound) { return lane_stack_overflow_entries((size_t)nBlocks * kBlockThreads, stackBound, kLdsStack); }

hipError_t launch_triquery(hipStream_t stream, const TriArgs& a, int nBlocks, int mode) {
  const int blocks = (int)std::min<long long>(nBlocks, ((long long)a.n + kBlockThreads - 1) / kBlockThreads);
  if (mode == BOX_LIST) launch_mode<BOX_LIST>(stream, a, blocks);
  else if (mode == BOX_COUNT) launch_mode<BOX_COUNT>(stream, a, blocks);
  else launch_mode<BOX_ANY>(stream, a, blocks);
  return hipGetLastError();
}

}  // namespace pt
