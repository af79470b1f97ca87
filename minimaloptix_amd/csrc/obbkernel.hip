// obbkernel.hip -- oriented box queries (pt_obb.h) for gfx950: does anything meet the caller's rotated box, how many primitives do, and
// which.
//
// Its own translation unit, as the box kernel's: nothing of this pass is compiled into another kernel.
//
// Execution model: the box queries' (boxkernel.hip).  One box per lane, walked to its end with the if-if step (pt_obb.h obb_step).  The
// grid is ceil(n / 256) workgroups up to a cap of CUs x blocksPerCU; past the cap a lane goes on to the box one grid further (grid-stride
// loop), so the stack overflow area is sized by the cap, not by n, and a result goes to its box's own index: nothing depends on the
// scheduling.  A box is read as four 16-byte loads; its absolute axes and its grown world box are computed once, in front of the walk.
// The traversal stack holds child references alone, four bytes an entry: 16 entries per lane in LDS ([entry][lane], 16 KB per workgroup)
// with a global overflow column per thread.  The list is the box queries': appended to the box's own slice, heap-sorted there.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_lanestack.h"
#include "pt_obb.h"
#include "obbkernel.h"

namespace pt {

namespace {

constexpr int kBlockThreads = 256;
constexpr int kWavesPerBlock = kBlockThreads / 64;
constexpr int kLdsStack = 16;          // entries per lane kept in LDS (4 bytes each: 16 KB per workgroup)

using ObbStack = LaneStack<kLdsStack, int>;

template <int MODE, bool N64>
__global__ void __launch_bounds__(kBlockThreads) pt_obbquery(const ObbArgs a) {
  __shared__ int ldsStack[kWavesPerBlock * kLdsStack * 64];
  const SceneView& sc = a.scene;
  const int gthread = blockIdx.x * kBlockThreads + threadIdx.x, stride = gridDim.x * kBlockThreads;
  ObbStack st;
  st.init(ldsStack, a.stackOverflow, gthread, stride);
  const float4* obbs = reinterpret_cast<const float4*>(a.obbs);
  for (int i = gthread; i < a.n; i += stride) {           // n <= kObbMaxLaunch = 2^30 and stride <= 2^22: no overflow
    const float4 f0 = obbs[4 * (size_t)i], f1 = obbs[4 * (size_t)i + 1], f2 = obbs[4 * (size_t)i + 2], f3 = obbs[4 * (size_t)i + 3];
    const float f[16] = { f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w, f2.x, f2.y, f2.z, f2.w, f3.x, f3.y, f3.z, f3.w };
    const Obb q = obb_make(f);
    BoxOut o;
    o.slice = nullptr; o.cap = 0; o.count = 0;
    if constexpr (MODE == BOX_LIST) {
      const long long first = a.offsets[i], cap = a.offsets[(size_t)i + 1] - first;
      o.slice = a.prims + first; o.cap = cap > 0 ? cap : 0;
    }
    BoxTrav tv;
    obb_begin<MODE>(sc, q, obb_valid(f), tv, o);
    while (tv.node != kTravDone) obb_step<MODE, N64>(sc, q, tv, st, o);
    if constexpr (MODE == BOX_LIST) box_list_finish(o);
    a.out[i] = MODE == BOX_ANY ? (o.count > 0 ? 1 : 0) : o.count;
  }
}

template <int MODE>
void launch_mode(hipStream_t stream, const ObbArgs& a, int blocks) {
  if (a.scene.nodes64 != nullptr) pt_obbquery<MODE, true><<<blocks, kBlockThreads, 0, stream>>>(a);
  else                            pt_obbquery<MODE, false><<<blocks, kBlockThreads, 0, stream>>>(a);
}

}  // namespace

size_t obbkernel_overflow_ints(int nBlocks, int stackBound) { return lane_stack_overflow_entries((size_t)nBlocks * kBlockThreads, stackBound, kLdsStack); }

hipError_t launch_obbquery(hipStream_t stream, const ObbArgs& a, int nBlocks, int mode) {
  const int blocks = (int)std::min<long long>(nBlocks, ((long long)a.n + kBlockThreads - 1) / kBlockThreads);
  if (mode == BOX_LIST) launch_mode<BOX_LIST>(stream, a, blocks);
  else if (mode == BOX_COUNT) launch_mode<BOX_COUNT>(stream, a, blocks);
  else launch_mode<BOX_ANY>(stream, a, blocks);
  return hipGetLastError();
}

}  // namespace pt
