// boxkernel.hip -- box overlap queries (pt_box.h) for gfx950: does anything meet the caller's axis-aligned box, how many primitives do,
// and which.
//
// Its own translation unit, as the point kernel's: nothing of this pass is compiled into another kernel.
//
// Execution model: the point queries' (pointkernel.hip).  One box per lane, walked to its end with the if-if step (pt_box.h box_step).
// The grid is ceil(n / 256) workgroups up to a cap of CUs x blocksPerCU; past the cap a lane goes on to the box one grid further
// (grid-stride loop), so the stack overflow area is sized by the cap, not by n, and a result goes to its box's own index: nothing depends
// on the scheduling.  A box is read as three 8-byte loads.
// The traversal stack holds child references alone, four bytes an entry: 16 entries per lane in LDS ([entry][lane], 16 KB per workgroup;
// the point queries' count) with a global overflow column per thread.
// The list mode appends the ids to the box's own slice of the caller's array while they fit and heap-sorts that slice in place at the
// end: the list costs no registers and no LDS, and a lane only ever re-reads what it stored itself.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_lanestack.h"
#include "pt_box.h"
#include "boxkernel.h"

namespace pt {

namespace {

constexpr int kBlockThreads = 256;
constexpr int kWavesPerBlock = kBlockThreads / 64;
constexpr int kLdsStack = 16;          // entries per lane kept in LDS (4 bytes each: 16 KB per workgroup)

using BoxStack = LaneStack<kLdsStack, int>;

template <int MODE, bool N64>
__global__ void __launch_bounds__(kBlockThreads) pt_boxquery(const BoxArgs a) {
  __shared__ int ldsStack[kWavesPerBlock * kLdsStack * 64];
  const SceneView& sc = a.scene;
  const int gthread = blockIdx.x * kBlockThreads + threadIdx.x, stride = gridDim.x * kBlockThreads;
  BoxStack st;
  st.init(ldsStack, a.stackOverflow, gthread, stride);
  const float2* boxes = reinterpret_cast<const float2*>(a.boxes);
  for (int i = gthread; i < a.n; i += stride) {           // n <= kBoxMaxLaunch = 2^30 and stride <= 2^22: no overflow
    const float2 b0 = boxes[3 * (size_t)i], b1 = boxes[3 * (size_t)i + 1], b2 = boxes[3 * (size_t)i + 2];
    const float b[6] = { b0.x, b0.y, b1.x, b1.y, b2.x, b2.y };
    Box6 q;
    q.lo = mk3(b[0], b[1], b[2]); q.hi = mk3(b[3], b[4], b[5]);
    BoxOut o;
    o.slice = nullptr; o.cap = 0; o.count = 0;
    if constexpr (MODE == BOX_LIST) {
      const long long first = a.offsets[i], cap = a.offsets[(size_t)i + 1] - first;
      o.slice = a.prims + first; o.cap = cap > 0 ? cap : 0;
    }
    BoxTrav tv;
    box_begin<MODE>(sc, q, box_valid(b), tv, o);
    while (tv.node != kTravDone) box_step<MODE, N64>(sc, q, tv, st, o);
    if constexpr (MODE == BOX_LIST) box_list_finish(o);
    a.out[i] = MODE == BOX_ANY ? (o.count > 0 ? 1 : 0) : o.count;
  }
}

template <int MODE>
void launch_mode(hipStream_t stream, const BoxArgs& a, int blocks) {
  if (a.scene.nodes64 != nullptr) pt_boxquery<MODE, true><<<blocks, kBlockThreads, 0, stream>>>(a);
  else                            pt_boxquery<MODE, false><<<blocks, kBlockThreads, 0, stream>>>(a);
}

}  // namespace

size_t boxkernel_overflow_ints(int nBlocks, int stackBound) { return lane_stack_overflow_entries((size_t)nBlocks * kBlockThreads, stackBound, kLdsStack); }

hipError_t launch_boxquery(hipStream_t stream, const BoxArgs& a, int nBlocks, int mode) {
  const int blocks = (int)std::min<long long>(nBlocks, ((long long)a.n + kBlockThreads - 1) / kBlockThreads);
  if (mode == BOX_LIST) launch_mode<BOX_LIST>(stream, a, blocks);
  else if (mode == BOX_COUNT) launch_mode<BOX_COUNT>(stream, a, blocks);
  else launch_mode<BOX_ANY>(stream, a, blocks);
  return hipGetLastError();
}

}  // namespace pt
