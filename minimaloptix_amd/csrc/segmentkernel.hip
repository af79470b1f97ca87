// segmentkernel.hip -- segment queries (pt_segment.h) for gfx950: the nearest surface point to each of the caller's segments, or "is
// anything within maxDist of it".
//
// Its own translation unit, as the point and sweep kernels': nothing of this pass is compiled into another kernel.
//
// Execution model: the point queries' (pointkernel.hip).  One segment per lane, walked to its end with the if-if step (pt_segment.h
// segment_step).  The grid is ceil(n / 256) workgroups up to a cap of CUs x blocksPerCU; past the cap a lane goes on to the segment one
// grid further (grid-stride loop), so the stack overflow area is sized by the cap, not by n, and a result goes to its segment's own
// index: nothing depends on the scheduling.  A segment is read as two 16-byte loads, a record written as two 16-byte stores.
// The traversal stack holds a child reference and the distance bound of its box side by side, eight bytes an entry: 16 entries per
// lane in LDS ([entry][lane], 32 KB per workgroup) with a global overflow column per thread.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_lanestack.h"
#include "pt_segment.h"
#include "segmentkernel.h"

namespace pt {

namespace {

constexpr int kBlockThreads = 256;
constexpr int kWavesPerBlock = kBlockThreads / 64;
constexpr int kLdsStack = 16;          // entries per lane kept in LDS (8 bytes each: 32 KB per workgroup)

// LaneStack (pt_lanestack.h) over eight-byte entries: reference + box distance
struct SegmentStack : LaneStack<kLdsStack, unsigned long long> {
  __device__ __forceinline__ void store(int sp, int ref, float d2) {
    LaneStack::store(sp, ((unsigned long long)(uint32_t)f2i(d2) << 32) | (uint32_t)ref);
  }
  __device__ __forceinline__ void load(int sp, int& ref, float& d2) const {
    const unsigned long long e = LaneStack::load(sp);
    ref = (int32_t)(uint32_t)e; d2 = i2f((int32_t)(e >> 32));
  }
};

template <int MODE, bool N64>
__global__ void __launch_bounds__(kBlockThreads) pt_segmentquery(const SegmentArgs a) {
  constexpr bool ANY = MODE == SEGMENT_ANY;
  __shared__ unsigned long long ldsStack[kWavesPerBlock * kLdsStack * 64];
  const SceneView& sc = a.scene;
  const int gthread = blockIdx.x * kBlockThreads + threadIdx.x, stride = gridDim.x * kBlockThreads;
  SegmentStack st;
  st.init(ldsStack, a.stackOverflow, gthread, stride);
  const uint4* __restrict__ segments = reinterpret_cast<const uint4*>(a.segments);
  for (int i = gthread; i < a.n; i += stride) {           // n <= kSegmentMaxLaunch = 2^30 and stride <= 2^22: no overflow
    const uint4 r0 = segments[2 * (size_t)i], r1 = segments[2 * (size_t)i + 1];
    const float s[8] = { i2f((int32_t)r0.x), i2f((int32_t)r0.y), i2f((int32_t)r0.z), i2f((int32_t)r0.w),
                         i2f((int32_t)r1.x), i2f((int32_t)r1.y), i2f((int32_t)r1.z), i2f((int32_t)r1.w) };
    SegQ q;
    segment_query(s, q);
    PointTrav tv;
    segment_begin<ANY>(sc, q, segment_valid(s), tv);
    while (tv.node != kTravDone) segment_step<ANY, N64>(sc, q, tv, st);
    if constexpr (ANY) {
      static_cast<int*>(a.out)[i] = tv.bestPrim >= 0 ? 1 : 0;
    } else {
      SegmentHit h;
      segment_hit(sc, q, tv, h);
      uint4* o = static_cast<uint4*>(a.out) + 2 * (size_t)i;
      o[0] = make_uint4((uint32_t)f2i(h.dist), (uint32_t)h.prim, (uint32_t)h.mat, (uint32_t)f2i(h.s));
      o[1] = make_uint4((uint32_t)f2i(h.p[0]), (uint32_t)f2i(h.p[1]), (uint32_t)f2i(h.p[2]), (uint32_t)h.feature);
    }
  }
}

template <int MODE>
void launch_mode(hipStream_t stream, const SegmentArgs& a, int blocks) {
  if (a.scene.nodes64 != nullptr) pt_segmentquery<MODE, true><<<blocks, kBlockThreads, 0, stream>>>(a);
  else                            pt_segmentquery<MODE, false><<<blocks, kBlockThreads, 0, stream>>>(a);
}

}  // namespace

size_t segmentkernel_overflow_entries(int nBlocks, int stackBound) { return lane_stack_overflow_entries((size_t)nBlocks * kBlockThreads, stackBound, kLdsStack); }

hipError_t launch_segmentquery(hipStream_t stream, const SegmentArgs& a, int nBlocks, int mode) {
  const int blocks = (int)std::min<long long>(nBlocks, ((long long)a.n + kBlockThreads - 1) / kBlockThreads);
  if (mode == SEGMENT_ANY) launch_mode<SEGMENT_ANY>(stream, a, blocks);
  else launch_mode<SEGMENT_CLOSEST>(stream, a, blocks);
  return hipGetLastError();
}

}  // namespace pt
