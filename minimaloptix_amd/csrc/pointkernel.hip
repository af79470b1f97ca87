// pointkernel.hip -- closest-point queries (pt_point.h) for gfx950: the nearest surface point, or "is anything within maxDist", for
// caller-supplied points.
//
// Its own translation unit, as the ray-query kernel's: nothing of this pass is compiled into the trace kernels.
//
// Execution model: the ray queries' (querykernel.hip).  One point per lane, walked to its end with the if-if step (pt_point.h point_step).
// The grid is ceil(n / 256) workgroups up to a cap of CUs x blocksPerCU; past the cap a lane goes on to the point one grid further
// (grid-stride loop), so the stack overflow area is sized by the cap, not by n, and a result goes to its point's own index: nothing depends
// on the scheduling.  A point is read as one 16-byte load, a record written as two 16-byte stores.
// The traversal stack holds a child reference and the squared distance to its box side by side, eight bytes an entry: 16 entries per lane
// in LDS ([entry][lane], 32 KB per workgroup as the ray queries' 32 four-byte ones) with a global overflow column per thread.
// The signed mode is the closest walk followed by point_hit_signed (pt_sign.h): the feature of the winner, one v3 of its sign record, the
// sign.  Its argument record carries the table behind the others' (PointSignedArgs), so the kernel is a template over the record too.
// The K-nearest queries (pt_pointmulti.h) are a kernel of their own beside it, pt_pointquery_multi: the same grid, loop and stack.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_lanestack.h"
#include "pt_sign.h"
#include "pt_pointmulti.h"
#include "pointkernel.h"

namespace pt {

namespace {

constexpr int kBlockThreads = 256;
constexpr int kWavesPerBlock = kBlockThreads / 64;
constexpr int kLdsStack = 16;          // entries per lane kept in LDS (8 bytes each: 32 KB per workgroup)

// LaneStack (pt_lanestack.h) over eight-byte entries: reference + box distance
struct PointStack : LaneStack<kLdsStack, unsigned long long> {
  __device__ __forceinline__ void store(int sp, int ref, float d2) {
    LaneStack::store(sp, ((unsigned long long)(uint32_t)f2i(d2) << 32) | (uint32_t)ref);
  }
  __device__ __forceinline__ void load(int sp, int& ref, float& d2) const {
    const unsigned long long e = LaneStack::load(sp);
    ref = (int32_t)(uint32_t)e; d2 = i2f((int32_t)(e >> 32));
  }
};

__device__ __forceinline__ const PointArgs& point_args(const PointArgs& s) { return s; }
__device__ __forceinline__ const PointArgs& point_args(const PointSignedArgs& s) { return s.p; }

// MODE: POINT_CLOSEST / POINT_ANY over PointArgs, POINT_SIGNED over PointSignedArgs
template <int MODE, bool N64, class Args>
__global__ void __launch_bounds__(kBlockThreads) pt_pointquery(const Args s) {
  constexpr bool ANY = MODE == POINT_ANY;
  __shared__ unsigned long long ldsStack[kWavesPerBlock * kLdsStack * 64];
  const PointArgs& a = point_args(s);
  const SceneView& sc = a.scene;
  const int gthread = blockIdx.x * kBlockThreads + threadIdx.x, stride = gridDim.x * kBlockThreads;
  PointStack st;
  st.init(ldsStack, a.stackOverflow, gthread, stride);
  const uint4* __restrict__ points = reinterpret_cast<const uint4*>(a.points);
  for (int i = gthread; i < a.n; i += stride) {           // n <= kPointMaxLaunch = 2^30 and stride <= 2^22: no overflow
    const uint4 r = points[(size_t)i];
    const float p[4] = { i2f((int32_t)r.x), i2f((int32_t)r.y), i2f((int32_t)r.z), i2f((int32_t)r.w) };
    const v3 q = mk3(p[0], p[1], p[2]);
    PointTrav tv;
    point_begin<ANY>(sc, q, p[3] * p[3], point_valid(p), tv);
    while (tv.node != kTravDone) point_step<ANY, N64>(sc, q, tv, st);
    if constexpr (ANY) {
      static_cast<int*>(a.out)[i] = tv.bestPrim >= 0 ? 1 : 0;
    } else {
      PointHit h;
      if constexpr (MODE == POINT_SIGNED) point_hit_signed(sc, s.table, q, p[3], tv, h);
      else point_hit(sc, q, p[3], tv, h);
      uint4* o = static_cast<uint4*>(a.out) + 2 * (size_t)i;
      o[0] = make_uint4((uint32_t)f2i(h.dist), (uint32_t)h.prim, (uint32_t)h.mat, (uint32_t)f2i(h.u));
      o[1] = make_uint4((uint32_t)f2i(h.v), (uint32_t)f2i(h.p[0]), (uint32_t)f2i(h.p[1]), (uint32_t)f2i(h.p[2]));
    }
  }
}

// K nearest (pt_pointmulti.h): the same grid, loop and stack.  The K candidates of a point live in its own slice of the output while it is
// walked (16-byte keys, turned into records in place at the end), so K costs no registers and no LDS: the lane holds the count, the total
// and the K-th key.
template <bool N64, bool ALL>
__global__ void __launch_bounds__(kBlockThreads) pt_pointquery_multi(const PointMultiArgs a) {
  __shared__ unsigned long long ldsStack[kWavesPerBlock * kLdsStack * 64];
  const SceneView& sc = a.scene;
  const int gthread = blockIdx.x * kBlockThreads + threadIdx.x, stride = gridDim.x * kBlockThreads;
  PointStack st;
  st.init(ldsStack, a.stackOverflow, gthread, stride);
  const uint4* __restrict__ points = reinterpret_cast<const uint4*>(a.points);
  for (int i = gthread; i < a.n; i += stride) {           // n x max(maxNear, 1) <= kPointMaxLaunch: the record index fits 32 bits too
    const uint4 r = points[(size_t)i];
    const float p[4] = { i2f((int32_t)r.x), i2f((int32_t)r.y), i2f((int32_t)r.z), i2f((int32_t)r.w) };
    const v3 q = mk3(p[0], p[1], p[2]);
    const float r2 = p[3] * p[3];
    PointTrav tv;
    NearList nl;
    nl.init(static_cast<Word4*>(a.hits) + 2 * (size_t)i * (size_t)a.maxNear, a.maxNear);      // maxNear 0: never dereferenced
    pointmulti_begin<ALL>(sc, q, r2, point_valid(p), tv, nl);
    while (tv.node != kTravDone) pointmulti_step<ALL, N64>(sc, q, r2, tv, st, nl);
    pointmulti_finish(sc, q, p[3], nl);
    a.counts[i] = ALL ? nl.total : nl.count;
  }
}

}  // namespace

size_t pointkernel_overflow_entries(int nBlocks, int stackBound) { return lane_stack_overflow_entries((size_t)nBlocks * kBlockThreads, stackBound, kLdsStack); }

hipError_t launch_pointquery(hipStream_t stream, const PointArgs& a, const SignRecord* table, int nBlocks, int mode) {
  const int blocks = (int)std::min<long long>(nBlocks, ((long long)a.n + kBlockThreads - 1) / kBlockThreads);
  const bool n64 = a.scene.nodes64 != nullptr;
  if (mode == POINT_SIGNED) {
    const PointSignedArgs s = { a, table };
    if (n64) pt_pointquery<POINT_SIGNED, true><<<blocks, kBlockThreads, 0, stream>>>(s);
    else     pt_pointquery<POINT_SIGNED, false><<<blocks, kBlockThreads, 0, stream>>>(s);
  } else if (mode == POINT_ANY) {
    if (n64) pt_pointquery<POINT_ANY, true><<<blocks, kBlockThreads, 0, stream>>>(a);
    else     pt_pointquery<POINT_ANY, false><<<blocks, kBlockThreads, 0, stream>>>(a);
  } else {
    if (n64) pt_pointquery<POINT_CLOSEST, true><<<blocks, kBlockThreads, 0, stream>>>(a);
    else     pt_pointquery<POINT_CLOSEST, false><<<blocks, kBlockThreads, 0, stream>>>(a);
  }
  return hipGetLastError();
}

hipError_t launch_pointquery_multi(hipStream_t stream, const PointMultiArgs& a, int nBlocks, bool countAll) {
  const int blocks = (int)std::min<long long>(nBlocks, ((long long)a.n + kBlockThreads - 1) / kBlockThreads);
  const bool n64 = a.scene.nodes64 != nullptr;
  if (countAll) {
    if (n64) pt_pointquery_multi<true, true><<<blocks, kBlockThreads, 0, stream>>>(a);
    else     pt_pointquery_multi<false, true><<<blocks, kBlockThreads, 0, stream>>>(a);
  } else {
    if (n64) pt_pointquery_multi<true, false><<<blocks, kBlockThreads, 0, stream>>>(a);
    else     pt_pointquery_multi<false, false><<<blocks, kBlockThreads, 0, stream>>>(a);
  }
  return hipGetLastError();
}

}  // namespace pt
