// querykernel.hip -- batched ray queries (pt_query.h) for gfx950: closest hit and occlusion for caller-supplied rays.
//
// Its own translation unit, as the AOV kernel's: nothing of this pass is compiled into the trace kernels.
//
// Execution model: one ray per lane, walked to its end with the if-if step (pt_query.h query_step), as k_debug_trace does.  The grid is
// ceil(n / 256) workgroups up to a cap of CUs x blocksPerCU; past the cap a lane goes on to the ray one grid further (grid-stride loop), so
// the stack overflow area is sized by the cap, not by n, and a result goes to its ray's own index: nothing depends on the scheduling.
// A ray is read as two 16-byte loads, a hit record written as two 16-byte stores; the traversal stack is 32 entries per lane in LDS
// ([entry][lane]) with a global overflow column per thread.
// A persistent grid over a ray counter, with pt_megakernel's while-while loop and finished lanes refilled below a threshold of live lanes,
// was built first and measured at a quarter of k_debug_trace's rate on either ray set (NOTEBOOK.md round 12, profiles/r12_query.txt): not kept.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_lanestack.h"
#include "pt_multihit.h"
#include "pt_query.h"
#include "querykernel.h"

namespace pt {

namespace {

constexpr int kBlockThreads = 256;
constexpr int kWavesPerBlock = kBlockThreads / 64;
constexpr int kLdsStack = 32;          // entries per lane kept in LDS (32 KB per workgroup)

template <bool ANY, bool N64>
__global__ void __launch_bounds__(kBlockThreads) pt_rayquery(const QueryArgs a) {
  __shared__ int ldsStack[kWavesPerBlock * kLdsStack * 64];
  const SceneView& sc = a.scene;
  const int gthread = blockIdx.x * kBlockThreads + threadIdx.x, stride = gridDim.x * kBlockThreads;
  LaneStack<kLdsStack> st;
  st.init(ldsStack, a.stackOverflow, gthread, stride);
  const uint4* __restrict__ rays = reinterpret_cast<const uint4*>(a.rays);
  Counters ct;                      // not counted: never written
  for (int i = gthread; i < a.n; i += stride) {           // n <= kQueryMaxLaunch = 2^30 and stride <= 2^22: no overflow
    const uint4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
    const float r[8] = { i2f((int32_t)r0.x), i2f((int32_t)r0.y), i2f((int32_t)r0.z), i2f((int32_t)r0.w),
                         i2f((int32_t)r1.x), i2f((int32_t)r1.y), i2f((int32_t)r1.z), i2f((int32_t)r1.w) };
    PathState ps;
    Trav tv;
    const bool valid = query_ray(r, ps);
    query_begin<ANY>(sc, ps, valid, tv, ct);
    while (tv.node != kTravDone) query_step<ANY, N64>(sc, ps, tv, st, ct);
    if constexpr (ANY) {
      static_cast<int*>(a.out)[i] = tv.bestPrim >= 0 ? 1 : 0;
    } else {
      QueryHit h;
      query_hit(sc, ps, tv, h);
      uint4* o = static_cast<uint4*>(a.out) + 2 * (size_t)i;
      o[0] = make_uint4((uint32_t)f2i(h.t), (uint32_t)h.prim, (uint32_t)h.mat, (uint32_t)f2i(h.u));
      o[1] = make_uint4((uint32_t)f2i(h.v), (uint32_t)f2i(h.ng[0]), (uint32_t)f2i(h.ng[1]), (uint32_t)f2i(h.ng[2]));
    }
  }
}

// Multi-hit (pt_multihit.h): the same grid, loop and stack.  The K candidates of a ray live in its own slice of the output while it walks
// (16-byte keys, turned into records in place at the end), so K costs no registers and no LDS: the lane holds the count and the K-th key.
template <bool N64, bool ALL>
__global__ void __launch_bounds__(kBlockThreads) pt_rayquery_multi(const MultiArgs a) {
  __shared__ int ldsStack[kWavesPerBlock * kLdsStack * 64];
  const SceneView& sc = a.scene;
  const int gthread = blockIdx.x * kBlockThreads + threadIdx.x, stride = gridDim.x * kBlockThreads;
  LaneStack<kLdsStack> st;
  st.init(ldsStack, a.stackOverflow, gthread, stride);
  const uint4* __restrict__ rays = reinterpret_cast<const uint4*>(a.rays);
  Counters ct;                      // not counted: never written
  for (int i = gthread; i < a.n; i += stride) {           // n x max(maxHits, 1) <= kQueryMaxLaunch: the record index fits 32 bits too
    const uint4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
    const float r[8] = { i2f((int32_t)r0.x), i2f((int32_t)r0.y), i2f((int32_t)r0.z), i2f((int32_t)r0.w),
                         i2f((int32_t)r1.x), i2f((int32_t)r1.y), i2f((int32_t)r1.z), i2f((int32_t)r1.w) };
    PathState ps;
    Trav tv;
    HitList hl;
    const bool valid = query_ray(r, ps);
    hl.init(static_cast<Word4*>(a.hits) + 2 * (size_t)i * (size_t)a.maxHits, a.maxHits);      // maxHits 0: never dereferenced
    multi_begin<ALL>(sc, ps, valid, tv, hl);
    while (tv.node != kTravDone) multi_step<ALL, N64>(sc, ps, tv, st, hl, ct);
    multi_finish(sc, ps, hl);
    a.counts[i] = ALL ? hl.total : hl.count;
  }
}

}  // namespace

int querykernel_blocks(int nCUs, int blocksPerCU) { return (nCUs > 0 ? nCUs : 256) * blocksPerCU; }
size_t querykernel_overflow_ints(int nBlocks, int stackBound) { return lane_stack_overflow_entries((size_t)nBlocks * kBlockThreads, stackBound, kLdsStack); }

hipError_t launch_rayquery(hipStream_t stream, const QueryArgs& a, int nBlocks, int mode) {
  const int blocks = (int)std::min<long long>(nBlocks, ((long long)a.n + kBlockThreads - 1) / kBlockThreads);
  const bool n64 = a.scene.nodes64 != nullptr;
  if (mode == QUERY_ANY) {
    if (n64) pt_rayquery<true, true><<<blocks, kBlockThreads, 0, stream>>>(a);
    else     pt_rayquery<true, false><<<blocks, kBlockThreads, 0, stream>>>(a);
  } else {
    if (n64) pt_rayquery<false, true><<<blocks, kBlockThreads, 0, stream>>>(a);
    else     pt_rayquery<false, false><<<blocks, kBlockThreads, 0, stream>>>(a);
  }
  return hipGetLastError();
}

hipError_t launch_rayquery_multi(hipStream_t stream, const MultiArgs& a, int nBlocks, bool countAll) {
  const int blocks = (int)std::min<long long>(nBlocks, ((long long)a.n + kBlockThreads - 1) / kBlockThreads);
  const bool n64 = a.scene.nodes64 != nullptr;
  if (countAll) {
    if (n64) pt_rayquery_multi<true, true><<<blocks, kBlockThreads, 0, stream>>>(a);
    else     pt_rayquery_multi<false, true><<<blocks, kBlockThreads, 0, stream>>>(a);
  } else {
    if (n64) pt_rayquery_multi<true, false><<<blocks, kBlockThreads, 0, stream>>>(a);
    else     pt_rayquery_multi<false, false><<<blocks, kBlockThreads, 0, stream>>>(a);
  }
  return hipGetLastError();
}

}  // namespace pt
