// sweepkernel.hip -- sphere sweep queries (pt_sweep.h) for gfx950: the first contact of a moving sphere with the scene, or "does it touch
// anything on the way", for caller-supplied sweeps.
//
// Its own translation unit, as the point and box kernels': nothing of this pass is compiled into another kernel.
//
// Execution model: the point queries' (pointkernel.hip).  One sweep per lane, walked to its end with the if-if step (pt_sweep.h
// sweep_step).  The grid is ceil(n / 256) workgroups up to a cap of CUs x blocksPerCU; past the cap a lane goes on to the sweep one grid
// further (grid-stride loop), so the stack overflow area is sized by the cap, not by n, and a result goes to its sweep's own index:
// nothing depends on the scheduling.  A sweep is read as two 16-byte loads, a record written as two 16-byte stores.
// The traversal stack holds a child reference and the entry time of its grown box side by side, eight bytes an entry: 16 entries per
// lane in LDS ([entry][lane], 32 KB per workgroup) with a global overflow column per thread.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_lanestack.h"
#include "pt_sweep.h"
#include "sweepkernel.h"

namespace pt {

namespace {

constexpr int kBlockThreads = 256;
constexpr int kWavesPerBlock = kBlockThreads / 64;
constexpr int kLdsStack = 16;          // entries per lane kept in LDS (8 bytes each: 32 KB per workgroup)

// LaneStack (pt_lanestack.h) over eight-byte entries: reference + entry time
struct SweepStack : LaneStack<kLdsStack, unsigned long long> {
  __device__ __forceinline__ void store(int sp, int ref, float tn) {
    LaneStack::store(sp, ((unsigned long long)(uint32_t)f2i(tn) << 32) | (uint32_t)ref);
  }
  __device__ __forceinline__ void load(int sp, int& ref, float& tn) const {
    const unsigned long long e = LaneStack::load(sp);
    ref = (int32_t)(uint32_t)e; tn = i2f((int32_t)(e >> 32));
  }
};

template <int MODE, bool N64>
__global__ void __launch_bounds__(kBlockThreads) pt_sweepquery(const SweepArgs a) {
  constexpr bool ANY = MODE == SWEEP_ANY;
  __shared__ unsigned long long ldsStack[kWavesPerBlock * kLdsStack * 64];
  const SceneView& sc = a.scene;
  const int gthread = blockIdx.x * kBlockThreads + threadIdx.x, stride = gridDim.x * kBlockThreads;
  SweepStack st;
  st.init(ldsStack, a.stackOverflow, gthread, stride);
  const uint4* __restrict__ sweeps = reinterpret_cast<const uint4*>(a.sweeps);
  for (int i = gthread; i < a.n; i += stride) {           // n <= kSweepMaxLaunch = 2^30 and stride <= 2^22: no overflow
    const uint4 r0 = sweeps[2 * (size_t)i], r1 = sweeps[2 * (size_t)i + 1];
    const float s[8] = { i2f((int32_t)r0.x), i2f((int32_t)r0.y), i2f((int32_t)r0.z), i2f((int32_t)r0.w),
                         i2f((int32_t)r1.x), i2f((int32_t)r1.y), i2f((int32_t)r1.z), i2f((int32_t)r1.w) };
    SweepQ q;
    sweep_query(s, q);
    SweepTrav tv;
    sweep_begin<ANY>(sc, q, sweep_valid(s), tv);
    while (tv.node != kTravDone) sweep_step<ANY, N64>(sc, q, tv, st);
    if constexpr (ANY) {
      static_cast<int*>(a.out)[i] = tv.bestPrim >= 0 ? 1 : 0;
    } else {
      SweepHit h;
      sweep_hit(sc, q, tv, h);
      uint4* o = static_cast<uint4*>(a.out) + 2 * (size_t)i;
      o[0] = make_uint4((uint32_t)f2i(h.t), (uint32_t)h.prim, (uint32_t)h.mat, (uint32_t)f2i(h.u));
      o[1] = make_uint4((uint32_t)f2i(h.v), (uint32_t)f2i(h.p[0]), (uint32_t)f2i(h.p[1]), (uint32_t)f2i(h.p[2]));
    }
  }
}

template <int MODE>
void launch_mode(hipStream_t stream, const SweepArgs& a, int blocks) {
  if (a.scene.nodes64 != nullptr) pt_sweepquery<MODE, true><<<blocks, kBlockThreads, 0, stream>>>(a);
  else                            pt_sweepquery<MODE, false><<<blocks, kBlockThreads, 0, stream>>>(a);
}

}  // namespace

size_t sweepkernel_overflow_entries(int nBlocks, int stackBound) { return lane_stack_overflow_entries((size_t)nBlocks * kBlockThreads, stackBound, kLdsStack); }

hipError_t launch_sweepquery(hipStream_t stream, const SweepArgs& a, int nBlocks, int mode) {
  const int blocks = (int)std::min<long long>(nBlocks, ((long long)a.n + kBlockThreads - 1) / kBlockThreads);
  if (mode == SWEEP_ANY) launch_mode<SWEEP_ANY>(stream, a, blocks);
  else launch_mode<SWEEP_CLOSEST>(stream, a, blocks);
  return hipGetLastError();
}

}  // namespace pt
