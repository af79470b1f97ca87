// pt_lanestack.h -- what the kernels that give a lane its own ray share: the traversal stack of a lane, the wave-wide helpers and the
// reciprocal of the node step.  Device code, for the .hip files only; lane_stack_overflow_entries is the host's side of the stack.
//
// Everything here is forced inline and changes no code object: tools/isa_diff.py is the check, and a kernel for which a helper does not
// come out instruction for instruction keeps its own text and says so (NOTEBOOK.md, "one lane stack").
#pragma once
#include <hip/hip_runtime.h>

#include "pt_counters.h"
#include "pt_path.h"

namespace pt {

// Traversal stack of one lane: N entries in LDS, laid out [entry][lane] so that a push or pop of a wave is one conflict-free ds_write /
// ds_read, and a column of a global overflow area for deeper trees (stride = the launch's threads).  T is the entry.
template <int N, class T = int>
struct LaneStack {
  T* lds;         // this lane's column of its wave's [N][64] block
  T* ovf;         // this thread's overflow column, or nullptr
  int ovfStride;
  // ldsBase: the workgroup's [wave][N][64] array; overflow: the launch's area or nullptr; gthread: this thread's index in the launch, as
  // and where the kernel computes it (the address arithmetic follows its type, the schedule its place); threads: those of the launch
  template <class I> __device__ __forceinline__ void init(T* ldsBase, T* overflow, I gthread, int threads) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    lds = ldsBase + wave * (N * 64) + lane;
    ovfStride = threads;
    ovf = overflow ? overflow + gthread : nullptr;
  }
  __device__ __forceinline__ void store(int sp, T v) {
    if (sp < N) lds[sp * 64] = v;
    else ovf[(size_t)(sp - N) * ovfStride] = v;
  }
  __device__ __forceinline__ T load(int sp) const {
    return sp < N ? lds[sp * 64] : ovf[(size_t)(sp - N) * ovfStride];
  }
  __device__ __forceinline__ bool roomy(int sp) const { return sp + 3 <= N; }
  __device__ __forceinline__ void store_fast(int sp, T v) { lds[sp * 64] = v; }
  static constexpr bool kFlat = false;      // pt_path.h node_step_nearfar: this stack takes the branched tail
  __device__ __forceinline__ bool fits_fast(int, int) const { return false; }
  __device__ __forceinline__ T peek_fast(int) const { return 0; }
};
// the stack of a scene without a tree
struct NoStack {
  __device__ __forceinline__ void store(int, int) {}
  __device__ __forceinline__ int load(int) const { return kTravDone; }
  __device__ __forceinline__ bool roomy(int) const { return false; }
  __device__ __forceinline__ void store_fast(int, int) {}
  static constexpr bool kFlat = false;
  __device__ __forceinline__ bool fits_fast(int, int) const { return false; }
  __device__ __forceinline__ int peek_fast(int) const { return 0; }
};

// Entries of the overflow area behind LDS stacks of N entries: a column of stackBound - N + 1 per thread; 0 = the tree fits the LDS stack.
inline size_t lane_stack_overflow_entries(size_t threads, int stackBound, int N) {
  return stackBound > N ? threads * (size_t)(stackBound - N + 1) : 0;
}

__device__ __forceinline__ int popc64(unsigned long long m) { return __popcll(m); }
// number of set bits of mask below this lane
__device__ __forceinline__ int lane_rank(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}
// the sum over the wave, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// the per-lane counters of the counting build, summed over the wave, in the order of pt_counters.h
__device__ __forceinline__ void wave_sum_counters(const Counters& ct, uint32_t (&v)[kCntPerLane]) {
  v[kCntSamples] = wave_sum(ct.samples); v[kCntPrimaryRays] = wave_sum(ct.primaryRays); v[kCntBounceRays] = wave_sum(ct.bounceRays);
  v[kCntShadowRays] = wave_sum(ct.shadowRays); v[kCntNodeFetches] = wave_sum(ct.nodeFetches); v[kCntTriTests] = wave_sum(ct.triTests);
  v[kCntClosestHits] = wave_sum(ct.closestHits); v[kCntLightLoads] = wave_sum(ct.lightLoads); v[kCntAnalyticTests] = wave_sum(ct.analyticTests);
}
// slab_inv (pt_path.h) with the hardware reciprocal
__device__ __forceinline__ float node_inv(float d) {
  return __builtin_amdgcn_rcpf(__builtin_fabsf(d) < kSlabMinDir ? __builtin_copysignf(kSlabMinDir, d) : d);
}

// A lane that owns no path yet: the state in which the [A] / [B] loop of pt_megakernel and pt_radiancekernel starts.
__device__ __forceinline__ void idle_path(PathState& ps, Trav& tv) {
  ps.mode = M_NEW_PIXEL; ps.pixel = 0; ps.item = 0; ps.accum = mk3(0, 0, 0);
  ps.thr = mk3(0, 0, 0); ps.rad = mk3(0, 0, 0); ps.depth = 0; ps.seed = 0;
  ps.o = mk3(0, 0, 0); ps.d = mk3(0, 0, 1); ps.tmin = 0; ps.tmax = 0; ps.kind = RK_RADIANCE;
  ps.N = mk3(0, 0, 1); ps.V = mk3(0, 0, 1); ps.mat = 0; ps.light = 0; ps.pendW = mk3(0, 0, 0); ps.pendInv = 0;
  tv.node = kTravDone; tv.sp = 0; tv.started = 0; tv.tbest = 0; tv.bestPrim = -1; tv.bestTri = -1;
  tv.beta = 0; tv.gamma = 0; tv.att = mk3(1, 1, 1); tv.inv = mk3(0, 0, 0); tv.noi = mk3(0, 0, 0);
}

}  // namespace pt
