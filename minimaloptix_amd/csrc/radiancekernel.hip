// radiancekernel.hip -- radiance queries (pt_radiance.h) for gfx950: path-traced radiance along caller-supplied rays.
//
// Its own translation unit, as the AOV kernel's and the ray queries': nothing of this pass is compiled into the trace kernels.
//
// Execution model: pt_megakernel's (megakernel.hip), not pt_rayquery's -- the paths of one batch differ in length by two orders of
// magnitude (a miss is one ray, a path between glass walls a thousand), so a lane that finishes a sample takes the next work item from a
// global counter instead of waiting for its wave.  One path per lane; per wave the loop alternates [A] the path state machine (shade /
// next work item / next ray) and [B] the while-while BVH traversal, which the wave leaves once fewer than exitThreshold lanes still
// traverse while others wait to be shaded.  Work item k = i * nSamples + s is ray-major, so the lanes of a wave start on the same ray
// or its neighbours.  The traversal stack is 32 entries per lane in LDS ([entry][lane]) with a global overflow column per thread.
//
// Which lane traces which sample, and when, is left to the hardware; so no sample is ever added to anything here.  A finished sample
// goes to its own record k of a scratch buffer (one 16-byte store: r g b t), and a second kernel, one thread per ray, adds the ray's
// records in sample order onto the output: the sum's bits do not depend on the scheduling, the grid size or the number of passes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_lanestack.h"
#include "pt_radiance.h"
#include "radiancekernel.h"

namespace pt {

namespace {

constexpr int kBlockThreads = 256;
constexpr int kWavesPerBlock = kBlockThreads / 64;
constexpr int kLdsStack = 32;          // entries per lane kept in LDS (32 KB per workgroup)

template <bool N64>
__global__ void __launch_bounds__(kBlockThreads) pt_radiancekernel(const RadianceArgs a) {
  __shared__ int ldsStack[kWavesPerBlock * kLdsStack * 64];
  const SceneView& sc = a.scene;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  LaneStack<kLdsStack> st;      // not st.init: it takes the thread's index ready, and this kernel's code has it computed behind the LDS column
  st.lds = ldsStack + wave * (kLdsStack * 64) + lane;
  st.ovfStride = gridDim.x * kBlockThreads;
  st.ovf = a.stackOverflow ? a.stackOverflow + (blockIdx.x * kBlockThreads + threadIdx.x) : nullptr;
  const uint4* __restrict__ rays = reinterpret_cast<const uint4*>(a.rays);
  const int nWork = a.n * a.nSamples;                 // <= kRadianceMaxWork

  PathState ps;
  Trav tv;
  idle_path(ps, tv);
  ps.cdlin = mk3(0, 0, 0); tv.bestCls = 0;
  Counters ct;                      // not counted: never written
  float tFirst = 0.f;

  for (;;) {
    // ---- [A] path state machine: run until this lane owns a ray again or is out of work ----
    while (ps.mode != M_TRACE && ps.mode != M_DONE) {
      if (ps.mode == M_RESULT) {
        radiance_on_result<false>(sc, ps, tv, tFirst, ct);
      } else if (ps.mode == M_LIGHTS) {
        on_lights<false>(sc, ps, ct);
      } else if (ps.mode == M_NEW_SAMPLE) {               // the finished sample -> its own record
        const v3 v = radiance_value(ps, a.flags);
        reinterpret_cast<float4*>(a.scratch)[ps.item] = make_float4(v.x, v.y, v.z, tFirst);
        ps.mode = M_NEW_PIXEL;
      } else {  // M_NEW_PIXEL: next (ray, sample) work item
        const int k = atomicAdd(a.workCounter, 1);     // hipcc aggregates this per wave
        if (k >= nWork) { ps.mode = M_DONE; }
        else {
          const int i = k / a.nSamples, s = k - i * a.nSamples;
          const uint4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
          const float r[8] = { i2f((int32_t)r0.x), i2f((int32_t)r0.y), i2f((int32_t)r0.z), i2f((int32_t)r0.w),
                               i2f((int32_t)r1.x), i2f((int32_t)r1.y), i2f((int32_t)r1.z), i2f((int32_t)r1.w) };
          const uint32_t state = a.states ? a.states[(size_t)i * a.statesStride + (size_t)s]
                                          : radiance_state(a.indexBase + (uint32_t)i, a.seeds[s]);
          ps.item = k;
          radiance_begin(sc, ps, r, state, tFirst);
        }
      }
    }
    if (__ballot(ps.mode != M_DONE) == 0ull) break;

    // ---- [B] traversal ----
    if (ps.mode == M_TRACE && !tv.started) trav_begin<false>(sc, ps, tv, ct);
    for (;;) {
      const bool active = (ps.mode == M_TRACE) & (tv.node != kTravDone);
      const unsigned long long am = __ballot(active);
      if (am == 0ull) break;
      const int nActive = popc64(am);
      if (nActive < a.exitThreshold) {
        // leave only if somebody is actually waiting to be shaded / given new work
        const unsigned long long wm = __ballot((ps.mode == M_TRACE) & (tv.node == kTravDone));
        if (wm != 0ull) break;
      }
      // while-while: node steps until enough lanes are parked at a leaf, then one leaf pass
      const bool atNode = active & (tv.node >= 0);
      const unsigned long long nm = __ballot(atNode);
      const int nLeaf = nActive - popc64(nm);
      if (nm != 0ull && nLeaf < a.leafThreshold) {
        if (atNode) trav_node_step<false, N64>(sc, ps, tv, st, ct);
      } else {
        if (active & (tv.node < 0)) trav_leaf_step<false>(sc, ps, tv, st, ct);
      }
    }
    if (ps.mode == M_TRACE && tv.node == kTravDone) { ps.mode = M_RESULT; tv.started = 0; }
  }
}

// out[i] (+)= the ray's records in sample order; t from the ray's first record (every sample of a ray carries the same one).
__global__ void __launch_bounds__(kBlockThreads) k_radiance_sum(const RadianceArgs a) {
  const int i = blockIdx.x * kBlockThreads + threadIdx.x;
  if (i >= a.n) return;
  float4* o = reinterpret_cast<float4*>(a.out) + i;
  const float* rec = a.scratch + 4 * ((size_t)i * (size_t)a.nSamples);
  v3 acc = mk3(0.f, 0.f, 0.f);
  if (!a.firstPass) { const float4 p = *o; acc = mk3(p.x, p.y, p.z); }
  acc = radiance_sum(acc, rec, a.nSamples, 4);
  *o = make_float4(acc.x, acc.y, acc.z, rec[3]);
}

}  // namespace

size_t radiancekernel_overflow_ints(int nBlocks, int stackBound) { return lane_stack_overflow_entries((size_t)nBlocks * kBlockThreads, stackBound, kLdsStack); }

hipError_t launch_radiance(hipStream_t stream, const RadianceArgs& a, int nBlocks) {
  const long long nWork = (long long)a.n * a.nSamples;
  if (a.n <= 0 || a.nSamples <= 0 || nWork > kRadianceMaxWork) return hipErrorInvalidValue;
  const int blocks = (int)std::min<long long>(nBlocks, (nWork + kBlockThreads - 1) / kBlockThreads);
  if (a.scene.nodes64 != nullptr) pt_radiancekernel<true><<<blocks, kBlockThreads, 0, stream>>>(a);
  else                            pt_radiancekernel<false><<<blocks, kBlockThreads, 0, stream>>>(a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  k_radiance_sum<<<(a.n + kBlockThreads - 1) / kBlockThreads, kBlockThreads, 0, stream>>>(a);
  return hipGetLastError();
}

}  // namespace pt
