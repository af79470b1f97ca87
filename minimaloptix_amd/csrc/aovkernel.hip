// aovkernel.hip -- first-hit AOVs of the primary rays (pt_aov.h) for gfx950: albedo, normal, depth, hit count, primitive and
// material id per pixel, summed over a list of launch seeds.
//
// Its own translation unit: the trace kernels' register allocation moves with code they never run (NOTEBOOK.md), so nothing of
// this pass is compiled into them, and nothing of theirs changes for it.
//
// Work split: a wave owns an 8x8 pixel tile (a lane = a pixel), so the primary rays of a wave are coherent and share the L1's
// node lines; waves take tiles from a counter (persistent grid, kBlocksPerCU workgroups per CU).  A lane loops over the seeds of
// its pixel and keeps the sums in registers -- seed order, no atomics, no per-sample buffer.  Lanes advance independently: a lane
// whose ray has finished adds its sample and starts the ray of its next seed in the same loop iteration, so the wave stays full
// until the last lane's last seed instead of waiting for its slowest lane at every seed.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "aovkernel.h"
#include "pt_aov.h"
#include "pt_lanestack.h"

namespace pt {

namespace {

constexpr int kBlockThreads = 256;
constexpr int kWavesPerBlock = kBlockThreads / 64;
constexpr int kLdsStack = 32;          // entries per lane kept in LDS (32 KB per workgroup)
constexpr int kBlocksPerCU = 4;

// N64: walk the 64-byte nodes (sc.nodes64), else the 128-byte ones.  tileCounter: zeroed before the launch.
template <bool N64>
__global__ void __launch_bounds__(kBlockThreads) pt_aovkernel(const AovArgs a, int* tileCounter) {
  __shared__ int ldsStack[kWavesPerBlock * kLdsStack * 64];
  const SceneView& sc = a.scene;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  LaneStack<kLdsStack> st;      // not st.init: this kernel adds the block's and the thread's offset to the pointer one after the other
  st.lds = ldsStack + wave * (kLdsStack * 64) + lane;
  st.ovfStride = gridDim.x * kBlockThreads;
  st.ovf = a.stackOverflow ? a.stackOverflow + blockIdx.x * kBlockThreads + threadIdx.x : nullptr;
  const int tilesX = (sc.width + 7) >> 3, nTiles = tilesX * ((sc.height + 7) >> 3);
  Counters ct;                      // not counted (CNT = false): never written
  for (;;) {
    int tile = 0;
    if (lane == 0) tile = atomicAdd(tileCounter, 1);
    tile = __shfl(tile, 0);
    if (tile >= nTiles) break;
    const int x = (tile % tilesX) * 8 + (lane & 7), y = (tile / tilesX) * 8 + (lane >> 3);
    const bool inFrame = x < sc.width && y < sc.height;
    const int pixel = y * sc.width + x;
    AovPixel acc;
    acc.albedo = mk3(0.f, 0.f, 0.f); acc.normal = mk3(0.f, 0.f, 0.f); acc.depth = 0.f; acc.hits = 0.f; acc.prim = -1; acc.mat = -1;
    if (inFrame) {
      const size_t p3 = 3 * (size_t)pixel;
      acc.albedo = mk3(a.albedo[p3], a.albedo[p3 + 1], a.albedo[p3 + 2]);
      acc.normal = mk3(a.normal[p3], a.normal[p3 + 1], a.normal[p3 + 2]);
      acc.depth = a.depth[pixel]; acc.hits = a.hits[pixel];
    }
    PathState ps;
    Trav tv;
    tv.node = kTravDone;
    int s = 0;
    bool live = inFrame && a.nSeeds > 0;
    if (live) {
      ps.pixel = pixel;
      begin_sample<false>(sc, ps, a.seeds[0], ct);
      trav_begin<false>(sc, ps, tv, ct);
    }
    while (live) {
      if (tv.node != kTravDone) {
        trav_step<false, N64>(sc, ps, tv, st, ct);
      } else {                      // the ray has finished: add its sample, start the next seed's ray in the same iteration
        AovSample smp;
        aov_sample(sc, ps, tv, smp);
        aov_add(acc, smp, a.writeIds != 0 && s == 0);
        if (++s < a.nSeeds) {
          begin_sample<false>(sc, ps, a.seeds[s], ct);
          trav_begin<false>(sc, ps, tv, ct);
        } else {
          live = false;
        }
      }
    }
    if (inFrame && a.nSeeds > 0) {
      const size_t p3 = 3 * (size_t)pixel;
      a.albedo[p3] = acc.albedo.x; a.albedo[p3 + 1] = acc.albedo.y; a.albedo[p3 + 2] = acc.albedo.z;
      a.normal[p3] = acc.normal.x; a.normal[p3 + 1] = acc.normal.y; a.normal[p3 + 2] = acc.normal.z;
      a.depth[pixel] = acc.depth; a.hits[pixel] = acc.hits;
      if (a.writeIds) { a.primId[pixel] = acc.prim; a.matId[pixel] = acc.mat; }
    }
  }
}

int aov_blocks(int nCUs) { return (nCUs > 0 ? nCUs : 256) * kBlocksPerCU; }

}  // namespace

int aovkernel_threads(int nCUs) { return aov_blocks(nCUs) * kBlockThreads; }
size_t aovkernel_overflow_ints(int nCUs, int stackBound) { return lane_stack_overflow_entries(aovkernel_threads(nCUs), stackBound, kLdsStack); }

hipError_t launch_aovkernel(hipStream_t stream, const AovArgs& a, int nCUs, int* tileCounter, bool node64) {
  const long long nTiles = (long long)((a.scene.width + 7) / 8) * ((a.scene.height + 7) / 8);
  const int blocks = (int)std::min<long long>(aov_blocks(nCUs), (nTiles + kWavesPerBlock - 1) / kWavesPerBlock);
  hipError_t e = hipMemsetAsync(tileCounter, 0, sizeof(int), stream);
  if (e != hipSuccess) return e;
  if (node64) pt_aovkernel<true><<<blocks, kBlockThreads, 0, stream>>>(a, tileCounter);
  else        pt_aovkernel<false><<<blocks, kBlockThreads, 0, stream>>>(a, tileCounter);
  return hipGetLastError();
}

}  // namespace pt
