// temporalkernel.hip -- temporal accumulation with reprojection (pt_temporal.h) in front of the a-trous denoiser (pt_denoise.h), for
// gfx950: SVGF's temporal half.  Last call's pre-filter accumulation is fetched through the first-hit geometry and blended with
// this frame's beauty; the temporal luminance moments drive the filter's edge stop where a pixel has history.
//
// Its own translation unit, as aovkernel.hip and denoisekernel.hip: the trace kernels' register allocation moves with code they
// never run (NOTEBOOK.md), so nothing of this pass is compiled into them.  This file holds the reprojection and its counters; the
// a-trous passes behind them, the variance-keeping prepass k_tp_prepass included, are denoisekernel.hip's (launch_atrous).
//
// The denoiser's mapping (image_tile.h): a lane per pixel, a 256-thread workgroup covers 16x16 pixels as four 8x8 tiles, one per wave.  Under
// camera motion a wave's 2x2 bilinear taps fall on a 9x9-pixel neighbourhood of the history: three 16-byte records per tap
// ({I_acc, h}, {N, Z}, {m1, m2, matId, -}), each one vector load, the material id in the moments record's spare component.
// The counters of moptix_temporal_info are reduced per wave (ballot / shuffle), then per workgroup through LDS into one 16-byte
// partial record per workgroup (a plain vector store); k_tp_reduce, one workgroup, sums the records.  Integer sums: their value does
// not depend on the order.  (One atomic per wave and counter on a single record serialised in the L2 and cost 1.5 ms at 1920x1080.)
#include <hip/hip_runtime.h>

#include "denoisekernel.h"
#include "image_tile.h"
#include "temporalkernel.h"

namespace pt {

namespace {

constexpr int kBlockThreads = kImageBlockThreads;

// not pt_lanestack.h's wave_sum: that one leaves the sum in every lane (__shfl_xor), other instructions than these
__device__ __forceinline__ unsigned int wave_sum(unsigned int v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;                                                     // lane 0 holds the sum
}

// kFaces: the triangle case of the contract's step 2 (option "temporal_face_motion"); false is the kernel without it, and what runs
// whenever no face can have moved.
template <bool kFaces> __global__ void __launch_bounds__(kBlockThreads) k_tp_reproject(const TemporalArgs a) {
  int x, y;
  const bool inside = image_pixel(a.k.width, a.k.height, x, y);   // no early return: the whole wave takes part in the reduction
  bool geometry = false, history = false, movedFace = false;
  unsigned int hlen = 0;
  if (inside) {
    const int p = y * a.k.width + x;
    v4 col, guide, side;
    dn_decode(a.accum, a.albedo, a.normal, a.depth, a.hits, a.nAccumulation, a.nSamples, a.demodulate, p, col, guide, side);
    const TpResult r = kFaces ? tp_reproject_faces(a.t, a.prevCol, a.prevGuide, a.prevMom, a.motion, a.faces, x, y, col, guide, a.primId[p], a.matId[p])
                              : tp_reproject(a.t, a.prevCol, a.prevGuide, a.prevMom, a.motion, x, y, col, guide, a.primId[p], a.matId[p]);
    a.colA[p] = r.col; a.side[p] = side;
    a.histCol[p] = r.hist; a.histGuide[p] = guide; a.histMom[p] = r.mom;
    a.motionOut[2 * (size_t)p] = r.mvx; a.motionOut[2 * (size_t)p + 1] = r.mvy;
    a.historyOut[p] = r.hist.w;
    geometry = r.geometry; history = r.history; movedFace = r.movedFace;
    hlen = geometry ? (unsigned int)r.hist.w : 0u;
  }
  const unsigned int nGeo = __popcll(__ballot(geometry)), nHist = __popcll(__ballot(history));
  const unsigned int sumH = wave_sum(hlen);
  unsigned int nMoved = 0;
  if constexpr (kFaces) nMoved = __popcll(__ballot(movedFace));
  __shared__ unsigned int part[kBlockThreads / 64][kFaces ? 4 : 3];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[wave][0] = nGeo; part[wave][1] = nHist; part[wave][2] = sumH;
    if constexpr (kFaces) part[wave][3] = nMoved;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    for (int w = 0; w < kBlockThreads / 64; w++) {
      r.x += part[w][0]; r.y += part[w][1]; r.z += part[w][2];
      if constexpr (kFaces) r.w += part[w][3];
    }
    a.partials[blockIdx.y * gridDim.x + blockIdx.x] = r;       // at most 256 pixels x maxHistory 65536 = 2^24 per workgroup
  }
}

// One workgroup: the sum of the per-workgroup records {geometry, history, sum of h, -} -> TemporalCounters.
__global__ void __launch_bounds__(kBlockThreads) k_tp_reduce(const uint4* __restrict__ partials, int n, TemporalCounters* __restrict__ out) {
  unsigned long long geo = 0, hist = 0, sum = 0;
  for (int i = threadIdx.x; i < n; i += kBlockThreads) { const uint4 r = partials[i]; geo += r.x; hist += r.y; sum += r.z; }
  for (int d = 32; d > 0; d >>= 1) { geo += __shfl_down(geo, d, 64); hist += __shfl_down(hist, d, 64); sum += __shfl_down(sum, d, 64); }
  __shared__ unsigned long long part[kBlockThreads / 64][3];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { part[wave][0] = geo; part[wave][1] = hist; part[wave][2] = sum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    geo = hist = sum = 0;
    for (int w = 0; w < kBlockThreads / 64; w++) { geo += part[w][0]; hist += part[w][1]; sum += part[w][2]; }
    out->geometry = geo; out->history = hist; out->disoccluded = geo - hist; out->historySum = sum;
  }
}

}  // namespace

hipError_t launch_temporal(hipStream_t stream, const TemporalArgs& a) {
  const dim3 grid = image_grid(a.k.width, a.k.height);
  if (a.faces.nTracked > 0) k_tp_reproject<true><<<grid, kBlockThreads, 0, stream>>>(a);
  else k_tp_reproject<false><<<grid, kBlockThreads, 0, stream>>>(a);
  k_tp_reduce<<<1, kBlockThreads, 0, stream>>>(a.partials, (int)(grid.x * grid.y), a.counters);
  return launch_atrous(stream, a.k, a.colA, a.colB, a.histGuide, a.side, a.iterations, true, a.out);
}

}  // namespace pt
