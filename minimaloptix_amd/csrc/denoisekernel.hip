// denoisekernel.hip -- edge-aware a-trous denoiser (pt_denoise.h) for gfx950: the first-hit AOVs guide a 5x5 a-trous filter of the
// demodulated beauty mean with SVGF's luminance-variance edge stop.  The prepass / iterate / final kernels and their launch chain
// (launch_atrous) serve the spatial entry (launch_denoise: decode + chain) and the temporal one (temporalkernel.hip: reproject + reduce +
// chain, with the prepass that keeps the temporal variance).
//
// Its own translation unit, as aovkernel.hip: the trace kernels' register allocation moves with code they never run (NOTEBOOK.md),
// so nothing of this pass is compiled into them.
//
// One kernel per pass, a lane per pixel in the mapping of image_tile.h, so a wave's taps at step 2^i fall on 8-row blocks of the 16-byte
// col and guide buffers (two loads per tap) that neighbouring lanes share in the L1.  At 1920x1080 each float4 buffer is 33 MB: all four
// fit the Infinity Cache, and no pass goes to HBM for its taps.
#include <hip/hip_runtime.h>

#include "denoisekernel.h"
#include "image_tile.h"
#include "pt_temporal.h"

namespace pt {

namespace {

constexpr int kBlockThreads = kImageBlockThreads;

__global__ void __launch_bounds__(kBlockThreads) k_dn_decode(const DenoiseArgs a) {
  int x, y;
  if (!image_pixel(a.k.width, a.k.height, x, y)) return;
  const int p = y * a.k.width + x;
  v4 col, guide, side;
  dn_decode(a.accum, a.albedo, a.normal, a.depth, a.hits, a.nAccumulation, a.nSamples, a.demodulate, p, col, guide, side);
  a.colA[p] = col; a.guide[p] = guide; a.side[p] = side;
}

template <bool kTemporalVariance>
__device__ __forceinline__ void prepass_pixel(const DenoiseConsts& k, const v4* __restrict__ colIn, const v4* __restrict__ guide,
                                              v4* __restrict__ colOut, v4* __restrict__ side) {
  int x, y;
  if (!image_pixel(k.width, k.height, x, y)) return;
  const int p = y * k.width + x;
  v4 c = colIn[p];
  if (dn_geometry(guide[p])) {
    float g;
    c.w = kTemporalVariance ? tp_prepass(k, colIn, guide, x, y, g) : dn_prepass(k, colIn, guide, x, y, g);
    side[p].w = g;
  }
  colOut[p] = c;
}
__global__ void __launch_bounds__(kBlockThreads) k_dn_prepass(const DenoiseConsts k, const v4* __restrict__ colIn, const v4* __restrict__ guide,
                                                             v4* __restrict__ colOut, v4* __restrict__ side) {
  prepass_pixel<false>(k, colIn, guide, colOut, side);
}
__global__ void __launch_bounds__(kBlockThreads) k_tp_prepass(const DenoiseConsts k, const v4* __restrict__ colIn, const v4* __restrict__ guide,
                                                             v4* __restrict__ colOut, v4* __restrict__ side) {
  prepass_pixel<true>(k, colIn, guide, colOut, side);
}

__global__ void __launch_bounds__(kBlockThreads) k_dn_iterate(const DenoiseConsts k, const v4* __restrict__ colIn, const v4* __restrict__ guide,
                                                             const v4* __restrict__ side, v4* __restrict__ colOut, int step) {
  int x, y;
  if (!image_pixel(k.width, k.height, x, y)) return;
  const int p = y * k.width + x;
  colOut[p] = dn_geometry(guide[p]) ? dn_iterate(k, colIn, guide, x, y, step, side[p].w) : colIn[p];
}

__global__ void __launch_bounds__(kBlockThreads) k_dn_final(const DenoiseConsts k, const v4* __restrict__ col, const v4* __restrict__ guide,
                                                           const v4* __restrict__ side, float* __restrict__ out) {
  int x, y;
  if (!image_pixel(k.width, k.height, x, y)) return;
  const int p = y * k.width + x;
  dn_final(col[p], guide[p], side[p], out, p);
}

}  // namespace

hipError_t launch_atrous(hipStream_t stream, const DenoiseConsts& k, v4* colA, v4* colB, const v4* guide, v4* side, int iterations,
                         bool temporalVariance, float* out) {
  const dim3 grid = image_grid(k.width, k.height);
  v4* cur = colA;
  if (iterations > 0) {
    if (temporalVariance) k_tp_prepass<<<grid, kBlockThreads, 0, stream>>>(k, colA, guide, colB, side);
    else k_dn_prepass<<<grid, kBlockThreads, 0, stream>>>(k, colA, guide, colB, side);
    cur = colB;
    for (int i = 0; i < iterations; i++) {
      v4* next = cur == colA ? colB : colA;
      k_dn_iterate<<<grid, kBlockThreads, 0, stream>>>(k, cur, guide, side, next, 1 << i);
      cur = next;
    }
  }
  k_dn_final<<<grid, kBlockThreads, 0, stream>>>(k, cur, guide, side, out);
  return hipGetLastError();
}

hipError_t launch_denoise(hipStream_t stream, const DenoiseArgs& a) {
  k_dn_decode<<<image_grid(a.k.width, a.k.height), kBlockThreads, 0, stream>>>(a);
  return launch_atrous(stream, a.k, a.colA, a.colB, a.guide, a.side, a.iterations, false, a.out);
}

}  // namespace pt
