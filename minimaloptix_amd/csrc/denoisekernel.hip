// denoisekernel.hip -- edge-aware a-trous denoiser (pt_denoise.h) for gfx950: the first-hit AOVs guide a 5x5 a-trous filter of the
// demodulated beauty mean with SVGF's luminance-variance edge stop.
//
// Its own translation unit, as aovkernel.hip: the trace kernels' register allocation moves with code they never run (NOTEBOOK.md),
// so nothing of this pass is compiled into them.
//
// One kernel per pass, a lane per pixel: a 256-thread workgroup covers 16x16 pixels as four 8x8 tiles, one per wave, so a wave's
// taps at step 2^i fall on 8-row blocks of the 16-byte col and guide buffers (two loads per tap) that neighbouring lanes share in the
// L1.  At 1920x1080 each float4 buffer is 33 MB: all four fit the Infinity Cache, and no pass goes to HBM for its taps.
#include <hip/hip_runtime.h>

#include "denoisekernel.h"

namespace pt {

namespace {

constexpr int kBlockThreads = 256;

__device__ __forceinline__ bool dn_pixel(int width, int height, int& x, int& y) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  x = (blockIdx.x * 2 + (wave & 1)) * 8 + (lane & 7);
  y = (blockIdx.y * 2 + (wave >> 1)) * 8 + (lane >> 3);
  return x < width && y < height;
}

__global__ void __launch_bounds__(kBlockThreads) k_dn_decode(const DenoiseArgs a) {
  int x, y;
  if (!dn_pixel(a.k.width, a.k.height, x, y)) return;
  const int p = y * a.k.width + x;
  v4 col, guide, side;
  dn_decode(a.accum, a.albedo, a.normal, a.depth, a.hits, a.nAccumulation, a.nSamples, a.demodulate, p, col, guide, side);
  a.colA[p] = col; a.guide[p] = guide; a.side[p] = side;
}

__global__ void __launch_bounds__(kBlockThreads) k_dn_prepass(const DenoiseConsts k, const v4* __restrict__ colIn, const v4* __restrict__ guide,
                                                             v4* __restrict__ colOut, v4* __restrict__ side) {
  int x, y;
  if (!dn_pixel(k.width, k.height, x, y)) return;
  const int p = y * k.width + x;
  v4 c = colIn[p];
  if (dn_geometry(guide[p])) {
    float g;
    c.w = dn_prepass(k, colIn, guide, x, y, g);
    side[p].w = g;
  }
  colOut[p] = c;
}

__global__ void __launch_bounds__(kBlockThreads) k_dn_iterate(const DenoiseConsts k, const v4* __restrict__ colIn, const v4* __restrict__ guide,
                                                             const v4* __restrict__ side, v4* __restrict__ colOut, int step) {
  int x, y;
  if (!dn_pixel(k.width, k.height, x, y)) return;
  const int p = y * k.width + x;
  colOut[p] = dn_geometry(guide[p]) ? dn_iterate(k, colIn, guide, x, y, step, side[p].w) : colIn[p];
}

__global__ void __launch_bounds__(kBlockThreads) k_dn_final(const DenoiseConsts k, const v4* __restrict__ col, const v4* __restrict__ guide,
                                                           const v4* __restrict__ side, float* __restrict__ out) {
  int x, y;
  if (!dn_pixel(k.width, k.height, x, y)) return;
  const int p = y * k.width + x;
  dn_final(col[p], guide[p], side[p], out, p);
}

}  // namespace

hipError_t launch_denoise(hipStream_t stream, const DenoiseArgs& a) {
  const dim3 grid((a.k.width + 15) / 16, (a.k.height + 15) / 16);
  k_dn_decode<<<grid, kBlockThreads, 0, stream>>>(a);
  v4* cur = a.colA;
  if (a.iterations > 0) {
    k_dn_prepass<<<grid, kBlockThreads, 0, stream>>>(a.k, a.colA, a.guide, a.colB, a.side);
    cur = a.colB;
    for (int i = 0; i < a.iterations; i++) {
      v4* next = cur == a.colA ? a.colB : a.colA;
      k_dn_iterate<<<grid, kBlockThreads, 0, stream>>>(a.k, cur, a.guide, a.side, next, 1 << i);
      cur = next;
    }
  }
  k_dn_final<<<grid, kBlockThreads, 0, stream>>>(a.k, cur, a.guide, a.side, a.out);
  return hipGetLastError();
}

}  // namespace pt
