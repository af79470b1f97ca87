// adaptivekernel.hip -- adaptive sampling (pt_adaptive.h) for gfx950: the fused reduction that stands in for k_reduce_samples in an
// adaptive pass, the mask kernel that decides which pixels are sampled further, the count-aware mean and 8-bit resolve.
//
// Its own translation unit, as aovkernel.hip, denoisekernel.hip and temporalkernel.hip: the trace kernels' register allocation moves
// with code they never run (NOTEBOOK.md), so nothing of this is compiled into them.
//
// k_ad_reduce: a lane per pixel SLOT in slot order, as k_reduce_samples -- consecutive lanes read consecutive 12-byte entries of each
// seed's row of the per-sample buffer, so the loads stay coalesced whatever the active set looks like; a slot whose pixel is
// converged (it was not handed out in this pass) or outside the frame is skipped.  One read of the buffer serves the colour sum and
// the luminance moments.
// k_ad_mask: the denoiser's mapping (image_tile.h), a lane per pixel, a 256-thread workgroup covers 16x16 pixels as four 8x8 tiles, one per wave --
// the wave's tile is a tile of the trace kernels' slot numbering, so lane l of the wave owns slot tile * 64 + l and the keys are written
// as one 256-byte row per wave.  The 3x3 window's errors are recomputed from count / moments (nine 12-byte loads per pixel, served
// by the L1/L2: a wave's window is a 10x10-pixel neighbourhood) instead of from an error buffer written by a kernel of its own: that
// would add a launch and a 4-byte round trip per pixel and pass to save a square root and two divisions per tap, on 2 M pixels.
// The totals are reduced per wave (ballot / shuffle), per workgroup through LDS into one 16-byte record (a plain vector store), and
// summed by k_ad_fold, one workgroup -- not by one atomic per wave on one line (temporalkernel.hip tells what that cost).
#include <hip/hip_runtime.h>

#include "adaptivekernel.h"
#include "image_tile.h"

namespace pt {

namespace {

constexpr int kBlockThreads = kImageBlockThreads;

__global__ void __launch_bounds__(kBlockThreads) k_ad_reduce(const AdaptiveArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nItems) return;
  if (a.workCounter[1] != 0) return;      // the trace kernel gave up (watchdog): its sample buffer is incomplete
  int x, y;
  if (!ad_slot_to_pixel(a.k.width, a.k.height, a.tilesX, i, x, y)) return;
  const int pixel = y * a.k.width + x;
  if (a.converged[pixel]) return;         // not handed out in this pass
  float* px = a.accum + 3 * (size_t)pixel;
  float* mo = a.moments + 2 * (size_t)pixel;
  v3 acc = mk3(px[0], px[1], px[2]);
  float s1 = mo[0], s2 = mo[1];
  for (int k = 0; k < a.nSeeds; k++) {
    const float* sp = a.sampleBuf + 3 * ((size_t)k * a.nItems + i);
    const v3 s = mk3(sp[0], sp[1], sp[2]);
    acc = acc + s;
    ad_add_sample(s, s1, s2);
  }
  px[0] = acc.x; px[1] = acc.y; px[2] = acc.z;
  mo[0] = s1; mo[1] = s2;
  a.count[pixel] += (uint32_t)a.nSeeds;
}

__global__ void __launch_bounds__(kBlockThreads) k_ad_mask(const AdaptiveArgs a, int decide) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int x, y, tx, ty;
  const bool inside = image_pixel(a.k.width, a.k.height, x, y, tx, ty);      // no early return: the whole wave takes part in the reduction
  bool active = false, conv = false;
  unsigned int cmin = 0xffffffffu, cmax = 0u;
  if (inside) {
    const int p = y * a.k.width + x;
    const uint32_t n = a.count[p];
    conv = a.converged[p] != 0;
    if (decide && !conv && !ad_needs(a.k, a.count, a.moments, x, y)) { conv = true; a.converged[p] = 1; }
    a.error[p] = ad_error(n, a.moments[2 * (size_t)p], a.moments[2 * (size_t)p + 1]);
    active = !conv;
    const int slot = ((ty * a.tilesX + tx) << 6) + lane;     // ad_pixel_to_slot(a.tilesX, x, y)
    a.key[slot] = active ? (a.tileCost ? min(a.tileCost[slot], 0xfffffffeu) : 0u) + 1u : 0u;
    cmin = cmax = n;
  }
  const unsigned int nActive = __popcll(__ballot(active)), nConv = __popcll(__ballot(conv));
  for (int d = 32; d > 0; d >>= 1) { cmin = min(cmin, __shfl_down(cmin, d, 64)); cmax = max(cmax, __shfl_down(cmax, d, 64)); }
  __shared__ unsigned int part[kBlockThreads / 64][4];
  if (lane == 0) { part[wave][0] = nActive; part[wave][1] = nConv; part[wave][2] = cmin; part[wave][3] = cmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint4 r = make_uint4(0u, 0u, 0xffffffffu, 0u);
    for (int w = 0; w < kBlockThreads / 64; w++) { r.x += part[w][0]; r.y += part[w][1]; r.z = min(r.z, part[w][2]); r.w = max(r.w, part[w][3]); }
    a.partials[blockIdx.y * gridDim.x + blockIdx.x] = r;
  }
}

// One workgroup: the per-workgroup records {active, converged, min count, max count} -> AdaptiveTotals.
__global__ void __launch_bounds__(kBlockThreads) k_ad_fold(const uint4* __restrict__ partials, int n, AdaptiveTotals* __restrict__ out) {
  unsigned int act = 0, conv = 0, cmin = 0xffffffffu, cmax = 0;
  for (int i = threadIdx.x; i < n; i += kBlockThreads) { const uint4 r = partials[i]; act += r.x; conv += r.y; cmin = min(cmin, r.z); cmax = max(cmax, r.w); }
  for (int d = 32; d > 0; d >>= 1) {
    act += __shfl_down(act, d, 64); conv += __shfl_down(conv, d, 64);
    cmin = min(cmin, __shfl_down(cmin, d, 64)); cmax = max(cmax, __shfl_down(cmax, d, 64));
  }
  __shared__ unsigned int part[kBlockThreads / 64][4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { part[wave][0] = act; part[wave][1] = conv; part[wave][2] = cmin; part[wave][3] = cmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    act = conv = cmax = 0; cmin = 0xffffffffu;
    for (int w = 0; w < kBlockThreads / 64; w++) { act += part[w][0]; conv += part[w][1]; cmin = min(cmin, part[w][2]); cmax = max(cmax, part[w][3]); }
    out->active = act; out->converged = conv; out->minCount = cmin; out->maxCount = cmax;
  }
}

__global__ void __launch_bounds__(kBlockThreads) k_ad_mean(const AdaptiveArgs a, float* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.k.width * a.k.height) return;
  const v3 m = ad_mean(a.accum, a.count, p);
  float* o = out + 3 * (size_t)p;
  o[0] = m.x; o[1] = m.y; o[2] = m.z;
}

// k_resolve_rgb8 (megakernel.hip) with the pixel's own count as the divisor: clamp, 16-bit round, high byte, rows flipped
__global__ void __launch_bounds__(kBlockThreads) k_ad_resolve_rgb8(const AdaptiveArgs a, uint8_t* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.k.width * a.k.height) return;
  const int i = p / a.k.width, j = p % a.k.width;
  const v3 m = ad_mean(a.accum, a.count, p);
  uint8_t* dst = out + 3 * ((size_t)(a.k.height - i - 1) * a.k.width + j);
  dst[0] = ad_rgb8(m.x); dst[1] = ad_rgb8(m.y); dst[2] = ad_rgb8(m.z);
}

}  // namespace

hipError_t launch_adaptive_reduce(hipStream_t stream, const AdaptiveArgs& a) {
  k_ad_reduce<<<(a.nItems + kBlockThreads - 1) / kBlockThreads, kBlockThreads, 0, stream>>>(a);
  return hipGetLastError();
}

hipError_t launch_adaptive_mask(hipStream_t stream, const AdaptiveArgs& a, int decide) {
  const dim3 grid = image_grid(a.k.width, a.k.height);
  k_ad_mask<<<grid, kBlockThreads, 0, stream>>>(a, decide);
  k_ad_fold<<<1, kBlockThreads, 0, stream>>>(a.partials, (int)(grid.x * grid.y), a.totals);
  return hipGetLastError();
}

hipError_t launch_adaptive_mean(hipStream_t stream, const AdaptiveArgs& a, float* out) {
  const int n = a.k.width * a.k.height;
  k_ad_mean<<<(n + kBlockThreads - 1) / kBlockThreads, kBlockThreads, 0, stream>>>(a, out);
  return hipGetLastError();
}

hipError_t launch_adaptive_resolve_rgb8(hipStream_t stream, const AdaptiveArgs& a, uint8_t* out) {
  const int n = a.k.width * a.k.height;
  k_ad_resolve_rgb8<<<(n + kBlockThreads - 1) / kBlockThreads, kBlockThreads, 0, stream>>>(a, out);
  return hipGetLastError();
}

}  // namespace pt
