// pt_adaptive.h -- per-pixel code of adaptive sampling (include/moptix.h "adaptive sampling", DESIGN.md "Adaptive sampling").
//
// Every pixel keeps the number of samples added to it and the first two moments of their luminance; after each pass the relative
// standard error of the mean decides, over a 3x3 window, which pixels are sampled further.  The kernels (adaptivekernel.hip) and their
// CPU mirror (tests/adaptivesim) run exactly these functions, so they agree bit for bit.  Arithmetic: the contract of pt_math.h
// (AC4, -ffp-contract=off): every operation below is one correctly rounded binary32 operation in the order written.
//
// Buffers, per pixel p = y * width + x (row 0 = bottom, the accumulation buffer's layout):
//   count      uint32     samples added since the clear
//   moments    2 x float  s1 = sum l, s2 = sum l * l, l = dn_luminance(sample), plain adds in seed order
//   converged  uint8      sticky: set by ad_decide, cleared by moptix_adaptive_clear only
//   error      float      ad_error of the pixel, as of the last pass
#pragma once
#include "pt_denoise.h"

namespace pt {

constexpr float kAdFloor = 0.01f;      // about 2.5 / 255: below it a pixel's noise does not show in an 8-bit image

struct AdaptiveConsts {
  int width, height;
  int minSamples;
  float threshold;
};

// The argument check of moptix_render_adaptive: null when the parameters are in range, else what is wrong with them.
PT_HD const char* ad_bad_params(float threshold, int minSamples, int batch) {
  if (!__builtin_isfinite(threshold) || !(threshold >= 0.0f)) return "threshold must be finite and >= 0";
  if (minSamples < 1) return "minSamples must be >= 1";
  if (batch < 1) return "batch must be >= 1";
  return nullptr;
}

// One sample added to a pixel's moments: l = dn_luminance(sample); s1 += l; s2 += l * l.
PT_HD void ad_add_sample(v3 sample, float& s1, float& s2) {
  const float l = dn_luminance(sample);
  s1 = s1 + l;
  s2 = s2 + l * l;
}

// e = sqrt(v / n) / (m + 0.01), m = s1 / n, v = max(0, s2 / n - m * m) (biased): the relative standard error of the mean luminance.
// 0 for a pixel without samples.
PT_HD float ad_error(uint32_t count, float s1, float s2) {
  if (count == 0u) return 0.0f;
  const float n = (float)count;
  const float m = s1 / n;
  const float v = fmaxf_(0.0f, s2 / n - m * m);
  return __builtin_sqrtf(v / n) / (m + kAdFloor);
}

// Does pixel (x, y) need more samples?  n < minSamples, or the largest ad_error over the in-frame pixels of its 3x3 window (rows
// bottom to top, left to right) is above the threshold.  threshold == 0: always (no pixel ever converges).
PT_HD bool ad_needs(const AdaptiveConsts& k, const uint32_t* count, const float* moments, int x, int y) {
  const int p = y * k.width + x;
  if (count[p] < (uint32_t)k.minSamples || k.threshold == 0.0f) return true;
  float e = 0.0f;
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      const int qx = x + dx, qy = y + dy;
      if (qx < 0 || qy < 0 || qx >= k.width || qy >= k.height) continue;
      const int q = qy * k.width + qx;
      e = fmaxf_(e, ad_error(count[q], moments[2 * (size_t)q], moments[2 * (size_t)q + 1]));
    }
  return e > k.threshold;
}

// Pixel slot i of a whole-frame launch (megakernel.h item_to_pixel with partition (0, 1)): the (i & 63)-th pixel of the (i >> 6)-th
// 8x8 tile in raster order.  False for the padding slots outside the frame.
PT_HD bool ad_slot_to_pixel(int width, int height, int tilesX, int slot, int& x, int& y) {
  const int t = slot >> 6, in = slot & 63;
  x = (t % tilesX) * 8 + (in & 7); y = (t / tilesX) * 8 + (in >> 3);
  return x < width && y < height;
}
PT_HD int ad_pixel_to_slot(int tilesX, int x, int y) { return (((y >> 3) * tilesX + (x >> 3)) << 6) + ((y & 7) << 3) + (x & 7); }

// accum / count per channel (0 where count is 0): the mean a per-pixel sample count needs.
PT_HD v3 ad_mean(const float* accum, const uint32_t* count, int p) {
  const uint32_t c = count[p];
  if (c == 0u) return mk3(0.0f, 0.0f, 0.0f);
  const float n = (float)c;
  const size_t p3 = 3 * (size_t)p;
  return mk3(accum[p3] / n, accum[p3 + 1] / n, accum[p3 + 2] / n);
}

// k_resolve_rgb8's rounding of one channel of the mean (megakernel.hip: clamp, * 65535 + 0.5, high byte)
PT_HD uint8_t ad_rgb8(float mean) {
  const float v = clampf(mean, 0.f, 1.f);
  return (uint8_t)(((uint32_t)(v * 65535.0f + 0.5f)) >> 8);
}

// The pass schedule: seeds [first, first + n) of a call's list form the next pass.  The first pass of a cleared state is the
// minSamples pass; every other pass takes up to `batch` seeds.
PT_HD int ad_pass_seeds(bool statePassDone, int minSamples, int batch, int remaining) {
  const int want = statePassDone ? batch : minSamples;
  return want < remaining ? want : remaining;
}

}  // namespace pt
