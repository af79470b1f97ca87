// adaptivesim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of moptix_render_adaptive (minimaloptix_amd/csrc/adaptivekernel.hip and the pass
// schedule of api_adaptive.hip): the same per-pixel code (pt_adaptive.h), compiled for the host and run pass by pass over caller-given
// per-seed sample images, with the state kept in an object between calls.  A sample image is what one seed adds to a zero
// accumulator -- the clamped colour the trace kernel stores -- so the mirror needs no renderer of its own.  The GPU tests compare the
// device's buffers and stats with this bit for bit.  It is not part of the product: nothing under minimaloptix_amd/ builds or loads it.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/moptix.h"
#include "../../minimaloptix_amd/csrc/pt_adaptive.h"

using namespace pt;

namespace {

struct Sim {
  int width = 0, height = 0;
  std::vector<float> accum, moments, error;
  std::vector<uint32_t> count;
  std::vector<uint8_t> converged;
  bool have = false;
};

// the argument check of moptix_render_adaptive (pt_adaptive.h: the code the library runs)
int bad_params(const moptix_adaptive_params* p) { return !p || ad_bad_params(p->threshold, p->minSamples, p->batch) != nullptr; }

}  // namespace

extern "C" {

void* adaptivesim_create() { return new Sim; }
void adaptivesim_destroy(void* h) { delete static_cast<Sim*>(h); }

// moptix_adaptive_clear (and the first call at a frame size)
void adaptivesim_clear(void* h, int width, int height) {
  Sim& s = *static_cast<Sim*>(h);
  const size_t px = (size_t)width * height;
  s.width = width; s.height = height; s.have = false;
  s.accum.assign(3 * px, 0.0f); s.moments.assign(2 * px, 0.0f); s.error.assign(px, 0.0f);
  s.count.assign(px, 0u); s.converged.assign(px, 0);
}

int adaptivesim_check_params(const moptix_adaptive_params* p) { return bad_params(p) ? MOPTIX_ERR_INVALID : MOPTIX_OK; }

// samples: [nSeeds][height][width][3], the image each seed of the call's list adds.  Returns MOPTIX_OK or MOPTIX_ERR_INVALID.
int adaptivesim_render(void* h, int width, int height, const float* samples, int nSeeds, const moptix_adaptive_params* p, moptix_adaptive_stats* out) {
  Sim& s = *static_cast<Sim*>(h);
  if (out) memset(out, 0, sizeof(*out));
  if (bad_params(p) || nSeeds < 0 || (nSeeds > 0 && !samples) || width <= 0 || height <= 0) return MOPTIX_ERR_INVALID;
  if (s.width != width || s.height != height) adaptivesim_clear(h, width, height);
  const int px = width * height;
  AdaptiveConsts k; k.width = width; k.height = height; k.minSamples = p->minSamples; k.threshold = p->threshold;
  uint64_t passes = 0, traced = 0;
  // k_ad_mask: decide, error, totals
  uint64_t active = 0;
  auto mask = [&](bool decide) {
    std::vector<uint8_t> conv(s.converged);
#pragma omp parallel for schedule(static)
    for (int q = 0; q < px; q++) {
      const int x = q % width, y = q / width;
      if (decide && !s.converged[q] && !ad_needs(k, s.count.data(), s.moments.data(), x, y)) conv[q] = 1;
      s.error[q] = ad_error(s.count[q], s.moments[2 * (size_t)q], s.moments[2 * (size_t)q + 1]);
    }
    s.converged.swap(conv);
    active = 0;
    for (int q = 0; q < px; q++) active += s.converged[q] ? 0 : 1;
  };
  mask(false);
  for (int first = 0; first < nSeeds && active > 0;) {
    const int n = ad_pass_seeds(s.have, p->minSamples, p->batch, nSeeds - first);
    s.have = true;
    // k_ad_reduce: the active pixels take all seeds of the pass, in seed order
#pragma omp parallel for schedule(static)
    for (int q = 0; q < px; q++) {
      if (s.converged[q]) continue;
      v3 acc = mk3(s.accum[3 * (size_t)q], s.accum[3 * (size_t)q + 1], s.accum[3 * (size_t)q + 2]);
      float s1 = s.moments[2 * (size_t)q], s2 = s.moments[2 * (size_t)q + 1];
      for (int j = 0; j < n; j++) {
        const float* sp = samples + 3 * ((size_t)(first + j) * px + q);
        const v3 c = mk3(sp[0], sp[1], sp[2]);
        acc = acc + c;
        ad_add_sample(c, s1, s2);
      }
      s.accum[3 * (size_t)q] = acc.x; s.accum[3 * (size_t)q + 1] = acc.y; s.accum[3 * (size_t)q + 2] = acc.z;
      s.moments[2 * (size_t)q] = s1; s.moments[2 * (size_t)q + 1] = s2;
      s.count[q] += (uint32_t)n;
    }
    traced += active * (uint64_t)n;
    first += n; passes++;
    mask(true);
  }
  if (out) {
    uint32_t cmin = 0xffffffffu, cmax = 0; uint64_t conv = 0;
    for (int q = 0; q < px; q++) { cmin = s.count[q] < cmin ? s.count[q] : cmin; cmax = s.count[q] > cmax ? s.count[q] : cmax; conv += s.converged[q] ? 1 : 0; }
    out->passes = passes; out->samplesTraced = traced; out->samplesUniform = (uint64_t)px * (uint64_t)nSeeds;
    out->activePixelsLast = active; out->convergedPixels = conv; out->minCount = cmin; out->maxCount = cmax;
  }
  return MOPTIX_OK;
}

// the state, as moptix_accum_read / moptix_adaptive_read return it; NULL members are skipped
void adaptivesim_read(void* h, float* accum, uint32_t* count, float* moments, float* error, uint8_t* converged) {
  const Sim& s = *static_cast<Sim*>(h);
  if (accum) memcpy(accum, s.accum.data(), sizeof(float) * s.accum.size());
  if (count) memcpy(count, s.count.data(), sizeof(uint32_t) * s.count.size());
  if (moments) memcpy(moments, s.moments.data(), sizeof(float) * s.moments.size());
  if (error) memcpy(error, s.error.data(), sizeof(float) * s.error.size());
  if (converged) memcpy(converged, s.converged.data(), s.converged.size());
}

// moptix_adaptive_mean and moptix_adaptive_resolve_rgb8
void adaptivesim_mean(void* h, float* mean, uint8_t* rgb8) {
  const Sim& s = *static_cast<Sim*>(h);
  for (int q = 0; q < s.width * s.height; q++) {
    const v3 m = ad_mean(s.accum.data(), s.count.data(), q);
    if (mean) { mean[3 * (size_t)q] = m.x; mean[3 * (size_t)q + 1] = m.y; mean[3 * (size_t)q + 2] = m.z; }
    if (rgb8) {
      const int i = q / s.width, j = q % s.width;
      uint8_t* dst = rgb8 + 3 * ((size_t)(s.height - i - 1) * s.width + j);
      dst[0] = ad_rgb8(m.x); dst[1] = ad_rgb8(m.y); dst[2] = ad_rgb8(m.z);
    }
  }
}

}  // extern "C"
