// denoisekernel.h -- launch interface of denoisekernel.hip (edge-aware a-trous denoiser, pt_denoise.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_denoise.h"

namespace pt {

struct DenoiseArgs {
  DenoiseConsts k;                                              // frame size, normal power, sigmas
  const float* accum;                                           // float3 W*H, row 0 = bottom
  const float *albedo, *normal, *depth, *hits;                  // AOV sums (float3, float3, float, float)
  float nAccumulation, nSamples;                                // C = accum / nAccumulation; AOV means = sums / nSamples
  int iterations, demodulate;                                   // 0..8; iterations == 0: the caller passes demodulate = 0
  v4 *colA, *colB, *guide, *side;                               // scratch, W*H each
  float* out;                                                   // float3 W*H
};

// All passes on `stream`, asynchronously: decode, prepass and iterations when iterations > 0, final.
hipError_t launch_denoise(hipStream_t stream, const DenoiseArgs& a);

}  // namespace pt
