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

// All passes on `stream`, asynchronously: decode, then the a-trous chain.
hipError_t launch_denoise(hipStream_t stream, const DenoiseArgs& a);

// The a-trous chain over colA (the decoded or reprojected signal): prepass colA -> colB and `iterations` ping-pong passes at step 2^i when
// iterations > 0, final -> out.  temporalVariance: the prepass keeps col.w where tp_reproject left a temporal variance (pt_temporal.h
// tp_prepass) instead of taking the 3x3 spatial estimate everywhere.  This is the one place that says which buffer is current.
hipError_t launch_atrous(hipStream_t stream, const DenoiseConsts& k, v4* colA, v4* colB, const v4* guide, v4* side, int iterations,
                         bool temporalVariance, float* out);

}  // namespace pt
