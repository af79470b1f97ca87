// temporalkernel.h -- launch interface of temporalkernel.hip (temporal accumulation in front of the a-trous denoiser, pt_temporal.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_temporal.h"

namespace pt {

// moptix_temporal_info's device counters, over the pixels of the last call
struct TemporalCounters { unsigned long long geometry, history, disoccluded, historySum; };

struct TemporalArgs {
  DenoiseConsts k;                                              // frame size, normal power, sigmas
  TemporalConsts t;
  const float* accum;                                           // float3 W*H, row 0 = bottom
  const float *albedo, *normal, *depth, *hits;                  // AOV sums
  const int *primId, *matId;
  float nAccumulation, nSamples;
  int iterations, demodulate;                                   // iterations == 0: the caller passes demodulate = 0
  const v4 *prevCol, *prevGuide, *prevMom;                      // last call's history (not read when t.haveHistory == 0)
  const v4* motion;                                             // t.nSpheres entries: centre now - centre then
  TpFaces faces;                                                // per-face motion (facemotionkernel.hip wrote the records); nTracked == 0: off
  v4 *histCol, *histGuide, *histMom;                            // this call's history; histGuide also guides the a-trous passes
  v4 *colA, *colB, *side;                                       // the denoiser's scratch, W*H each
  float *motionOut, *historyOut;                                // W*H*2, W*H
  uint4* partials;                                              // one record per 16x16 workgroup: ((W + 15) / 16) * ((H + 15) / 16);
                                                                // {geometry, history, sum of h, pixels on moved faces (0 with faces off)}
  TemporalCounters* counters;                                   // written by the launch's reduction
  float* out;                                                   // float3 W*H
};

// All passes on `stream`, asynchronously: reproject + accumulate, prepass and iterations when iterations > 0, final.
// a.faces.nTracked > 0 runs the reprojection with the triangle case (pt_temporal.h tp_reproject_faces), else today's kernel.
hipError_t launch_temporal(hipStream_t stream, const TemporalArgs& a);

}  // namespace pt
