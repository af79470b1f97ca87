// adaptivekernel.h -- launch interface of adaptivekernel.hip (adaptive sampling, pt_adaptive.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_adaptive.h"

namespace pt {

// What the mask launch counts over the in-frame pixels: pixels still active, pixels converged, smallest and largest sample count.
struct AdaptiveTotals { unsigned int active, converged, minCount, maxCount; };

struct AdaptiveArgs {
  AdaptiveConsts k;                       // frame size, minSamples, threshold
  int nItems, tilesX;                     // pixel slots of the whole frame (tiles * 64), 8x8 tiles per row
  float* accum;                           // float3 W*H, row 0 = bottom
  uint32_t* count;                        // W*H
  float* moments;                         // W*H*2
  float* error;                           // W*H
  uint8_t* converged;                     // W*H
  // the pass that k_ad_reduce folds: the trace kernel's per-sample buffer [nSeeds][nItems] float3 and its work counter ([1] = watchdog flag)
  const float* sampleBuf; const int* workCounter; int nSeeds;
  // the order list's sort keys, one per pixel slot (padding slots keep the 0 they were cleared to), and the depth history they are made of
  unsigned int* key; const unsigned int* tileCost;      // tileCost may be null: no history
  uint4* partials;                        // one record per 16x16 workgroup of the mask kernel
  AdaptiveTotals* totals;                 // written by the mask launch's fold
};

// accum += samples, moments += luminance moments, count += nSeeds for every pixel slot that is inside the frame and not converged: the
// adaptive passes' stand-in for launch_reduce_samples (same adds in the same order, same watchdog test).
hipError_t launch_adaptive_reduce(hipStream_t stream, const AdaptiveArgs& a);
// decide != 0: pixels that need no more samples become converged.  Either way: error, the slots' sort keys (active: depth history + 1,
// else 0) and the totals.
hipError_t launch_adaptive_mask(hipStream_t stream, const AdaptiveArgs& a, int decide);
hipError_t launch_adaptive_mean(hipStream_t stream, const AdaptiveArgs& a, float* out);              // W*H*3: accum / count
hipError_t launch_adaptive_resolve_rgb8(hipStream_t stream, const AdaptiveArgs& a, uint8_t* out);    // W*H*3 bytes, row 0 = top

}  // namespace pt
