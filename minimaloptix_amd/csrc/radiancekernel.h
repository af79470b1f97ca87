// radiancekernel.h -- launch interface of radiancekernel.hip (radiance queries, pt_radiance.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_types.h"

namespace pt {

// One launch: the samples s = 0 .. nSamples-1 of this pass for the rays i = 0 .. n-1 of this launch.  Work item k = i * nSamples + s.
struct RadianceArgs {
  SceneView scene;                // nodes64 set = walk the 64-byte nodes
  const float* rays;              // n x 8 floats, 16-byte aligned (device)
  const int* seeds;               // seeds mode: this pass's nSamples seeds (device), else null
  const uint32_t* states;         // states mode: the state of (i, s) is states[i * statesStride + s] (device), else null
  size_t statesStride;            // samples per ray of the whole call
  float* scratch;                 // per-sample records r g b t, n * nSamples x 16 bytes: work item k writes record k
  float* out;                     // n x 4 floats (device, 16-byte aligned)
  int* workCounter;               // zeroed before the launch
  int n, nSamples;                // n * nSamples <= kRadianceMaxWork
  uint32_t indexBase;             // seeds mode: ray i's index is indexBase + i (mod 2^32)
  uint32_t flags;                 // RADIANCE_CLAMP
  int firstPass;                  // the reduction starts a ray's sum from +0 (else from the output so far)
  int exitThreshold, leafThreshold;     // as LaunchArgs': when a wave leaves the traversal loop, when it runs the leaf pass (time only)
  int* stackOverflow;             // per-thread spill area for trees deeper than the LDS stack (or null), sized for the grid's cap
};
constexpr long long kRadianceMaxWork = 1ll << 30;     // work items per launch: the counter and the record index stay 32-bit

size_t radiancekernel_overflow_ints(int nBlocks, int stackBound);      // 0 = the tree fits the LDS stack
// Launches min(nBlocks, ceil(n * nSamples / 256)) workgroups of the trace kernel on `stream`, then the ordered reduction of the records.
hipError_t launch_radiance(hipStream_t stream, const RadianceArgs& a, int nBlocks);

}  // namespace pt
