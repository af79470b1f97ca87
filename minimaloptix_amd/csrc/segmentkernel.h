// segmentkernel.h -- launch interface of segmentkernel.hip (segment queries, pt_segment.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_segment.h"

namespace pt {

struct SegmentArgs {
  SceneView scene;                      // nodes64 set = walk the 64-byte nodes
  const float* segments;                // n x 8 floats ax ay az bx by bz maxDist pad, 16-byte aligned (device)
  void* out;                            // closest: n x SegmentHit, 16-byte aligned; any: n x int32 (device)
  int n;                                // segments of this launch (the host cuts longer batches: indices stay 32-bit)
  unsigned long long* stackOverflow;    // per-thread spill area (reference + box distance) for trees deeper than the LDS stack, or null
};
constexpr int kSegmentMaxLaunch = 1 << 30;    // segments per launch

size_t segmentkernel_overflow_entries(int nBlocks, int stackBound);      // 0 = the tree fits the LDS stack
// mode: SEGMENT_CLOSEST / SEGMENT_ANY (pt_segment.h).  Launches min(nBlocks, ceil(n / 256)) workgroups on `stream`.
hipError_t launch_segmentquery(hipStream_t stream, const SegmentArgs& a, int nBlocks, int mode);

}  // namespace pt
