// facemotionkernel.h -- launch interface of facemotionkernel.hip (per-face displacement records and the position snapshot of the
// temporal stage's option "temporal_face_motion", pt_temporal.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_temporal.h"

namespace pt {

constexpr int kFaceMotionBlock = 256;
inline int face_motion_blocks(size_t nFaces) { return (int)((nFaces + kFaceMotionBlock - 1) / kFaceMotionBlock); }

// moptix_temporal_face_info's device counters, of the last call that ran the face pass
struct FaceMotionCounters { unsigned long long movedFaces, movedPixels; };

struct FaceMotionArgs {
  const float* now;               // the faces' positions, 9 floats per face
  float* prev;                    // the snapshot, same layout: read, then overwritten with `now`
  v4* rec;                        // three records per face (pt_temporal.h TpFaces)
  int nFaces;
  int snapshotOnly;               // no snapshot to compare with: zero records, prev = now
  unsigned int* partials;         // moved faces per workgroup: face_motion_blocks(nFaces) words
};

// Asynchronously on `stream`: one lane per face.
hipError_t launch_face_motion(hipStream_t stream, const FaceMotionArgs& a);
// One workgroup: the face pass's partials and the fourth word of the reprojection's per-workgroup records -> counters.
hipError_t launch_face_motion_reduce(hipStream_t stream, const unsigned int* facePartials, int nFacePartials, const uint4* pixelPartials,
                                     int nPixelPartials, FaceMotionCounters* out);

}  // namespace pt
