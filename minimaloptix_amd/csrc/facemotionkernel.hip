// facemotionkernel.hip -- the per-face pass of the temporal stage's option "temporal_face_motion", for gfx950: what each face moved by
// since the previous moptix_denoise_temporal call (pt_temporal.h tp_face_record), and the snapshot the next call compares with.
//
// Its own translation unit, as temporalkernel.hip: nothing of this is compiled into the trace kernels.
//
// A lane per face.  The 36-byte face stride makes a lane's nine loads strided dwords; a wave covers 64 x 36 contiguous bytes and uses
// every byte of every line it touches, so the pass stays at that until a profile says otherwise.  The records are three 16-byte vector
// stores per face.  Moved faces are counted per wave by ballot, per workgroup through LDS into one word per workgroup (a plain store),
// and k_fm_reduce, one workgroup, sums the words -- temporalkernel.hip's scheme, no atomics on one record.
#include <hip/hip_runtime.h>

#include "facemotionkernel.h"

namespace pt {

namespace {

constexpr int kBlock = kFaceMotionBlock;

__global__ void __launch_bounds__(kBlock) k_face_motion(const FaceMotionArgs a) {
  const size_t f = (size_t)blockIdx.x * kBlock + threadIdx.x;      // no early return: the whole wave takes part in the ballot
  bool moved = false;
  if (f < (size_t)a.nFaces) {
    float now[9];
    for (int i = 0; i < 9; i++) now[i] = a.now[9 * f + i];
    v4 rec[3];
    if (a.snapshotOnly) {
      rec[0] = rec[1] = rec[2] = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    } else {
      float prev[9];
      for (int i = 0; i < 9; i++) prev[i] = a.prev[9 * f + i];
      moved = tp_face_record(now, prev, rec);
    }
    for (int i = 0; i < 3; i++) a.rec[3 * f + i] = rec[i];
    for (int i = 0; i < 9; i++) a.prev[9 * f + i] = now[i];
  }
  const unsigned int n = __popcll(__ballot(moved));
  __shared__ unsigned int part[kBlock / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int s = 0;
    for (int w = 0; w < kBlock / 64; w++) s += part[w];
    a.partials[blockIdx.x] = s;
  }
}

__global__ void __launch_bounds__(kBlock) k_fm_reduce(const unsigned int* __restrict__ facePartials, int nFace, const uint4* __restrict__ pixelPartials,
                                                      int nPixel, FaceMotionCounters* __restrict__ out) {
  unsigned long long faces = 0, pixels = 0;
  for (int i = threadIdx.x; i < nFace; i += kBlock) faces += facePartials[i];
  for (int i = threadIdx.x; i < nPixel; i += kBlock) pixels += pixelPartials[i].w;
  for (int d = 32; d > 0; d >>= 1) { faces += __shfl_down(faces, d, 64); pixels += __shfl_down(pixels, d, 64); }
  __shared__ unsigned long long part[kBlock / 64][2];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { part[wave][0] = faces; part[wave][1] = pixels; }
  __syncthreads();
  if (threadIdx.x == 0) {
    faces = pixels = 0;
    for (int w = 0; w < kBlock / 64; w++) { faces += part[w][0]; pixels += part[w][1]; }
    out->movedFaces = faces; out->movedPixels = pixels;
  }
}

}  // namespace

hipError_t launch_face_motion(hipStream_t stream, const FaceMotionArgs& a) {
  if (a.nFaces <= 0) return hipSuccess;
  k_face_motion<<<face_motion_blocks((size_t)a.nFaces), kBlock, 0, stream>>>(a);
  return hipGetLastError();
}

hipError_t launch_face_motion_reduce(hipStream_t stream, const unsigned int* facePartials, int nFacePartials, const uint4* pixelPartials,
                                     int nPixelPartials, FaceMotionCounters* out) {
  k_fm_reduce<<<1, kBlock, 0, stream>>>(facePartials, nFacePartials, pixelPartials, nPixelPartials, out);
  return hipGetLastError();
}

}  // namespace pt
