// signkernel.hip -- signed point queries for gfx950 (pt_sign.h): the table of angle-weighted pseudonormals, rebuilt on the device after
// the faces moved.  The query itself is pointkernel.hip's signed mode.
//
// The table build is three small, regular passes over arrays the topology fixes (pt_signtopo.h), one thread per element in workgroups
// of 256: per face the unit normal and the three corner angles; per welded vertex and per edge the sum over its list, in the list's
// order (a handful of 32-byte loads per thread: a valence is about 6, an edge has 2 faces); per face the 96-byte record, gathered from
// the sums.  No atomics: every word has one writer and a fixed order of additions.
#include <hip/hip_runtime.h>

#include "pt_sign.h"
#include "signkernel.h"

namespace pt {

namespace {

constexpr int kBlock = 256;
inline int grid_for(int n) { return (n + kBlock - 1) / kBlock; }

__global__ void __launch_bounds__(kBlock) k_sign_faces(const SignBuildArgs a) {
  const int f = blockIdx.x * kBlock + threadIdx.x;
  if (f >= a.nFaces) return;
  float p[9];
  for (int k = 0; k < 9; k++) p[k] = a.facePos[9 * (size_t)f + k];
  a.faces[f] = sign_face(p, a.faceIds[6 * (size_t)f] < 0);
}

// threads 0 .. nVerts: a vertex each; nVerts .. nVerts + nEdges: an edge each
__global__ void __launch_bounds__(kBlock) k_sign_gather(const SignBuildArgs a) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < a.nVerts) {
    const v3 s = sign_vertex_sum(a.faces, a.vertexCorner, a.vertexStart[i], a.vertexStart[i + 1]);
    a.vertexN[i] = mk4(s.x, s.y, s.z, 0.f);
  } else if (i - a.nVerts < a.nEdges) {
    const int e = i - a.nVerts;
    const v3 s = sign_edge_sum(a.faces, a.edgeFace, a.edgeStart[e], a.edgeStart[e + 1]);
    a.edgeN[e] = mk4(s.x, s.y, s.z, 0.f);
  }
}

__global__ void __launch_bounds__(kBlock) k_sign_records(const SignBuildArgs a) {
  const int f = blockIdx.x * kBlock + threadIdx.x;
  if (f >= a.nFaces) return;
  int ids[6];
  for (int k = 0; k < 6; k++) ids[k] = a.faceIds[6 * (size_t)f + k];
  a.table[f] = sign_record(ids, a.faces[f], a.vertexN, a.edgeN);
}

}  // namespace

hipError_t launch_sign_table(hipStream_t stream, const SignBuildArgs& a) {
  if (a.nFaces <= 0) return hipSuccess;
  k_sign_faces<<<grid_for(a.nFaces), kBlock, 0, stream>>>(a);
  if (a.nVerts + a.nEdges > 0) k_sign_gather<<<grid_for(a.nVerts + a.nEdges), kBlock, 0, stream>>>(a);
  k_sign_records<<<grid_for(a.nFaces), kBlock, 0, stream>>>(a);
  return hipGetLastError();
}

}  // namespace pt
