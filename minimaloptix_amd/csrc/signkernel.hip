// signkernel.hip -- signed point queries for gfx950 (pt_sign.h): the table of angle-weighted pseudonormals, rebuilt on the device after
// the faces moved, and the point kernel with the sign decided in its epilogue.
//
// Its own translation unit: the closest / any kernels of pointkernel.hip are not touched by it.
//
// The table build is three small, regular passes over arrays the topology fixes (pt_signtopo.h), one thread per element in workgroups
// of 256: per face the unit normal and the three corner angles; per welded vertex and per edge the sum over its list, in the list's
// order (a handful of 32-byte loads per thread: a valence is about 6, an edge has 2 faces); per face the 96-byte record, gathered from
// the sums.  No atomics: every word has one writer and a fixed order of additions.
// pt_pointsigned is pt_pointquery's closest instantiation -- the same execution model, stack and walk (pointkernel.hip) -- followed by
// point_hit_signed: the feature of the winner, one v3 of its sign record, the sign.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pt_pointstack.h"
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

template <bool N64>
__global__ void __launch_bounds__(kPointBlockThreads) pt_pointsigned(const PointSignedArgs s) {
  __shared__ unsigned long long ldsStack[kPointWavesPerBlock * kPointLdsStack * 64];
  const PointArgs& a = s.p;
  const SceneView& sc = a.scene;
  const int gthread = blockIdx.x * kPointBlockThreads + threadIdx.x, stride = gridDim.x * kPointBlockThreads;
  PointStack st;
  st.init(ldsStack, a.stackOverflow, gthread, stride);
  const uint4* __restrict__ points = reinterpret_cast<const uint4*>(a.points);
  for (int i = gthread; i < a.n; i += stride) {           // n <= kPointMaxLaunch = 2^30 and stride <= 2^22: no overflow
    const uint4 r = points[(size_t)i];
    const float p[4] = { i2f((int32_t)r.x), i2f((int32_t)r.y), i2f((int32_t)r.z), i2f((int32_t)r.w) };
    const v3 q = mk3(p[0], p[1], p[2]);
    PointTrav tv;
    point_begin<false>(sc, q, p[3] * p[3], point_valid(p), tv);
    while (tv.node != kTravDone) point_step<false, N64>(sc, q, tv, st);
    PointHit h;
    point_hit_signed(sc, s.table, q, p[3], tv, h);
    uint4* o = static_cast<uint4*>(a.out) + 2 * (size_t)i;
    o[0] = make_uint4((uint32_t)f2i(h.dist), (uint32_t)h.prim, (uint32_t)h.mat, (uint32_t)f2i(h.u));
    o[1] = make_uint4((uint32_t)f2i(h.v), (uint32_t)f2i(h.p[0]), (uint32_t)f2i(h.p[1]), (uint32_t)f2i(h.p[2]));
  }
}

}  // namespace

hipError_t launch_sign_table(hipStream_t stream, const SignBuildArgs& a) {
  if (a.nFaces <= 0) return hipSuccess;
  k_sign_faces<<<grid_for(a.nFaces), kBlock, 0, stream>>>(a);
  if (a.nVerts + a.nEdges > 0) k_sign_gather<<<grid_for(a.nVerts + a.nEdges), kBlock, 0, stream>>>(a);
  k_sign_records<<<grid_for(a.nFaces), kBlock, 0, stream>>>(a);
  return hipGetLastError();
}

hipError_t launch_pointsigned(hipStream_t stream, const PointSignedArgs& a, int nBlocks) {
  const int blocks = (int)std::min<long long>(nBlocks, ((long long)a.p.n + kPointBlockThreads - 1) / kPointBlockThreads);
  if (a.p.scene.nodes64 != nullptr) pt_pointsigned<true><<<blocks, kPointBlockThreads, 0, stream>>>(a);
  else                              pt_pointsigned<false><<<blocks, kPointBlockThreads, 0, stream>>>(a);
  return hipGetLastError();
}

}  // namespace pt
