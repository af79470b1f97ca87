// pt_signtopo.h -- the connectivity the sign table (pt_sign.h) is gathered over, taken once from the face positions.  Host only: the
// library (api_sign.hip) and the CPU mirror (tests/hostsim/signsim.cpp) build it with this one function, as they share the refit's plan
// (pt_refit.h refit_plan_levels).
//
//   weld       two corners are one vertex when their three position words are equal, -0 taken as +0; ids in order of first appearance
//              by (face, corner)
//   degenerate a face with two corners welded together, or whose normal is zero or non-finite by sign_face's test on the positions the
//              topology is taken from.  It joins no list below, its ids are -1 and its record is zero for the topology's life
//   edge       an unordered pair of welded ids; ids in order of first appearance by (face, slot 01, 02, 12) over the other faces
//   lists      per welded vertex its corners (3 * face + corner) ascending; per edge its faces ascending: the order of pt_sign.h's sums
//   report     boundary edges (one face), non-manifold edges (more than two), flipped edges (two faces that run along the edge in the
//              same direction), degenerate faces, closed = none of these and at least one face, and the signed volume
//              sum dot(p0, cross(p1, p2)) / 6 in binary64 (negative: the mesh is wound inwards and every sign comes out flipped)
#pragma once
#include <cstring>
#include <unordered_map>
#include <vector>

#include "pt_sign.h"

namespace pt {

struct SignTopology {
  int nFaces = 0, nVerts = 0, nEdges = 0;
  std::vector<int> faceIds;                                     // six per face: welded vertex ids 0 1 2, edge ids 01 02 12; -1 x 6 = degenerate
  std::vector<int> vertexStart, vertexCorner, edgeStart, edgeFace;      // CSR: nVerts + 1, corners; nEdges + 1, faces
  unsigned boundaryEdges = 0, nonManifoldEdges = 0, flippedEdges = 0, degenerateFaces = 0;
  double signedVolume = 0.0;
  bool closed() const { return nFaces > 0 && !boundaryEdges && !nonManifoldEdges && !flippedEdges && !degenerateFaces; }
};

namespace signtopo {
struct Key { uint32_t w[3]; bool operator==(const Key& o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2]; } };
struct KeyHash {
  size_t operator()(const Key& k) const {
    unsigned long long h = 1469598103934665603ull;
    for (int i = 0; i < 3; i++) { h ^= k.w[i]; h *= 1099511628211ull; }
    return (size_t)(h ^ (h >> 29));
  }
};
}  // namespace signtopo

// facePos: nine floats per face, p0 p1 p2
inline void sign_build_topology(const float* facePos, size_t nFaces, SignTopology& t) {
  t = SignTopology();
  t.nFaces = (int)nFaces;
  t.faceIds.assign(6 * nFaces, -1);
  std::unordered_map<signtopo::Key, int, signtopo::KeyHash> weld;
  weld.reserve(2 * nFaces + 16);
  std::vector<int> corner(3 * nFaces);
  for (size_t c = 0; c < 3 * nFaces; c++) {
    signtopo::Key k;
    memcpy(k.w, facePos + 3 * c, sizeof(k.w));
    for (int i = 0; i < 3; i++) if (k.w[i] == 0x80000000u) k.w[i] = 0u;
    corner[c] = weld.emplace(k, (int)weld.size()).first->second;
  }
  t.nVerts = (int)weld.size();
  // edges of the faces that count; per edge its number of faces and the directions of the first two
  struct Edge { int faces; bool dir[2]; };
  std::unordered_map<unsigned long long, int> edgeId;
  edgeId.reserve(3 * nFaces + 16);
  std::vector<Edge> edges;
  static const int from[3] = { 0, 2, 1 }, to[3] = { 1, 0, 2 };      // slots 01, 02, 12 in the face's own direction: 0 -> 1, 2 -> 0, 1 -> 2
  double vol = 0.0;
  for (size_t f = 0; f < nFaces; f++) {
    const float* p = facePos + 9 * f;
    const double a[3] = { p[0], p[1], p[2] }, b[3] = { p[3], p[4], p[5] }, c[3] = { p[6], p[7], p[8] };
    vol += a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
    const int* v = &corner[3 * f];
    const bool dead = v[0] == v[1] || v[1] == v[2] || v[0] == v[2] || !length_is_nonzero(sign_face(p, false).un);
    if (dead) { t.degenerateFaces++; continue; }
    int* ids = &t.faceIds[6 * f];
    for (int s = 0; s < 3; s++) {
      ids[s] = v[s];
      const int x = v[from[s]], y = v[to[s]];
      const unsigned long long key = ((unsigned long long)(uint32_t)(x < y ? x : y) << 32) | (uint32_t)(x < y ? y : x);
      const auto it = edgeId.emplace(key, (int)edges.size());
      if (it.second) edges.push_back(Edge{ 0, { false, false } });
      Edge& e = edges[it.first->second];
      if (e.faces < 2) e.dir[e.faces] = x < y;
      e.faces++;
      ids[3 + s] = it.first->second;
    }
  }
  t.signedVolume = vol / 6.0;
  t.nEdges = (int)edges.size();
  for (const Edge& e : edges) {
    if (e.faces == 1) t.boundaryEdges++;
    else if (e.faces > 2) t.nonManifoldEdges++;
    else if (e.dir[0] == e.dir[1]) t.flippedEdges++;
  }
  // the lists: counted, then filled face by face, so that each comes out ascending
  t.vertexStart.assign((size_t)t.nVerts + 1, 0); t.edgeStart.assign((size_t)t.nEdges + 1, 0);
  for (size_t f = 0; f < nFaces; f++) {
    const int* ids = &t.faceIds[6 * f];
    if (ids[0] < 0) continue;
    for (int s = 0; s < 3; s++) { t.vertexStart[(size_t)ids[s] + 1]++; t.edgeStart[(size_t)ids[3 + s] + 1]++; }
  }
  for (int i = 0; i < t.nVerts; i++) t.vertexStart[(size_t)i + 1] += t.vertexStart[i];
  for (int i = 0; i < t.nEdges; i++) t.edgeStart[(size_t)i + 1] += t.edgeStart[i];
  t.vertexCorner.assign((size_t)t.vertexStart[t.nVerts], 0); t.edgeFace.assign((size_t)t.edgeStart[t.nEdges], 0);
  std::vector<int> vfill(t.vertexStart.begin(), t.vertexStart.end() - 1), efill(t.edgeStart.begin(), t.edgeStart.end() - 1);
  for (size_t f = 0; f < nFaces; f++) {
    const int* ids = &t.faceIds[6 * f];
    if (ids[0] < 0) continue;
    for (int s = 0; s < 3; s++) { t.vertexCorner[(size_t)vfill[ids[s]]++] = (int)(3 * f) + s; t.edgeFace[(size_t)efill[ids[3 + s]]++] = (int)f; }
  }
}

}  // namespace pt
