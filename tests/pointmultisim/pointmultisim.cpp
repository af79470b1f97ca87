// pointmultisim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of the K-nearest point query (minimaloptix_amd/csrc/pointkernel.hip
// pt_pointquery_multi): the same per-point code (pt_pointmulti.h over pt_point.h's node step), compiled for the host and run one point at a
// time, on the scene and tree of a hostsim_create handle (tests/hostsim/hostsim.h) -- and beside it the definition itself: a loop over every
// primitive record that collects the near set, orders it by (d2, prim) and fills the records, without a tree, a bound or a list.  The GPU
// tests compare the kernel's output with the first bit for bit, the CPU tests the first with the second.  A library of its own,
// libpointmultisim.so, built with libhostsim.so's flags: it reads the handle's built scene through hostsim.h and calls nothing of that
// library.  It is not part of the product: nothing under minimaloptix_amd/ builds or loads it.
#include <algorithm>
#include <cstring>
#include <vector>
#include "../hostsim/hostsim.h"
#include "../../minimaloptix_amd/csrc/pt_pointmulti.h"

using namespace hostsim;

namespace {

bool bad_args(void* h, const float* points, int64_t n, int maxNear, uint32_t flags, void* hits, int32_t* counts) {
  if (!h || n < 0 || (flags & ~(uint32_t)POINT_MULTI_COUNT_ALL) != 0) return true;
  if (maxNear < ((flags & POINT_MULTI_COUNT_ALL) ? 0 : 1) || maxNear > kPointMultiMaxNear) return true;
  return n > 0 && (!points || !counts || (maxNear > 0 && !hits));
}

// deepest: the most stack entries the walk held, where asked for.  finish = false: the slice keeps the walk's keys (pointmultisim_keys).
template <bool ALL, bool N64>
void multi_one(const SceneView& sc, const float* p, int maxNear, Word4* slice, int32_t* count, int* deepest = nullptr, bool finish = true) {
  LocalPointStack st;
  PointTrav tv;
  NearList nl;
  const v3 q = mk3(p[0], p[1], p[2]);
  const float r2 = p[3] * p[3];
  nl.init(slice, maxNear);
  pointmulti_begin<ALL>(sc, q, r2, point_valid(p), tv, nl);
  while (tv.node != kTravDone) {
    pointmulti_step<ALL, N64>(sc, q, r2, tv, st, nl);
    if (deepest && tv.sp > *deepest) *deepest = tv.sp;
  }
  if (finish) pointmulti_finish(sc, q, p[3], nl);
  *count = ALL ? nl.total : nl.count;
}

void multi_any(const SceneView& sc, bool all, bool n64, const float* p, int maxNear, Word4* slice, int32_t* count, int* deepest = nullptr,
               bool finish = true) {
  if (all) {
    if (n64) multi_one<true, true>(sc, p, maxNear, slice, count, deepest, finish); else multi_one<true, false>(sc, p, maxNear, slice, count, deepest, finish);
  } else {
    if (n64) multi_one<false, true>(sc, p, maxNear, slice, count, deepest, finish); else multi_one<false, false>(sc, p, maxNear, slice, count, deepest, finish);
  }
}

struct BruteNear { float d2; int prim, tri; };

void brute_one(const SceneView& sc, const float* p, int maxNear, bool all, PointHit* out, int32_t* count) {
  const v3 q = mk3(p[0], p[1], p[2]);
  const float r2 = p[3] * p[3];
  std::vector<BruteNear> S;
  if (point_valid(p)) {
    PointCand k;
    for (int i = 0; i < sc.nSpheres; i++) {
      point_sphere(q, sc.spheres[i].center, sc.spheres[i].radius, k);
      if (k.d2 < r2) S.push_back({ k.d2, i, -1 });
    }
    for (int i = 0; i < sc.nQuads; i++) {
      point_quad(q, sc.quads[i].v1, sc.quads[i].v2, sc.quads[i].anchor, k);
      if (k.d2 < r2) S.push_back({ k.d2, sc.nSpheres + i, -1 });
    }
    for (int t = 0; t < sc.nTris; t++) {
      const Tri48& r = sc.tris[t];
      point_tri(q, r.p0, r.e0, r.e1, k);
      if (k.d2 < r2) S.push_back({ k.d2, sc.nSpheres + sc.nQuads + r.prim, t });
    }
  }
  const int c = (int)std::min<size_t>(S.size(), (size_t)maxNear);
  // the c least of all pairs in front, in order (the library's selection sort of a prefix: with 168,000 pairs per point a full sort is
  // most of the loop's time, and nothing behind the c-th pair is read)
  std::partial_sort(S.begin(), S.begin() + c, S.end(), [](const BruteNear& a, const BruteNear& b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.prim < b.prim); });
  for (int j = 0; j < maxNear; j++) {
    PointTrav tv;
    tv.bestD2 = 0.f; tv.bestPrim = -1; tv.bestTri = -1; tv.sp = 0; tv.node = kTravDone;
    if (j < c) { tv.bestD2 = S[j].d2; tv.bestPrim = S[j].prim; tv.bestTri = S[j].tri; }
    point_hit(sc, q, p[3], tv, out[j]);
  }
  *count = all ? (int32_t)S.size() : c;
}

}  // namespace

extern "C" {

// moptix_query_points_multi on the CPU.  points: n x 4 floats; hits: n x maxNear 32-byte records, 16-byte aligned (may be null with
// maxNear 0); counts: n x int32.
int pointmultisim_query(void* h, int nodeFormat, const float* points, int64_t n, int maxNear, uint32_t flags, void* hits, int32_t* counts) {
  if (bad_args(h, points, n, maxNear, flags, hits, counts) || (reinterpret_cast<uintptr_t>(hits) & 15u) != 0) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat), all = (flags & POINT_MULTI_COUNT_ALL) != 0;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; i++)
    multi_any(sc, all, n64, points + 4 * (size_t)i, maxNear, static_cast<Word4*>(hits) + 2 * (size_t)i * (size_t)maxNear, counts + i);
  return 0;
}

// The same answer from the definition: every primitive record, no tree.
int pointmultisim_brute(void* h, const float* points, int64_t n, int maxNear, uint32_t flags, void* hits, int32_t* counts) {
  if (bad_args(h, points, n, maxNear, flags, hits, counts)) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool all = (flags & POINT_MULTI_COUNT_ALL) != 0;
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t i = 0; i < n; i++)
    brute_one(sc, points + 4 * (size_t)i, maxNear, all, static_cast<PointHit*>(hits) + (size_t)i * (size_t)maxNear, counts + i);
  return 0;
}

// The walk's list as pointmulti_finish finds it: keys: n x maxNear x 4 words (d2 bits, prim, triangle record or -1, 0), the first
// min(maxNear, |S|) of a point written, the rest left as they were.  A record's dist is the square root of its key's d2, and the square
// root sends neighbouring d2 to one dist: the order by (d2, prim) itself can only be read here.
int pointmultisim_keys(void* h, int nodeFormat, const float* points, int64_t n, int maxNear, uint32_t flags, uint32_t* keys, int32_t* counts) {
  if (bad_args(h, points, n, maxNear, flags, keys, counts)) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat), all = (flags & POINT_MULTI_COUNT_ALL) != 0;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; i++) {
    std::vector<Word4> slice((size_t)maxNear + 1);
    multi_any(sc, all, n64, points + 4 * (size_t)i, maxNear, slice.data(), counts + i, nullptr, false);
    const int kept = counts[i] < maxNear ? counts[i] : maxNear;
    for (int j = 0; j < kept; j++) memcpy(keys + 4 * ((size_t)i * (size_t)maxNear + (size_t)j), &slice[j], sizeof(Word4));
  }
  return 0;
}

// Most stack entries any of the points needs at this maxNear and these flags: what the kernel's LDS part and overflow column have to hold.
int pointmultisim_stack_depth(void* h, int nodeFormat, const float* points, int64_t n, int maxNear, uint32_t flags) {
  if (!h || n < 0 || (n > 0 && !points) || (flags & ~(uint32_t)POINT_MULTI_COUNT_ALL) != 0) return -1;
  if (maxNear < ((flags & POINT_MULTI_COUNT_ALL) ? 0 : 1) || maxNear > kPointMultiMaxNear) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat), all = (flags & POINT_MULTI_COUNT_ALL) != 0;
  std::vector<Word4> slice(2 * (size_t)maxNear + 1);
  int deepest = 0;
  for (int64_t i = 0; i < n; i++) {
    int32_t count;
    multi_any(sc, all, n64, points + 4 * (size_t)i, maxNear, slice.data(), &count, &deepest);
  }
  return deepest;
}

}  // extern "C"
