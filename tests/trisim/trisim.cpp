// trisim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of the triangle queries (minimaloptix_amd/csrc/trikernel.hip pt_triquery): the same
// per-query code (pt_tri.h), compiled for the host and run one query at a time, on the scene and tree of a hostsim_create handle
// (tests/hostsim/hostsim.h) -- and beside it the definition itself: a loop over every primitive record through its predicate, without a
// tree, the ids sorted by the library's sort.  The GPU tests compare the kernel's output with the first bit for bit, the CPU tests the
// first with the second.  The three predicates are also exported on explicit inputs, for references that share no code with them.
// A library of its own, libtrisim.so, built with libhostsim.so's flags: it reads the handle's built scene through hostsim.h and calls
// nothing of that library.  It is not part of the product: nothing under minimaloptix_amd/ builds or loads it.
#include <algorithm>
#include <vector>
#include "../hostsim/hostsim.h"
#include "../../minimaloptix_amd/csrc/pt_tri.h"

using namespace hostsim;

namespace {

// deepest: the most stack entries the walk held, where asked for
template <int MODE, bool N64>
int walk_one(const SceneView& sc, const float* f, int* slice, long long cap, int* deepest) {
  LocalStack st;
  const TriQ q = tri_make(f);
  BoxOut o;
  o.slice = slice; o.cap = cap > 0 ? cap : 0; o.count = 0;
  BoxTrav tv;
  tri_begin<MODE>(sc, q, tri_valid(f), tv, o);
  while (tv.node != kTravDone) {
    tri_step<MODE, N64>(sc, q, tv, st, o);
    if (deepest && tv.sp > *deepest) *deepest = tv.sp;
  }
  if (MODE == BOX_LIST) box_list_finish(o);
  return MODE == BOX_ANY ? (o.count > 0 ? 1 : 0) : o.count;
}

int walk_any(const SceneView& sc, int mode, bool n64, const float* f, int* slice, long long cap, int* deepest = nullptr) {
  if (mode == BOX_LIST) return n64 ? walk_one<BOX_LIST, true>(sc, f, slice, cap, deepest) : walk_one<BOX_LIST, false>(sc, f, slice, cap, deepest);
  if (mode == BOX_COUNT) return n64 ? walk_one<BOX_COUNT, true>(sc, f, slice, cap, deepest) : walk_one<BOX_COUNT, false>(sc, f, slice, cap, deepest);
  return n64 ? walk_one<BOX_ANY, true>(sc, f, slice, cap, deepest) : walk_one<BOX_ANY, false>(sc, f, slice, cap, deepest);
}

// S(query) by the definition, ascending
void brute_set(const SceneView& sc, const float* f, std::vector<int>& S) {
  S.clear();
  if (!tri_valid(f)) return;
  const TriQ q = tri_make(f);
  for (int i = 0; i < sc.nSpheres; i++)
    if (tri_sphere(sc.spheres[i].center, sc.spheres[i].radius, q)) S.push_back(i);
  for (int i = 0; i < sc.nQuads; i++)
    if (tri_quad(sc.quads[i].v1, sc.quads[i].v2, sc.quads[i].anchor, q)) S.push_back(sc.nSpheres + i);
  for (int t = 0; t < sc.nTris; t++) {
    const Tri48& r = sc.tris[t];
    if (tri_tri(r.p0, r.e0, r.e1, q)) S.push_back(sc.nSpheres + sc.nQuads + r.prim);
  }
  std::sort(S.begin(), S.end());
}

bool bad_offsets(const int64_t* offsets, int64_t n) {
  if (offsets[0] < 0) return true;
  for (int64_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i]) return true;
  return false;
}

}  // namespace

extern "C" {

// moptix_query_tris on the CPU.  tris: n x 9 floats; mode 0 = any, 1 = count; out: n x int32.
int trisim_query(void* h, int nodeFormat, const float* tris, int64_t n, int mode, int32_t* out) {
  if (!h || n < 0 || (mode != BOX_ANY && mode != BOX_COUNT) || (n > 0 && (!tris || !out))) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat);
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; i++) out[i] = walk_any(sc, mode, n64, tris + 9 * (size_t)i, nullptr, 0);
  return 0;
}

// moptix_query_tris_list on the CPU.  offsets: n + 1 int64, non-decreasing from >= 0; prims: offsets[n] int32; counts: n x int32.
int trisim_list(void* h, int nodeFormat, const float* tris, int64_t n, const int64_t* offsets, int32_t* prims, int32_t* counts) {
  if (!h || n < 0 || (n > 0 && (!tris || !offsets || !prims || !counts))) return -1;
  if (n > 0 && bad_offsets(offsets, n)) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat);
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; i++)
    counts[i] = walk_any(sc, BOX_LIST, n64, tris + 9 * (size_t)i, prims + offsets[i], offsets[i + 1] - offsets[i]);
  return 0;
}

// The same answers from the definition: every primitive record, no tree.
int trisim_brute(void* h, const float* tris, int64_t n, int mode, int32_t* out) {
  if (!h || n < 0 || (mode != BOX_ANY && mode != BOX_COUNT) || (n > 0 && (!tris || !out))) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
#pragma omp parallel for schedule(dynamic, 4)
  for (int64_t i = 0; i < n; i++) {
    std::vector<int> S;
    brute_set(sc, tris + 9 * (size_t)i, S);
    out[i] = mode == BOX_ANY ? (S.empty() ? 0 : 1) : (int32_t)S.size();
  }
  return 0;
}

int trisim_brute_list(void* h, const float* tris, int64_t n, const int64_t* offsets, int32_t* prims, int32_t* counts) {
  if (!h || n < 0 || (n > 0 && (!tris || !offsets || !prims || !counts))) return -1;
  if (n > 0 && bad_offsets(offsets, n)) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
#pragma omp parallel for schedule(dynamic, 4)
  for (int64_t i = 0; i < n; i++) {
    std::vector<int> S;
    brute_set(sc, tris + 9 * (size_t)i, S);
    const int64_t cap = offsets[i + 1] - offsets[i];
    int32_t* slice = prims + offsets[i];
    const bool fits = (int64_t)S.size() <= cap;
    for (int64_t j = 0; j < cap; j++) slice[j] = fits && j < (int64_t)S.size() ? S[(size_t)j] : -1;
    counts[i] = (int32_t)S.size();
  }
  return 0;
}

// Most stack entries the walk of any of the queries holds in this mode: what the kernel's LDS part and overflow column have to hold.
int trisim_stack_depth(void* h, int nodeFormat, const float* tris, int64_t n, int mode) {
  if (!h || n < 0 || (n > 0 && !tris) || (mode != BOX_ANY && mode != BOX_COUNT)) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat);
  int deepest = 0;
  for (int64_t i = 0; i < n; i++) walk_any(sc, mode, n64, tris + 9 * (size_t)i, nullptr, 0, &deepest);
  return deepest;
}

// The three predicates on explicit inputs, pair by pair: queries n x 9, out n x int32.  An invalid query gives 0, as in the queries.
// prims: n x 9 floats, the three vertices as the predicate takes them (no record in between)
int trisim_tri(const float* prims, const float* tris, int64_t n, int32_t* out) {
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < n; i++) {
    const float* t = prims + 9 * (size_t)i;
    const float* f = tris + 9 * (size_t)i;
    out[i] = tri_valid(f) && tri_tri_verts(mk3(t[0], t[1], t[2]), mk3(t[3], t[4], t[5]), mk3(t[6], t[7], t[8]), tri_make(f)) ? 1 : 0;
  }
  return 0;
}
// spheres: n x 4 floats, centre and radius
int trisim_sphere(const float* spheres, const float* tris, int64_t n, int32_t* out) {
  for (int64_t i = 0; i < n; i++) {
    const float* s = spheres + 4 * (size_t)i;
    const float* f = tris + 9 * (size_t)i;
    out[i] = tri_valid(f) && tri_sphere(mk3(s[0], s[1], s[2]), s[3], tri_make(f)) ? 1 : 0;
  }
  return 0;
}
// quads: n x 9 floats, the record's v1, v2 (the inverted edges) and anchor
int trisim_quad(const float* quads, const float* tris, int64_t n, int32_t* out) {
  for (int64_t i = 0; i < n; i++) {
    const float* g = quads + 9 * (size_t)i;
    const float* f = tris + 9 * (size_t)i;
    out[i] = tri_valid(f) && tri_quad(mk3(g[0], g[1], g[2]), mk3(g[3], g[4], g[5]), mk3(g[6], g[7], g[8]), tri_make(f)) ? 1 : 0;
  }
  return 0;
}

}  // extern "C"
