// segmentsim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of the segment queries (minimaloptix_amd/csrc/segmentkernel.hip pt_segmentquery):
// the same per-segment code (pt_segment.h), compiled for the host and run one segment at a time, on the scene and tree of a
// hostsim_create handle (tests/hostsim/hostsim.h) -- and beside it the definition itself: a loop over every primitive record through
// its distance function, without a tree.  The GPU tests compare the kernel's output with the first bit for bit, the CPU tests the first
// with the second.  The per-primitive functions are also exported on explicit inputs, for references that share no code with them.
// A library of its own, libsegmentsim.so, built with libhostsim.so's flags: it reads the handle's built scene through hostsim.h and
// calls nothing of that library.  It is not part of the product: nothing under minimaloptix_amd/ builds or loads it.
#include "../hostsim/hostsim.h"
#include "../../minimaloptix_amd/csrc/pt_segment.h"

using namespace hostsim;

namespace {

void write_result(const SceneView& sc, int mode, const SegQ& q, const PointTrav& tv, void* out, size_t i) {
  if (mode == SEGMENT_ANY) static_cast<int32_t*>(out)[i] = tv.bestPrim >= 0 ? 1 : 0;
  else segment_hit(sc, q, tv, static_cast<SegmentHit*>(out)[i]);
}

// deepest: the most stack entries the walk held, where asked for
template <bool ANY, bool N64>
void walk_one(const SceneView& sc, const float* s, void* out, size_t i, int* deepest) {
  LocalPointStack st;
  SegQ q;
  segment_query(s, q);
  PointTrav tv;
  segment_begin<ANY>(sc, q, segment_valid(s), tv);
  while (tv.node != kTravDone) {
    segment_step<ANY, N64>(sc, q, tv, st);
    if (deepest && tv.sp > *deepest) *deepest = tv.sp;
  }
  if (out) write_result(sc, ANY ? SEGMENT_ANY : SEGMENT_CLOSEST, q, tv, out, i);
}

void walk_any(const SceneView& sc, int mode, bool n64, const float* s, void* out, size_t i, int* deepest = nullptr) {
  if (mode == SEGMENT_ANY) { if (n64) walk_one<true, true>(sc, s, out, i, deepest); else walk_one<true, false>(sc, s, out, i, deepest); }
  else { if (n64) walk_one<false, true>(sc, s, out, i, deepest); else walk_one<false, false>(sc, s, out, i, deepest); }
}

// the definition: every primitive record, no tree.  "any" is "closest reports a primitive".
void brute_one(const SceneView& sc, int mode, const float* s, void* out, size_t i) {
  SegQ q;
  segment_query(s, q);
  PointTrav tv;
  tv.bestD2 = q.r2; tv.bestPrim = -1; tv.bestTri = -1; tv.sp = 0; tv.node = kTravDone;
  if (segment_valid(s)) {
    SegCand c;
    for (int k = 0; k < sc.nSpheres; k++) {
      segment_sphere(q, sc.spheres[k].center, sc.spheres[k].radius, c);
      if (point_accept(c.d2, k, tv.bestD2, tv.bestPrim)) { tv.bestPrim = k; tv.bestD2 = c.d2; }
    }
    for (int k = 0; k < sc.nQuads; k++) {
      segment_quad(q, sc.quads[k].v1, sc.quads[k].v2, sc.quads[k].anchor, c);
      if (point_accept(c.d2, sc.nSpheres + k, tv.bestD2, tv.bestPrim)) { tv.bestPrim = sc.nSpheres + k; tv.bestD2 = c.d2; }
    }
    const int triBase = sc.nSpheres + sc.nQuads;
    for (int k = 0; k < sc.nTris; k++) {
      const Tri48& r = sc.tris[k];
      segment_tri(q, r.p0, r.e0, r.e1, c);
      if (point_accept(c.d2, triBase + r.prim, tv.bestD2, tv.bestPrim)) { tv.bestPrim = triBase + r.prim; tv.bestTri = k; tv.bestD2 = c.d2; }
    }
  }
  write_result(sc, mode, q, tv, out, i);
}

bool bad_mode(int mode) { return mode != SEGMENT_CLOSEST && mode != SEGMENT_ANY; }

}  // namespace

extern "C" {

// moptix_query_segments on the CPU.  segments: n x 8 floats; mode 0 = closest (out: n x SegmentHit), 1 = any (out: n x int32).
int segmentsim_query(void* h, int nodeFormat, const float* segments, int64_t n, int mode, void* out) {
  if (!h || n < 0 || bad_mode(mode) || (n > 0 && (!segments || !out))) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat);
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; i++) walk_any(sc, mode, n64, segments + 8 * (size_t)i, out, (size_t)i);
  return 0;
}

// The same answers from the definition: every primitive record, no tree.
int segmentsim_brute(void* h, const float* segments, int64_t n, int mode, void* out) {
  if (!h || n < 0 || bad_mode(mode) || (n > 0 && (!segments || !out))) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
#pragma omp parallel for schedule(dynamic, 4)
  for (int64_t i = 0; i < n; i++) brute_one(sc, mode, segments + 8 * (size_t)i, out, (size_t)i);
  return 0;
}

// Most stack entries the walk of any of the segments holds in this mode: what the kernel's LDS part and overflow column have to hold.
int segmentsim_stack_depth(void* h, int nodeFormat, const float* segments, int64_t n, int mode) {
  if (!h || n < 0 || bad_mode(mode) || (n > 0 && !segments)) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat);
  int deepest = 0;
  for (int64_t i = 0; i < n; i++) walk_any(sc, mode, n64, segments + 8 * (size_t)i, nullptr, 0, &deepest);
  return deepest;
}

// The per-primitive function on explicit inputs, pair by pair: segments n x 8, out n x SegmentHit with prim 0 where d2 < r2 (an invalid
// segment has none).  kind 0: triangles, n x 9 floats, the record's p0, e0, e1; 1: spheres, n x 4, centre and radius; 2: quads, n x 9, the
// record's v1, v2 (the inverted edges) and anchor.
int segmentsim_dist(int kind, const float* prims, const float* segments, int64_t n, void* out) {
  if (kind < 0 || kind > 2 || n < 0 || (n > 0 && (!prims || !segments || !out))) return -1;
  const int w = kind == 1 ? 4 : 9;
  for (int64_t i = 0; i < n; i++) {
    const float* g = prims + w * (size_t)i;
    const float* s = segments + 8 * (size_t)i;
    SegQ q;
    segment_query(s, q);
    SegmentHit& h = static_cast<SegmentHit*>(out)[i];
    h.dist = q.maxDist; h.prim = -1; h.mat = -1; h.s = 0.f; h.p[0] = 0.f; h.p[1] = 0.f; h.p[2] = 0.f; h.feature = 0;
    if (!segment_valid(s)) continue;
    SegCand c;
    if (kind == 0) segment_tri(q, mk3(g[0], g[1], g[2]), mk3(g[3], g[4], g[5]), mk3(g[6], g[7], g[8]), c);
    else if (kind == 1) segment_sphere(q, mk3(g[0], g[1], g[2]), g[3], c);
    else segment_quad(q, mk3(g[0], g[1], g[2]), mk3(g[3], g[4], g[5]), mk3(g[6], g[7], g[8]), c);
    if (!point_accept(c.d2, 0, q.r2, -1)) continue;
    h.dist = __builtin_sqrtf(c.d2); h.prim = 0; h.mat = 0; h.s = c.s; h.p[0] = c.c.x; h.p[1] = c.c.y; h.p[2] = c.c.z; h.feature = c.feature;
  }
  return 0;
}

}  // extern "C"
