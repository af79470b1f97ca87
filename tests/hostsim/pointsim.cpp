// pointsim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of the point-query kernel (minimaloptix_amd/csrc/pointkernel.hip): the same
// per-point code (pt_point.h, pt_sign.h), compiled for the host and run one point at a time, on the scene and tree of a hostsim_create
// handle (hostsim.h); and the loop over every primitive that the traversal must equal.  Both take the kernel's three modes; the entries
// of the signed one, which needs a table, are signsim.cpp's.  The GPU tests compare the kernel's output with this bit for bit.  It is not
// part of the product: nothing under minimaloptix_amd/ builds or loads it.
#include <cstring>
#include "hostsim.h"

using namespace hostsim;

namespace {

void write_out(const SceneView& sc, int mode, const SignRecord* table, const float* p, const PointTrav& tv, void* out, size_t i) {
  const v3 q = mk3(p[0], p[1], p[2]);
  if (mode == POINT_ANY) static_cast<int32_t*>(out)[i] = tv.bestPrim >= 0 ? 1 : 0;
  else if (mode == POINT_SIGNED) point_hit_signed(sc, table, q, p[3], tv, static_cast<PointHit*>(out)[i]);
  else point_hit(sc, q, p[3], tv, static_cast<PointHit*>(out)[i]);
}

template <bool ANY, bool N64>
void walk(const SceneView& sc, const float* p, PointTrav& tv) {
  LocalPointStack st;
  const v3 q = mk3(p[0], p[1], p[2]);
  point_begin<ANY>(sc, q, p[3] * p[3], point_valid(p), tv);
  while (tv.node != kTravDone) point_step<ANY, N64>(sc, q, tv, st);
}

bool bad_args(void* h, const float* points, int64_t n, int mode, void* out) {
  return !h || n < 0 || (n > 0 && (!points || !out)) || (mode != POINT_CLOSEST && mode != POINT_ANY);
}

}  // namespace

namespace hostsim {

void point_query_one(const SceneView& sc, int mode, bool n64, const SignRecord* table, const float* p, void* out, size_t i) {
  PointTrav tv;
  if (mode == POINT_ANY) { if (n64) walk<true, true>(sc, p, tv); else walk<true, false>(sc, p, tv); }
  else { if (n64) walk<false, true>(sc, p, tv); else walk<false, false>(sc, p, tv); }
  write_out(sc, mode, table, p, tv, out, i);
}

// No tree: every sphere, quad and triangle record through the per-primitive functions and the (d2, prim) rule.
void point_brute_one(const SceneView& sc, int mode, const SignRecord* table, const float* p, void* out, size_t i) {
  PointTrav tv;
  tv.bestD2 = p[3] * p[3]; tv.bestPrim = -1; tv.bestTri = -1; tv.sp = 0; tv.node = kTravDone;
  if (point_valid(p)) {
    const v3 q = mk3(p[0], p[1], p[2]);
    const bool any = mode == POINT_ANY;      // the bound stays r2: every primitive is asked "d2 < r2" alone
    PointCand k;
    for (int s = 0; s < sc.nSpheres; s++) {
      point_sphere(q, sc.spheres[s].center, sc.spheres[s].radius, k);
      if (point_accept(k.d2, s, tv.bestD2, tv.bestPrim)) { tv.bestPrim = s; if (!any) tv.bestD2 = k.d2; }
    }
    for (int g = 0; g < sc.nQuads; g++) {
      point_quad(q, sc.quads[g].v1, sc.quads[g].v2, sc.quads[g].anchor, k);
      if (point_accept(k.d2, sc.nSpheres + g, tv.bestD2, tv.bestPrim)) { tv.bestPrim = sc.nSpheres + g; if (!any) tv.bestD2 = k.d2; }
    }
    for (int t = 0; t < sc.nTris; t++) {
      const Tri48& r = sc.tris[t];
      point_tri(q, r.p0, r.e0, r.e1, k);
      const int prim = sc.nSpheres + sc.nQuads + r.prim;
      if (point_accept(k.d2, prim, tv.bestD2, tv.bestPrim)) { tv.bestPrim = prim; tv.bestTri = t; if (!any) tv.bestD2 = k.d2; }
    }
  }
  write_out(sc, mode, table, p, tv, out, i);
}

}  // namespace hostsim

extern "C" {

// moptix_query_points on the CPU.  points: n x 4 floats; mode 0 = closest (out: n x 32-byte records), 1 = any (out: n x int32).
int pointsim_query(void* h, int nodeFormat, const float* points, int64_t n, int mode, void* out) {
  if (bad_args(h, points, n, mode, out)) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat);
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; i++) point_query_one(sc, mode, n64, nullptr, points + 4 * (size_t)i, out, (size_t)i);
  return 0;
}

// The same answers from a plain loop over every primitive record of the handle's scene.
int pointsim_brute(void* h, const float* points, int64_t n, int mode, void* out) {
  if (bad_args(h, points, n, mode, out)) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t i = 0; i < n; i++) point_brute_one(sc, mode, nullptr, points + 4 * (size_t)i, out, (size_t)i);
  return 0;
}

// Most stack entries any of the points needs (closest mode): what the kernel's LDS part and overflow column have to hold.
int pointsim_stack_depth(void* h, int nodeFormat, const float* points, int64_t n) {
  if (!h || n < 0 || (n > 0 && !points)) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat);
  int deepest = 0;
  for (int64_t i = 0; i < n; i++) {
    const float* p = points + 4 * (size_t)i;
    LocalPointStack st;
    PointTrav tv;
    const v3 q = mk3(p[0], p[1], p[2]);
    point_begin<false>(sc, q, p[3] * p[3], point_valid(p), tv);
    while (tv.node != kTravDone) {
      if (n64) point_step<false, true>(sc, q, tv, st); else point_step<false, false>(sc, q, tv, st);
      if (tv.sp > deepest) deepest = tv.sp;
    }
  }
  return deepest;
}

}  // extern "C"
