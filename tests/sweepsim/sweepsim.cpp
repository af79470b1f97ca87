// sweepsim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of the sphere sweep queries (minimaloptix_amd/csrc/sweepkernel.hip pt_sweepquery):
// the same per-sweep code (pt_sweep.h), compiled for the host and run one sweep at a time, on the scene and tree of a hostsim_create
// handle (tests/hostsim/hostsim.h) -- and beside it the definition itself: a loop over every primitive record through its time of
// contact, without a tree.  The GPU tests compare the kernel's output with the first bit for bit, the CPU tests the first with the
// second.  The per-primitive functions are also exported on explicit inputs, for references that share no code with them.
// A library of its own, libsweepsim.so, built with libhostsim.so's flags: it reads the handle's built scene through hostsim.h and calls
// nothing of that library.  It is not part of the product: nothing under minimaloptix_amd/ builds or loads it.
#include "../hostsim/hostsim.h"
#include "../../minimaloptix_amd/csrc/pt_sweep.h"

using namespace hostsim;

namespace {

void write_result(const SceneView& sc, int mode, const SweepQ& q, const SweepTrav& tv, void* out, size_t i) {
  if (mode == SWEEP_ANY) static_cast<int32_t*>(out)[i] = tv.bestPrim >= 0 ? 1 : 0;
  else sweep_hit(sc, q, tv, static_cast<SweepHit*>(out)[i]);
}

// deepest: the most stack entries the walk held, where asked for
template <bool ANY, bool N64>
void walk_one(const SceneView& sc, const float* s, void* out, size_t i, int* deepest) {
  LocalPointStack st;
  SweepQ q;
  sweep_query(s, q);
  SweepTrav tv;
  sweep_begin<ANY>(sc, q, sweep_valid(s), tv);
  while (tv.node != kTravDone) {
    sweep_step<ANY, N64>(sc, q, tv, st);
    if (deepest && tv.sp > *deepest) *deepest = tv.sp;
  }
  if (out) write_result(sc, ANY ? SWEEP_ANY : SWEEP_CLOSEST, q, tv, out, i);
}

void walk_any(const SceneView& sc, int mode, bool n64, const float* s, void* out, size_t i, int* deepest = nullptr) {
  if (mode == SWEEP_ANY) { if (n64) walk_one<true, true>(sc, s, out, i, deepest); else walk_one<true, false>(sc, s, out, i, deepest); }
  else { if (n64) walk_one<false, true>(sc, s, out, i, deepest); else walk_one<false, false>(sc, s, out, i, deepest); }
}

// the definition: every primitive record, no tree.  "any" is "closest reports a primitive".
void brute_one(const SceneView& sc, int mode, const float* s, void* out, size_t i) {
  SweepQ q;
  sweep_query(s, q);
  SweepTrav tv;
  tv.tbest = q.tmax; tv.bestPrim = -1; tv.bestTri = -1; tv.sp = 0; tv.node = kTravDone;
  if (sweep_valid(s)) {
    float t;
    for (int k = 0; k < sc.nSpheres; k++)
      if (sweep_sphere(q, sc.spheres[k].center, sc.spheres[k].radius, t) && sweep_accept(t, k, tv.tbest, tv.bestPrim)) { tv.bestPrim = k; tv.tbest = t; }
    for (int k = 0; k < sc.nQuads; k++)
      if (sweep_quad(q, sc.quads[k].v1, sc.quads[k].v2, sc.quads[k].anchor, t) && sweep_accept(t, sc.nSpheres + k, tv.tbest, tv.bestPrim)) {
        tv.bestPrim = sc.nSpheres + k; tv.tbest = t;
      }
    const int triBase = sc.nSpheres + sc.nQuads;
    for (int k = 0; k < sc.nTris; k++) {
      const Tri48& r = sc.tris[k];
      if (sweep_tri(q, r.p0, r.e0, r.e1, t) && sweep_accept(t, triBase + r.prim, tv.tbest, tv.bestPrim)) { tv.bestPrim = triBase + r.prim; tv.bestTri = k; tv.tbest = t; }
    }
  }
  write_result(sc, mode, q, tv, out, i);
}

bool bad_mode(int mode) { return mode != SWEEP_CLOSEST && mode != SWEEP_ANY; }

// The record of a one-primitive answer: t and the closest-point function at the centre of contact; prim 0, or the miss record.
void one_prim_record(const SweepQ& q, bool hit, float t, int kind, const float* g, SweepHit& h) {
  h.t = q.tmax; h.prim = -1; h.mat = -1; h.u = 0.f; h.v = 0.f; h.p[0] = 0.f; h.p[1] = 0.f; h.p[2] = 0.f;
  if (!hit) return;
  const v3 c = sweep_centre(q, t);
  PointCand k;
  if (kind == 0) point_tri(c, mk3(g[0], g[1], g[2]), mk3(g[3], g[4], g[5]), mk3(g[6], g[7], g[8]), k);
  else if (kind == 1) point_sphere(c, mk3(g[0], g[1], g[2]), g[3], k);
  else point_quad(c, mk3(g[0], g[1], g[2]), mk3(g[3], g[4], g[5]), mk3(g[6], g[7], g[8]), k);
  h.t = t; h.prim = 0; h.mat = 0; h.u = k.u; h.v = k.v; h.p[0] = k.c.x; h.p[1] = k.c.y; h.p[2] = k.c.z;
}

}  // namespace

extern "C" {

// moptix_query_sweeps on the CPU.  sweeps: n x 8 floats; mode 0 = closest (out: n x SweepHit), 1 = any (out: n x int32).
int sweepsim_query(void* h, int nodeFormat, const float* sweeps, int64_t n, int mode, void* out) {
  if (!h || n < 0 || bad_mode(mode) || (n > 0 && (!sweeps || !out))) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat);
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; i++) walk_any(sc, mode, n64, sweeps + 8 * (size_t)i, out, (size_t)i);
  return 0;
}

// The same answers from the definition: every primitive record, no tree.
int sweepsim_brute(void* h, const float* sweeps, int64_t n, int mode, void* out) {
  if (!h || n < 0 || bad_mode(mode) || (n > 0 && (!sweeps || !out))) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
#pragma omp parallel for schedule(dynamic, 4)
  for (int64_t i = 0; i < n; i++) brute_one(sc, mode, sweeps + 8 * (size_t)i, out, (size_t)i);
  return 0;
}

// Most stack entries the walk of any of the sweeps holds in this mode: what the kernel's LDS part and overflow column have to hold.
int sweepsim_stack_depth(void* h, int nodeFormat, const float* sweeps, int64_t n, int mode) {
  if (!h || n < 0 || bad_mode(mode) || (n > 0 && !sweeps)) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat);
  int deepest = 0;
  for (int64_t i = 0; i < n; i++) walk_any(sc, mode, n64, sweeps + 8 * (size_t)i, nullptr, 0, &deepest);
  return deepest;
}

// The per-primitive time of contact on explicit inputs, pair by pair: sweeps n x 8, out n x SweepHit with prim 0 where there is a
// contact in [0, tmax] (an invalid sweep has none).  kind 0: triangles, n x 9 floats, the record's p0, e0, e1; 1: spheres, n x 4, centre
// and radius; 2: quads, n x 9, the record's v1, v2 (the inverted edges) and anchor.
int sweepsim_toi(int kind, const float* prims, const float* sweeps, int64_t n, void* out) {
  if (kind < 0 || kind > 2 || n < 0 || (n > 0 && (!prims || !sweeps || !out))) return -1;
  const int w = kind == 1 ? 4 : 9;
  for (int64_t i = 0; i < n; i++) {
    const float* g = prims + w * (size_t)i;
    const float* s = sweeps + 8 * (size_t)i;
    SweepQ q;
    sweep_query(s, q);
    float t = 0.0f;
    bool hit = false;
    if (sweep_valid(s)) {
      if (kind == 0) hit = sweep_tri(q, mk3(g[0], g[1], g[2]), mk3(g[3], g[4], g[5]), mk3(g[6], g[7], g[8]), t);
      else if (kind == 1) hit = sweep_sphere(q, mk3(g[0], g[1], g[2]), g[3], t);
      else hit = sweep_quad(q, mk3(g[0], g[1], g[2]), mk3(g[3], g[4], g[5]), mk3(g[6], g[7], g[8]), t);
    }
    one_prim_record(q, hit, t, kind, g, static_cast<SweepHit*>(out)[i]);
  }
  return 0;
}

}  // extern "C"
