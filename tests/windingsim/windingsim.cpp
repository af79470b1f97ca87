// windingsim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of the winding-number queries (minimaloptix_amd/csrc/windingkernel.hip pt_windingquery
// and k_winding_level): the same per-element code (pt_winding.h), compiled for the host and run one element at a time, on the scene and
// tree of a hostsim_create handle (tests/hostsim/hostsim.h) as it is now -- after refitsim_refit: the refitted tree -- and beside it the
// definition itself: every primitive in id order through the same binary32 terms into a binary64 sum, without a tree.  The GPU tests
// compare the kernel's output and table with the first bit for bit, the CPU tests the first with the second and both with a binary64
// reference that shares no code with either.  The triangle term is also exported on explicit inputs, and the walk's work per query:
// clusters approximated, triangles evaluated, stack depth reached.
// A library of its own, libwindingsim.so, built with libhostsim.so's flags: it reads the handle's built scene through hostsim.h and calls
// nothing of that library.  It is not part of the product: nothing under minimaloptix_amd/ builds or loads it.
#include <vector>
#include "../hostsim/hostsim.h"
#include "../../minimaloptix_amd/csrc/pt_winding.h"

using namespace hostsim;

namespace {

// The moments of the handle's tree as it is now: the nodes breadth first (pt_refit.h refit_plan_levels), taken back to front, so that a
// node's children are finished before it -- the order of the device's launches, level by level from the deepest.
bool make_table(const HostSim& hsim, std::vector<WindingNode>& table) {
  const HostBVH& b = hsim.hs.bvh;
  const int nNodes = (int)b.nodes.size();
  table.assign((size_t)nNodes, WindingNode());
  std::vector<int> order, levelFirst;
  if (!refit_plan_levels(b.nodes.data(), nNodes, order, levelFirst)) return false;
  for (size_t i = order.size(); i-- > 0;) {
    const int n = order[i];
    table[(size_t)n] = winding_node(b.nodes[(size_t)n], b.nodes.data(), b.tris.data(), table.data());
  }
  return true;
}

float brute_one(const SceneView& sc, const std::vector<int>& recordOfPrim, const float* p) {
  if (!winding_valid(p)) return i2f(0x7fc00000);
  const v3 q = mk3(p[0], p[1], p[2]);
  double acc = 0.0;
  for (int i = 0; i < sc.nSpheres; i++)
    if (winding_sphere(q, sc.spheres[i].center, sc.spheres[i].radius)) acc += kWinding4Pi;
  for (int i = 0; i < sc.nQuads; i++) winding_quad(q, sc.quads[i].v1, sc.quads[i].v2, sc.quads[i].anchor, acc);
  for (size_t f = 0; f < recordOfPrim.size(); f++) {
    if (recordOfPrim[f] < 0) continue;
    const Tri48& r = sc.tris[recordOfPrim[f]];
    acc += (double)winding_tri(q, r.p0, r.e0, r.e1);
  }
  return winding_result(acc);
}

}  // namespace

extern "C" {

// The table: 128 bytes per node into `table` (null: only the count).  Returns the node count, -1 on a bad handle or tree.
int windingsim_table(void* h, void* table) {
  if (!h) return -1;
  std::vector<WindingNode> t;
  if (!make_table(*static_cast<HostSim*>(h), t)) return -1;
  if (table && !t.empty()) memcpy(table, t.data(), sizeof(WindingNode) * t.size());
  return (int)t.size();
}

// moptix_query_winding on the CPU.  points: n x 4 floats x y z beta; out: n x float.
int windingsim_query(void* h, const float* points, int64_t n, float* out) {
  if (!h || n < 0 || (n > 0 && (!points || !out))) return -1;
  const HostSim& hsim = *static_cast<HostSim*>(h);
  const SceneView& sc = hsim.hs.view;
  std::vector<WindingNode> t;
  if (!make_table(hsim, t)) return -1;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; i++) {
    LocalStack st;
    out[i] = winding_query(sc, t.data(), points + 4 * (size_t)i, st);
  }
  return 0;
}

// The definition: every primitive in id order (spheres, quads, triangles by original face id), the same binary32 terms, a binary64
// sum, no tree and no approximation whatever beta says (validity is still the query's).
int windingsim_brute(void* h, const float* points, int64_t n, float* out) {
  if (!h || n < 0 || (n > 0 && (!points || !out))) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  int nFaces = 0;
  for (int t = 0; t < sc.nTris; t++) nFaces = sc.tris[t].prim + 1 > nFaces ? sc.tris[t].prim + 1 : nFaces;
  std::vector<int> recordOfPrim((size_t)nFaces, -1);
  for (int t = 0; t < sc.nTris; t++) recordOfPrim[(size_t)sc.tris[t].prim] = t;
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t i = 0; i < n; i++) out[i] = brute_one(sc, recordOfPrim, points + 4 * (size_t)i);
  return 0;
}

// The walk's work per query: clusters approximated, triangles evaluated, most stack entries held; n x int64 each.
int windingsim_work(void* h, const float* points, int64_t n, int64_t* clusters, int64_t* tris, int64_t* depth) {
  if (!h || n < 0 || (n > 0 && (!points || !clusters || !tris || !depth))) return -1;
  const HostSim& hsim = *static_cast<HostSim*>(h);
  const SceneView& sc = hsim.hs.view;
  std::vector<WindingNode> t;
  if (!make_table(hsim, t)) return -1;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; i++) {
    LocalStack st;
    WindingWork w = { 0, 0 };
    int deepest = 0;
    winding_query(sc, t.data(), points + 4 * (size_t)i, st, &w, &deepest);
    clusters[i] = w.clusters; tris[i] = w.tris; depth[i] = deepest;
  }
  return 0;
}

// The triangle term on explicit inputs, pair by pair: tris n x 9 floats (the three vertices), points n x 3 floats; out: n x float, the
// signed solid angle (not divided by 4 pi).
int windingsim_tri(const float* tris, const float* points, int64_t n, float* out) {
  for (int64_t i = 0; i < n; i++) {
    const float* t = tris + 9 * (size_t)i;
    const float* p = points + 3 * (size_t)i;
    out[i] = winding_tri_verts(mk3(p[0], p[1], p[2]), mk3(t[0], t[1], t[2]), mk3(t[3], t[4], t[5]), mk3(t[6], t[7], t[8]));
  }
  return 0;
}

}  // extern "C"
