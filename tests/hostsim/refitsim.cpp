// refitsim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of the mesh refit (minimaloptix_amd/csrc/refitkernel.hip): the same per-triangle and
// per-node code (pt_refit.h), compiled for the host and run one element at a time on the scene and tree of a hostsim_create handle
// (hostsim.h), which stays a handle like any other: hostsim_render, aovsim_render_aovs and querysim_query run on the refitted tree.
// The GPU tests compare the refitted device arrays with this byte for byte.  It is not part of the product: nothing under
// minimaloptix_amd/ builds or loads it.
#include <cstring>
#include "hostsim.h"

using namespace hostsim;

namespace {

double tree_cost(const HostBVH& b) {
  if (b.nodes.empty()) return 0.0;
  double s = 0.0;
  for (const Node128& n : b.nodes) s += refit_node_cost(n);
  const double a = refit_root_area(b.nodes[0]);
  return a > 0.0 ? s / a : 0.0;
}

void point_view(HostSim& r) {
  HostBVH& b = r.hs.bvh;
  r.hs.view.nodes = b.nodes.data(); r.hs.view.nodes64 = b.nodes64.empty() ? nullptr : b.nodes64.data();
  r.hs.view.tris = b.tris.data(); r.hs.view.triShade = b.shade.data();
}

}  // namespace

extern "C" {

struct refitsim_out {      // caller-allocated, any pointer may be NULL: nodes nNodes*128 B, nodes64 nNodes*64 B, tris / shade nFaces*48 B
  void* nodes; void* nodes64; void* tris; void* shade;
  int32_t nNodes, rootRef, has64;
  double sahCost, sahCostBuilt;
};

// moptix_update_faces
int refitsim_update(void* h, int32_t first, int32_t n, const float* pos9, const float* nrm9) {
  HostSim* r = static_cast<HostSim*>(h);
  if (!r || first < 0 || n < 0 || (size_t)first + (size_t)n > r->faceHasNrm.size() || (n > 0 && !pos9)) return -1;
  memcpy(r->facePos.data() + 9 * (size_t)first, pos9, sizeof(float) * 9 * (size_t)n);
  if (nrm9)
    for (int32_t f = 0; f < n; f++)
      if (r->faceHasNrm[first + f]) memcpy(&r->faceNrm[9 * (size_t)(first + f)], nrm9 + 9 * (size_t)f, 9 * sizeof(float));
  return 0;
}

// moptix_refit_accel
int refitsim_refit(void* h) {
  HostSim* r = static_cast<HostSim*>(h);
  HostBVH& b = r->hs.bvh;
  const int n = (int)b.tris.size(), nNodes = (int)b.nodes.size();
  if (n == 0) return 0;
  if (!r->planned) {
    if (!refit_plan_levels(b.nodes.data(), nNodes, r->order, r->levelFirst)) return -1;
    r->sahCostBuilt = tree_cost(b); r->sahCost = r->sahCostBuilt;
    r->raw.resize(n);
    r->planned = true;
  }
  v3 slo = mk3(1e37f, 1e37f, 1e37f), shi = mk3(-1e37f, -1e37f, -1e37f);
  for (int k = 0; k < n; k++) {
    const Tri48 old = b.tris[k];
    const int f = old.prim;
    refit_triangle(&r->facePos[9 * (size_t)f], &r->faceNrm[9 * (size_t)f], r->faceHasNrm[f] != 0, old, b.tris[k], b.shade[k], r->raw[k]);
    const RefitBox& x = r->raw[k];
    slo = mk3(fminf_(slo.x, x.lox), fminf_(slo.y, x.loy), fminf_(slo.z, x.loz));
    shi = mk3(fmaxf_(shi.x, x.hix), fmaxf_(shi.y, x.hiy), fmaxf_(shi.z, x.hiz));
  }
  const float padAbs = refit_pad_abs(slo, shi);
  bool ok64 = !b.nodes64.empty();
  for (size_t L = r->levelFirst.size(); L-- > 1;)
    for (int i = r->levelFirst[L - 1]; i < r->levelFirst[L]; i++) {
      const int nd = r->order[i];
      refit_node(b.nodes[nd], r->raw.data(), padAbs, b.nodes.data());
      if (!b.nodes64.empty() && !compress_node(b.nodes[nd], b.nodes64[nd])) ok64 = false;
    }
  if (!ok64) b.nodes64.clear();
  point_view(*r);
  if (nNodes > 0) r->sahCost = tree_cost(b);
  return 0;
}

int refitsim_read(void* h, refitsim_out* out) {
  HostSim* r = static_cast<HostSim*>(h);
  const HostBVH& b = r->hs.bvh;
  out->nNodes = (int)b.nodes.size(); out->rootRef = b.rootRef; out->has64 = !b.nodes.empty() && !b.nodes64.empty() ? 1 : 0;
  out->sahCost = r->planned ? r->sahCost : tree_cost(b); out->sahCostBuilt = r->planned ? r->sahCostBuilt : tree_cost(b);
  if (out->nodes && !b.nodes.empty()) memcpy(out->nodes, b.nodes.data(), b.nodes.size() * sizeof(Node128));
  if (out->nodes64 && !b.nodes64.empty()) memcpy(out->nodes64, b.nodes64.data(), b.nodes64.size() * sizeof(Node64));
  if (out->tris && !b.tris.empty()) memcpy(out->tris, b.tris.data(), b.tris.size() * sizeof(Tri48));
  if (out->shade && !b.shade.empty()) memcpy(out->shade, b.shade.data(), b.shade.size() * sizeof(TriShade));
  return 0;
}

}  // extern "C"
