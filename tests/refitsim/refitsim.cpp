// refitsim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of the mesh refit (minimaloptix_amd/csrc/refitkernel.hip): the same per-triangle and
// per-node code (pt_refit.h), compiled for the host and run one element at a time on the scene and tree that tests/hostsim builds (its
// source is included unchanged).  The GPU tests compare the refitted device arrays with this byte for byte.  It is not part of the
// product: nothing under minimaloptix_amd/ builds or loads it.
#include "../hostsim/hostsim.cpp"
#include "../../minimaloptix_amd/csrc/pt_query.h"
#include "../../minimaloptix_amd/csrc/pt_refit.h"

namespace {

struct RefitSim {
  HostScene hs;
  std::vector<float> facePos, faceNrm; std::vector<int> faceHasNrm;      // the staging, as the context keeps it
  std::vector<RefitBox> raw;
  std::vector<int> order, levelFirst;
  bool planned = false, had64 = false;
  double sahCost = 0.0, sahCostBuilt = 0.0;
};

double tree_cost(const HostBVH& b) {
  if (b.nodes.empty()) return 0.0;
  double s = 0.0;
  for (const Node128& n : b.nodes) s += refit_node_cost(n);
  const double a = refit_root_area(b.nodes[0]);
  return a > 0.0 ? s / a : 0.0;
}

void point_view(RefitSim& r) {
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

// the scene as built (hostsim's builder, hostsim_set_builder applies); the scene's arrays are copied
void* refitsim_create(const hostsim_scene* s, int leafSize) {
  RefitSim* r = new RefitSim();
  make_scene(*s, leafSize, r->hs);
  const size_t n = (size_t)(s->nFaces > 0 ? s->nFaces : 0);
  r->facePos.assign(s->facePos, s->facePos + 9 * n);
  r->faceNrm.assign(9 * n, 0.f); r->faceHasNrm.assign(n, 0);
  for (size_t f = 0; f < n; f++)
    if (s->faceNrm && s->faceHasNrm && s->faceHasNrm[f]) { r->faceHasNrm[f] = 1; memcpy(&r->faceNrm[9 * f], s->faceNrm + 9 * f, 9 * sizeof(float)); }
  r->had64 = !r->hs.bvh.nodes64.empty();
  return r;
}
void refitsim_free(void* h) { delete static_cast<RefitSim*>(h); }

// moptix_update_faces
int refitsim_update(void* h, int32_t first, int32_t n, const float* pos9, const float* nrm9) {
  RefitSim* r = static_cast<RefitSim*>(h);
  if (!r || first < 0 || n < 0 || (size_t)first + (size_t)n > r->faceHasNrm.size() || (n > 0 && !pos9)) return -1;
  memcpy(r->facePos.data() + 9 * (size_t)first, pos9, sizeof(float) * 9 * (size_t)n);
  if (nrm9)
    for (int32_t f = 0; f < n; f++)
      if (r->faceHasNrm[first + f]) memcpy(&r->faceNrm[9 * (size_t)(first + f)], nrm9 + 9 * (size_t)f, 9 * sizeof(float));
  return 0;
}

// moptix_refit_accel
int refitsim_refit(void* h) {
  RefitSim* r = static_cast<RefitSim*>(h);
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
  RefitSim* r = static_cast<RefitSim*>(h);
  const HostBVH& b = r->hs.bvh;
  out->nNodes = (int)b.nodes.size(); out->rootRef = b.rootRef; out->has64 = !b.nodes.empty() && !b.nodes64.empty() ? 1 : 0;
  out->sahCost = r->planned ? r->sahCost : tree_cost(b); out->sahCostBuilt = r->planned ? r->sahCostBuilt : tree_cost(b);
  if (out->nodes && !b.nodes.empty()) memcpy(out->nodes, b.nodes.data(), b.nodes.size() * sizeof(Node128));
  if (out->nodes64 && !b.nodes64.empty()) memcpy(out->nodes64, b.nodes64.data(), b.nodes64.size() * sizeof(Node64));
  if (out->tris && !b.tris.empty()) memcpy(out->tris, b.tris.data(), b.tris.size() * sizeof(Tri48));
  if (out->shade && !b.shade.empty()) memcpy(out->shade, b.shade.data(), b.shade.size() * sizeof(TriShade));
  return 0;
}

// hostsim_render on the tree as it stands.  hostsim_render_timed builds its own scene from a hostsim_scene and cannot be handed a tree, so
// this is its loop for the per-ray state machine (hostsim_set_packet(0), the default), statement for statement; counters as there.
int refitsim_render(void* h, int nodeFormat, const int32_t* seeds, int nSeeds, float* accum, uint64_t counters[9]) {
  RefitSim* r = static_cast<RefitSim*>(h);
  const SceneView& sc = r->hs.view;
  const int saved64 = g_node64;
  g_node64 = nodeFormat == 64;
  uint64_t tot[9] = { 0 };
  const int nPix = sc.width * sc.height;
#pragma omp parallel
  {
    uint64_t loc[9] = { 0 };
#pragma omp for schedule(dynamic, 64)
    for (int pix = 0; pix < nPix; pix++) {
      PathState ps; memset(&ps, 0, sizeof(ps));
      Trav tv; memset(&tv, 0, sizeof(tv));
      Counters ct; memset(&ct, 0, sizeof(ct));
      LocalStack st;
      ps.pixel = pix; ps.item = 0;
      v3 acc = mk3(accum[3 * pix], accum[3 * pix + 1], accum[3 * pix + 2]);
      int sIdx = 0;
      if (nSeeds > 0) begin_sample<true>(sc, ps, seeds[0], ct); else ps.mode = M_DONE;
      while (ps.mode != M_DONE) {
        if (ps.mode == M_NEW_SAMPLE) {
          acc = acc + ps.accum;
          if (++sIdx >= nSeeds) break;
          begin_sample<true>(sc, ps, seeds[sIdx], ct);
        } else if (ps.mode == M_TRACE) {
          trav_begin<true>(sc, ps, tv, ct);
          while (tv.node != kTravDone) host_trav_step(sc, ps, tv, st, ct);
          ps.mode = M_RESULT;
        } else if (ps.mode == M_RESULT) {
          on_result<true>(sc, ps, tv, ct);
        } else if (ps.mode == M_LIGHTS) {
          on_lights<true>(sc, ps, ct);
        }
      }
      ps.accum = acc;
      accum[3 * pix] = ps.accum.x; accum[3 * pix + 1] = ps.accum.y; accum[3 * pix + 2] = ps.accum.z;
      loc[0] += ct.samples; loc[1] += ct.primaryRays; loc[2] += ct.bounceRays; loc[3] += ct.shadowRays;
      loc[4] += ct.nodeFetches; loc[5] += ct.triTests; loc[6] += ct.closestHits; loc[7] += ct.lightLoads; loc[8] += ct.analyticTests;
    }
#pragma omp critical
    for (int i = 0; i < 9; i++) tot[i] += loc[i];
  }
  g_node64 = saved64;
  if (counters) for (int i = 0; i < 9; i++) counters[i] = tot[i];
  return 0;
}

// querysim_query on the tree as it stands (tests/querysim: the same per-ray code)
int refitsim_query(void* h, int nodeFormat, const float* rays, int64_t n, int mode, void* out) {
  RefitSim* r = static_cast<RefitSim*>(h);
  if (!r || n < 0 || (n > 0 && (!rays || !out)) || (mode != QUERY_CLOSEST && mode != QUERY_ANY)) return -1;
  const SceneView& sc = r->hs.view;
  const bool n64 = nodeFormat == 64 && sc.nodes64 != nullptr;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; i++) {
    LocalStack st;
    Counters ct; memset(&ct, 0, sizeof(ct));
    PathState ps; memset(&ps, 0, sizeof(ps));
    Trav tv; memset(&tv, 0, sizeof(tv));
    const bool valid = query_ray(rays + 8 * (size_t)i, ps);
    if (mode == QUERY_ANY) {
      query_begin<true>(sc, ps, valid, tv, ct);
      while (tv.node != kTravDone) { if (n64) query_step<true, true>(sc, ps, tv, st, ct); else query_step<true, false>(sc, ps, tv, st, ct); }
      static_cast<int32_t*>(out)[i] = tv.bestPrim >= 0 ? 1 : 0;
    } else {
      query_begin<false>(sc, ps, valid, tv, ct);
      while (tv.node != kTravDone) { if (n64) query_step<false, true>(sc, ps, tv, st, ct); else query_step<false, false>(sc, ps, tv, st, ct); }
      query_hit(sc, ps, tv, static_cast<QueryHit*>(out)[i]);
    }
  }
  return 0;
}

}  // extern "C"
