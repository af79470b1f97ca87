// multihitsim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of the multi-hit ray query (minimaloptix_amd/csrc/querykernel.hip pt_rayquery_multi): the
// same per-ray code (pt_multihit.h over pt_path.h's node step), compiled for the host and run one ray at a time, on the scene and tree of a
// hostsim_create handle (hostsim.h) -- and beside it the definition itself: a loop over every primitive record that collects the hit set,
// sorts it by (t, prim) and fills the records, without a tree, a bound or a list.  The GPU tests compare the kernel's output with the
// first bit for bit, the CPU tests the first with the second.  It is not part of the product: nothing under minimaloptix_amd/ builds or loads it.
#include <algorithm>
#include <cstring>
#include <vector>
#include "hostsim.h"
#include "../../minimaloptix_amd/csrc/pt_multihit.h"

using namespace hostsim;

namespace {

bool bad_args(void* h, const float* rays, int64_t n, int maxHits, uint32_t flags, void* hits, int32_t* counts) {
  if (!h || n < 0 || (flags & ~(uint32_t)MULTI_COUNT_ALL) != 0) return true;
  if (maxHits < ((flags & MULTI_COUNT_ALL) ? 0 : 1) || maxHits > kMultiMaxHits) return true;
  return n > 0 && (!rays || !counts || (maxHits > 0 && !hits));
}

template <bool ALL, bool N64>
void multi_one(const SceneView& sc, const float* r, int maxHits, Word4* slice, int32_t* count) {
  LocalStack st;
  Counters ct; memset(&ct, 0, sizeof(ct));
  PathState ps; memset(&ps, 0, sizeof(ps));
  Trav tv; memset(&tv, 0, sizeof(tv));
  HitList hl;
  const bool valid = query_ray(r, ps);
  hl.init(slice, maxHits);
  multi_begin<ALL>(sc, ps, valid, tv, hl);
  while (tv.node != kTravDone) multi_step<ALL, N64>(sc, ps, tv, st, hl, ct);
  multi_finish(sc, ps, hl);
  *count = ALL ? hl.total : hl.count;
}

struct BruteHit { float t; int prim, tri; float beta, gamma; };

void brute_one(const SceneView& sc, const float* r, int maxHits, bool all, QueryHit* out, int32_t* count) {
  PathState ps; memset(&ps, 0, sizeof(ps));
  std::vector<BruteHit> H;
  if (query_ray(r, ps)) {
    for (int i = 0; i < sc.nSpheres; i++) {
      float t1, t2;
      if (!sphere_roots(sc.spheres[i].center, sc.spheres[i].radius, ps.o, ps.d, t1, t2)) continue;
      if (t1 > ps.tmin && t1 < ps.tmax) H.push_back({ t1, i, -1, 0.f, 0.f });
      if (t2 > ps.tmin && t2 < ps.tmax && t2 != t1) H.push_back({ t2, i, -1, 0.f, 0.f });
    }
    for (int i = 0; i < sc.nQuads; i++) {
      const DevQuad& q = sc.quads[i];
      float t;
      if (quad_test(q.plane, q.v1, q.v2, q.anchor, ps.o, ps.d, ps.tmin, ps.tmax, t)) H.push_back({ t, sc.nSpheres + i, -1, 0.f, 0.f });
    }
    for (int k = 0; k < sc.nTris; k++) {
      const Tri48& tp = sc.tris[k];
      v3 n; float t, be, ga;
      if (tri_test(ps.o, ps.d, ps.tmin, ps.tmax, tp.p0, tp.e0, tp.e1, n, t, be, ga)) H.push_back({ t, sc.nSpheres + sc.nQuads + tp.prim, k, be, ga });
    }
    std::sort(H.begin(), H.end(), [](const BruteHit& a, const BruteHit& b) { return a.t < b.t || (a.t == b.t && a.prim < b.prim); });
  }
  const int c = (int)std::min<size_t>(H.size(), (size_t)maxHits);
  for (int j = 0; j < maxHits; j++) {
    Trav tv; memset(&tv, 0, sizeof(tv));
    query_miss(ps, tv);
    if (j < c) { tv.tbest = H[j].t; tv.bestPrim = H[j].prim; tv.bestTri = H[j].tri; tv.beta = H[j].beta; tv.gamma = H[j].gamma; }
    query_hit(sc, ps, tv, out[j]);
  }
  *count = all ? (int32_t)H.size() : c;
}

}  // namespace

extern "C" {

// moptix_query_rays_multi on the CPU.  rays: n x 8 floats; hits: n x maxHits 32-byte hit records, 16-byte aligned (may be null with
// maxHits 0); counts: n x int32.
int multihitsim_query(void* h, int nodeFormat, const float* rays, int64_t n, int maxHits, uint32_t flags, void* hits, int32_t* counts) {
  if (bad_args(h, rays, n, maxHits, flags, hits, counts) || (reinterpret_cast<uintptr_t>(hits) & 15u) != 0) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat), all = (flags & MULTI_COUNT_ALL) != 0;
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; i++) {
    const float* r = rays + 8 * (size_t)i;
    Word4* slice = static_cast<Word4*>(hits) + 2 * (size_t)i * (size_t)maxHits;
    if (all) { if (n64) multi_one<true, true>(sc, r, maxHits, slice, counts + i); else multi_one<true, false>(sc, r, maxHits, slice, counts + i); }
    else { if (n64) multi_one<false, true>(sc, r, maxHits, slice, counts + i); else multi_one<false, false>(sc, r, maxHits, slice, counts + i); }
  }
  return 0;
}

// The same answer from the definition: every primitive record, no tree.
int multihitsim_brute(void* h, const float* rays, int64_t n, int maxHits, uint32_t flags, void* hits, int32_t* counts) {
  if (bad_args(h, rays, n, maxHits, flags, hits, counts)) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool all = (flags & MULTI_COUNT_ALL) != 0;
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t i = 0; i < n; i++)
    brute_one(sc, rays + 8 * (size_t)i, maxHits, all, static_cast<QueryHit*>(hits) + (size_t)i * (size_t)maxHits, counts + i);
  return 0;
}

}  // extern "C"
