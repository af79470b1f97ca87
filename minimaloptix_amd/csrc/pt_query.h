// pt_query.h -- batched ray queries against the built scene: closest hit and occlusion (include/moptix.h "ray queries").
//
// A ray is eight floats  ox oy oz dx dy dz tmin tmax  (moptix_debug_trace's layout); the direction is used as given, t is in units of |d|.
//   closest   the nearest primitive by (t, primitive id) over the interval trav_begin and potential() define -- t in (tmin, tmax), at equal
//             t the lower id (rule D5) -- whatever its material: pt_path.h's radiance traversal, unchanged.  The record (QueryHit, the
//             C ABI's moptix_hit) carries what hit_attributes computes for the closest-hit programs, before any face-forward flip.
//   any       1 iff the closest query on the same ray reports a primitive.  Purely geometric: the shadow classes of RK_SHADOW (which
//             skips primitives without a Disney program) play no part, so the analytic lists and the leaf have their own small steps
//             here, which stop at the first accepted candidate.  The node step is pt_path.h's, with tbest = tmax throughout: a ray
//             that finds nothing walks exactly the boxes the closest query walks, so the two always agree.
//   invalid   a ray with a non-finite component, tmax <= tmin or a zero direction is a miss, decided before traversal.
//   tmin < 0  is walked as tmin = 0: the traversal works on t >= 0 (the node step orders children by the bit patterns of entry distances
//             clamped to tmin, pt_path.h ChildKey, and widens a box's far distance by a factor; moptix_set_params refuses a negative
//             rayEpsilonT for the same reason), so nothing behind the origin is ever reported.
// Used by the query kernel (querykernel.hip) and by its CPU mirror (tests/querysim); nothing of the render path includes it.
#pragma once
#include "pt_path.h"

namespace pt {

enum { QUERY_CLOSEST = 0, QUERY_ANY = 1 };

struct alignas(16) QueryHit { float t; int prim, mat; float u, v; float ng[3]; };
static_assert(sizeof(QueryHit) == 32, "QueryHit is moptix_hit: two 16-byte stores");

PT_HD bool query_finite(float x) { return (f2i(x) & 0x7f800000) != 0x7f800000; }

// r: the ray's eight floats.  Fills the ray in flight of ps; false = an invalid ray (ps.tmax is still the caller's: a miss reports it).
PT_HD bool query_ray(const float r[8], PathState& ps) {
  ps.o = mk3(r[0], r[1], r[2]); ps.d = mk3(r[3], r[4], r[5]);
  ps.tmin = r[6] > 0.0f ? r[6] : 0.0f;        // negative and -0 -> +0: entry distances are clamped to tmin and ordered by their bits
  ps.tmax = r[7]; ps.kind = RK_RADIANCE;
  bool ok = true;
  for (int k = 0; k < 8; k++) ok = ok & query_finite(r[k]);
  ok = ok & (r[7] > r[6]);
  ok = ok & ((r[3] != 0.0f) | (r[4] != 0.0f) | (r[5] != 0.0f));
  return ok;
}

// The traversal state of a ray that is over before it started: a miss.
PT_HD void query_miss(const PathState& ps, Trav& tv) {
  tv.tbest = ps.tmax; tv.bestPrim = -1; tv.bestTri = -1; tv.beta = 0.f; tv.gamma = 0.f;
  tv.sp = 0; tv.started = 1; tv.node = kTravDone;
}

// Occlusion: the brute-force lists in trav_begin's order, then the set-up of the BVH walk; tv.bestPrim >= 0 = occluded.
PT_HD void query_any_begin(const SceneView& sc, const PathState& ps, Trav& tv) {
  tv.tbest = ps.tmax; tv.bestPrim = -1; tv.bestTri = -1; tv.beta = 0.f; tv.gamma = 0.f;
  tv.inv = mk3(slab_inv(ps.d.x), slab_inv(ps.d.y), slab_inv(ps.d.z));
  tv.noi = neg_o_inv(ps.o, tv.inv);
  tv.sp = 0; tv.started = 1;
  bool hit = false;
  for (int i = 0; i < sc.nSpheres && !hit; i++) {
    const DevSphere s = load_uniform(sc.spheres + i);
    float t1, t2;
    if (sphere_roots(s.center, s.radius, ps.o, ps.d, t1, t2))
      hit = potential(t1, i, ps.tmin, ps.tmax, -1) || potential(t2, i, ps.tmin, ps.tmax, -1);
  }
  for (int i = 0; i < sc.nQuads && !hit; i++) {
    const DevQuad q = load_uniform(sc.quads + i);
    float t;
    hit = quad_test(q.plane, q.v1, q.v2, q.anchor, ps.o, ps.d, ps.tmin, ps.tmax, t) && potential(t, sc.nSpheres + i, ps.tmin, ps.tmax, -1);
  }
  if (hit) tv.bestPrim = 0;
  tv.node = (hit || sc.rootRef == kEmptyRef) ? kTravDone : sc.rootRef;
}

// Occlusion: one leaf for a lane with tv.node < 0; the first triangle the ray meets inside (tmin, tmax) ends the ray.
template <class Stack>
PT_HD void query_any_leaf_step(const SceneView& sc, const PathState& ps, Trav& tv, Stack& st) {
  const int count = leaf_count(tv.node);
  bool hit = false;
  for (int base = 0; base < count && !hit; base += 4) {
    LeafChunk ch;
    leaf_fetch4(sc, tv.node, base, ch);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 4; j++) {
      v3 n; float t, be, ga;
      if (base + j < count && tri_test(ps.o, ps.d, ps.tmin, ps.tmax, ch.p0[j], ch.e0[j], ch.e1[j], n, t, be, ga)) hit = true;
    }
  }
  if (hit) { tv.bestPrim = 0; tv.node = kTravDone; }
  else trav_pop(tv, st);
}

// Start of a query: valid = query_ray's verdict.
template <bool ANY>
PT_HD void query_begin(const SceneView& sc, const PathState& ps, bool valid, Trav& tv, Counters& ct) {
  if (!valid) query_miss(ps, tv);
  else if (ANY) query_any_begin(sc, ps, tv);
  else trav_begin<false>(sc, ps, tv, ct);
}

// One traversal step for a lane with tv.node != kTravDone (if-if form, as trav_step).
template <bool ANY, bool N64, class Stack>
PT_HD void query_step(const SceneView& sc, const PathState& ps, Trav& tv, Stack& st, Counters& ct) {
  if (tv.node >= 0) trav_node_step<false, N64>(sc, ps, tv, st, ct);
  else if (ANY) query_any_leaf_step(sc, ps, tv, st);
  else trav_leaf_step<false>(sc, ps, tv, st, ct);
}

// The finished closest query's record.  Normal and material are hit_attributes': what the closest-hit programs start from.
PT_HD void query_hit(const SceneView& sc, const PathState& ps, const Trav& tv, QueryHit& h) {
  h.t = tv.tbest; h.prim = tv.bestPrim; h.mat = -1; h.u = 0.f; h.v = 0.f; h.ng[0] = 0.f; h.ng[1] = 0.f; h.ng[2] = 0.f;
  if (tv.bestPrim < 0) { h.t = ps.tmax; return; }
  HitAttr a;
  hit_attributes(sc, ps, tv, a);
  h.mat = a.mat;
  if (tv.bestPrim >= sc.nSpheres + sc.nQuads) { h.u = tv.beta; h.v = tv.gamma; }
  h.ng[0] = a.geoNormal.x; h.ng[1] = a.geoNormal.y; h.ng[2] = a.geoNormal.z;
}

}  // namespace pt
