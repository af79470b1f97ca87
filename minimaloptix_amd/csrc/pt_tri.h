// pt_tri.h -- triangle overlap queries: the primitives that meet a triangle (include/moptix.h "triangle queries").
//
// A query is nine floats  ax ay az bx by bz cx cy cz, the three vertices a, b, c.  Valid: all nine finite.  An invalid query meets nothing,
// decided before any traversal.  A zero-area query (a segment, a point) is valid.  Triangles are closed sets: touching counts.
// S(query) is the set of primitive ids (spheres, then quads, then triangles by original face id) whose predicate below holds; every
// primitive counts, whatever its material.  S is a function of the nine floats and the device records alone: tree, leaf size, builder,
// node format, grid size and scheduling play no part.
//
// What is computed once per query (tri_make), every operation in order (pt_math.h: AC1 dot = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), AC2
// cross = (fma(a.y, b.z, -(a.z * b.y)), ...), AC4 every other operator one binary32 operation, no contraction):
//   lo / hi = the per-axis min / max of a, b, c by comparisons (box_min / box_max): the query's box, exact
//   q1 = b - a;  q2 = c - a                      the query in the frame at its first vertex; q0 = a - a is +0 by definition
//   e0 = q1;  e1 = q2 - q1;  e2 = -q2            its edges (e0 and e2 are no operations)
//   n1 = cross(e0, e1)                           its normal
//   m_i = cross(n1, e_i), i = 0, 1, 2            the in-plane edge normals
//
// The predicates.  Every rejection is a strict comparison, so a NaN, an equality or a zero axis rejects nothing.
//   triangle (v0, v1, v2)   of the Tri48 record as box_tri sees it: v0 = p0, v1 = p0 + e0, v2 = p0 - e1.
//                      A  step A of box_tri_verts word for word, with the query's box lo / hi as q: tmin / tmax = the per-axis min / max
//                         of v0, v1, v2 by comparisons; reject if tmax < lo or tmin > hi on an axis
//                      B  u_i = v_i - a;  f0 = u1 - u0, f1 = u2 - u1, f2 = u0 - u2;  n2 = cross(f0, f1).  The 23 axes, in this order:
//                            1       n1
//                            2       n2
//                            3..11   cross(e_i, f_j), i = 0, 1, 2 outer, j = 0, 1, 2 inner
//                           12..14   m_i = cross(n1, e_i)
//                           15..17   cross(n1, f_j)
//                           18..20   cross(n2, e_i)
//                           21..23   cross(n2, f_j)
//                         For an axis L:  s0 = +0, s1 = dot(L, q1), s2 = dot(L, q2);  t_i = dot(L, u_i);  smin / smax and tmin / tmax by
//                         comparisons (box_min(box_min(x0, x1), x2), likewise max);  reject if tmin > smax or tmax < smin.
//                         The result is the OR of the 23 rejections, so it does not depend on where an evaluation stops; the code looks
//                         at the two normals, then the nine edge pairs, then the twelve cross-normal axes, and stops after a group that
//                         rejected.
//                      Why 23.  For two triangles of non-zero area in general position the two normals and the nine edge pairs are the
//                      complete list.  For a coplanar pair every edge pair's cross product is parallel to the normal, and the in-plane
//                      edge normals cross(n1, e_i) and cross(n2, f_j) are the complete list of the two-dimensional problem.  A segment or
//                      point against a triangle of non-zero area n: out of the plane the list is n and cross(d, f_j) (edge pairs, d the
//                      segment), in the plane n, cross(n, f_j) and cross(n, d) -- cross(n, e_i) or cross(n, f_j) of the degenerate side.
//                      So the predicate is the geometric answer, up to rounding, whenever at least one of the two triangles has non-zero
//                      area.  Two zero-area triangles (segment against segment, point against segment) have n1 = n2 = 0 and at most the
//                      one axis cross(d1, d2): no finite list decides them.  For such a pair the predicate is still this fixed function
//                      of the floats, but only a superset of the geometric answer: it never misses a pair that meets, and reports some
//                      that do not (two collinear disjoint segments inside each other's box, say).
//   sphere           the surface, as everywhere in the family: point_tri(centre, a, q1, e2) of pt_point.h gives dmin2 = its d2, the squared
//                    distance from the centre to the query triangle (v1 = a + q1, v2 = a - e2 there);  dmax2 = the largest of
//                    point_d2(centre, a), point_d2(centre, b), point_d2(centre, c) by comparisons;  r2 = radius * radius;  overlap iff
//                    dmin2 <= r2 and dmax2 >= r2.  A triangle wholly inside the ball meets nothing.
//   quad             the four corners of box_quad (box_quad_corner on E1 = v1 / dot(v1, v1), E2 = v2 / dot(v2, v2)); the triangles
//                    (c00, c10, c11) and (c00, c11, c01) through the triangle predicate on their three vertices; the quad overlaps if
//                    either does.
//
// The walk is pt_box.h's, unchanged: box_node_step<N64>, box_pop, BoxTrav, BoxOut, box_take, box_list_finish, with the query's box lo / hi
// as the Box6.  One query per lane; a stack entry is one child reference.  Only tri_begin (spheres and quads brute force in point_begin's
// order) and tri_leaf_step are new.  There is no pruning margin.
//
// Why the walk's answer is the loop's over every primitive, with no slack.  It is pt_box.h's argument, because step A is a conjunct of this
// predicate as it is of that one and compares the same floats the node step compares:
//   * A triangle in S passed step A: tmin <= hi and tmax >= lo on every axis, tmin / tmax the exact min / max of the COMPUTED vertices
//     v0, v1, v2, lo / hi the exact min / max of the query's nine floats.
//   * v0 = p0 is the vertex the builder boxed; v1 = fl(p0 + fl(p1 - p0)) and v2 = fl(p0 - fl(p0 - p2)) are two roundings from p1 and p2, each
//     within 1.2e-7 x (|v| + the scene's largest extent) of the boxed vertex per axis.  Every triangle's box is padded per plane by
//     padAbs + 1e-6 |v|, padAbs = 1e-5 x the scene's largest extent + 1e-30 (pt_lbvh.h pad_lo / pad_hi), eight and eighty times that.  So the
//     leaf's box contains the computed vertices: leafLo <= tmin and tmax <= leafHi.
//   * After a refit: the refit rewrites the record and reproduces the padding on the new vertices (pt_refit.h), so the same holds for the
//     moved triangle.
//   * Boxes only grow towards the root (min / max are exact) and into the 64-byte node form, whose planes contain the 128-byte node's.
//   * Hence every ancestor's box, in either node form, has lo_c <= tmin <= hi and hi_c >= tmax >= lo: it passes box_node_step's exact
//     comparisons against lo / hi, the leaf is reached, and the predicate runs on the same record by the same operations as in the loop.
//     A triangle outside S is rejected wherever it is tested.  Equality passes on both sides, so touching is found.
// Not covered: scenes smaller than 1e-30 units (pt_box.h); pairs whose extent l (the largest |component| of q1, q2, u_i) is above 2^30 or
// below 2^-30 -- the projections on the cross-normal axes are of the order l^4 and leave binary32 beyond that: an axis that underflows to
// zero rejects nothing (a superset), one that overflows compares infinities or NaNs.
// Used by the triangle query kernel (trikernel.hip) and by its CPU mirror (tests/trisim/trisim.cpp); nothing else includes it.
#pragma once
#include "pt_box.h"

namespace pt {

#if defined(__HIP_DEVICE_COMPILE__)
#define PT_TRI_UNROLL _Pragma("unroll")
#define PT_TRI_NOUNROLL _Pragma("nounroll")
#else
#define PT_TRI_UNROLL
#define PT_TRI_NOUNROLL
#endif

struct TriQ {
  Box6 box;               // the query's box: exact min / max of a, b, c
  v3 a, b, c;
  v3 q1, q2;              // b - a, c - a
  v3 e1;                  // q2 - q1 (e0 = q1, e2 = -q2)
  v3 n1;                  // cross(e0, e1)
  v3 m[3];                // cross(n1, e_i)
};

// t: the query's nine floats.  false = an invalid query.
PT_HD bool tri_valid(const float t[9]) {
  bool ok = true;
  for (int k = 0; k < 9; k++) ok = ok & point_finite(t[k]);
  return ok;
}

PT_HD TriQ tri_make(const float t[9]) {
  TriQ q;
  q.a = mk3(t[0], t[1], t[2]); q.b = mk3(t[3], t[4], t[5]); q.c = mk3(t[6], t[7], t[8]);
  q.box.lo = mk3(box_min(box_min(q.a.x, q.b.x), q.c.x), box_min(box_min(q.a.y, q.b.y), q.c.y), box_min(box_min(q.a.z, q.b.z), q.c.z));
  q.box.hi = mk3(box_max(box_max(q.a.x, q.b.x), q.c.x), box_max(box_max(q.a.y, q.b.y), q.c.y), box_max(box_max(q.a.z, q.b.z), q.c.z));
  q.q1 = q.b - q.a; q.q2 = q.c - q.a;
  q.e1 = q.q2 - q.q1;
  q.n1 = cross(q.q1, q.e1);
  q.m[0] = cross(q.n1, q.q1); q.m[1] = cross(q.n1, q.e1); q.m[2] = cross(q.n1, -q.q2);
  return q;
}

// One axis of step B: true = L separates the query (0, q1, q2) from (u0, u1, u2).
PT_HD bool tri_axis_separates(v3 L, const TriQ& q, v3 u0, v3 u1, v3 u2) {
  const float s1 = dot(L, q.q1), s2 = dot(L, q.q2);
  const float t0 = dot(L, u0), t1 = dot(L, u1), t2 = dot(L, u2);
  const float smin = box_min(box_min(0.0f, s1), s2), smax = box_max(box_max(0.0f, s1), s2);
  const float tmin = box_min(box_min(t0, t1), t2), tmax = box_max(box_max(t0, t1), t2);
  return (tmin > smax) | (tmax < smin);
}

// The triangle predicate on three vertices.
PT_HD bool tri_tri_verts(v3 v0, v3 v1, v3 v2, const TriQ& q) {
  // A
  const v3 tmin = mk3(box_min(box_min(v0.x, v1.x), v2.x), box_min(box_min(v0.y, v1.y), v2.y), box_min(box_min(v0.z, v1.z), v2.z));
  const v3 tmax = mk3(box_max(box_max(v0.x, v1.x), v2.x), box_max(box_max(v0.y, v1.y), v2.y), box_max(box_max(v0.z, v1.z), v2.z));
  if ((tmax.x < q.box.lo.x) | (tmin.x > q.box.hi.x) | (tmax.y < q.box.lo.y) | (tmin.y > q.box.hi.y) | (tmax.z < q.box.lo.z) | (tmin.z > q.box.hi.z)) return false;
  // B
  const v3 u0 = v0 - q.a, u1 = v1 - q.a, u2 = v2 - q.a;
  const v3 f[3] = { u1 - u0, u2 - u1, u0 - u2 };
  const v3 e[3] = { q.q1, q.e1, -q.q2 };
  const v3 n2 = cross(f[0], f[1]);
  bool sep = tri_axis_separates(q.n1, q, u0, u1, u2);
  sep = sep | tri_axis_separates(n2, q, u0, u1, u2);
  if (sep) return false;
  PT_TRI_UNROLL
  for (int i = 0; i < 3; i++) {
    PT_TRI_UNROLL
    for (int j = 0; j < 3; j++) sep = sep | tri_axis_separates(cross(e[i], f[j]), q, u0, u1, u2);
  }
  if (sep) return false;
  PT_TRI_UNROLL
  for (int i = 0; i < 3; i++) sep = sep | tri_axis_separates(q.m[i], q, u0, u1, u2);
  PT_TRI_UNROLL
  for (int j = 0; j < 3; j++) sep = sep | tri_axis_separates(cross(q.n1, f[j]), q, u0, u1, u2);
  PT_TRI_UNROLL
  for (int i = 0; i < 3; i++) sep = sep | tri_axis_separates(cross(n2, e[i]), q, u0, u1, u2);
  PT_TRI_UNROLL
  for (int j = 0; j < 3; j++) sep = sep | tri_axis_separates(cross(n2, f[j]), q, u0, u1, u2);
  return !sep;
}

// The triangle predicate on a Tri48 record's p0, e0, e1.
PT_HD bool tri_tri(v3 p0, v3 e0, v3 e1, const TriQ& q) { return tri_tri_verts(p0, p0 + e0, p0 - e1, q); }

PT_HD bool tri_sphere(v3 centre, float radius, const TriQ& q) {
  PointCand k;
  point_tri(centre, q.a, q.q1, -q.q2, k);
  const float dmin2 = k.d2;
  const float dmax2 = box_max(box_max(point_d2(centre, q.a), point_d2(centre, q.b)), point_d2(centre, q.c));
  const float r2 = radius * radius;
  return (dmin2 <= r2) & (dmax2 >= r2);
}

PT_HD bool tri_quad(v3 v1, v3 v2, v3 anchor, const TriQ& q) {
  const v3 E1 = v1 / dot(v1, v1), E2 = v2 / dot(v2, v2);
  const v3 c00 = box_quad_corner(anchor, E1, E2, 0.0f, 0.0f), c10 = box_quad_corner(anchor, E1, E2, 1.0f, 0.0f);
  const v3 c11 = box_quad_corner(anchor, E1, E2, 1.0f, 1.0f), c01 = box_quad_corner(anchor, E1, E2, 0.0f, 1.0f);
  bool meets = false;
  // one copy of the triangle function, not two: (c00, c10, c11), then (c00, c11, c01)
  PT_TRI_NOUNROLL
  for (int h = 0; h < 2 && !meets; h++) meets = tri_tri_verts(c00, h == 0 ? c10 : c11, h == 0 ? c11 : c01, q);
  return meets;
}

// The brute-force lists in point_begin's order, then the set-up of the walk.  valid = tri_valid's verdict.
template <int MODE>
PT_HD void tri_begin(const SceneView& sc, const TriQ& q, bool valid, BoxTrav& tv, BoxOut& o) {
  tv.sp = 0; tv.node = kTravDone;
  if (!valid) return;
  bool done = false;
  for (int i = 0; i < sc.nSpheres && !done; i++) {
    const DevSphere s = load_uniform(sc.spheres + i);
    if (tri_sphere(s.center, s.radius, q)) done = box_take<MODE>(o, i);
  }
  for (int i = 0; i < sc.nQuads && !done; i++) {
    const DevQuad g = load_uniform(sc.quads + i);
    if (tri_quad(g.v1, g.v2, g.anchor, q)) done = box_take<MODE>(o, sc.nSpheres + i);
  }
  tv.node = (done || sc.rootRef == kEmptyRef) ? kTravDone : sc.rootRef;
}

// One leaf for a lane with tv.node < 0 (and != kTravDone): the records are fetched as the point walk fetches them.
template <int MODE, class Stack>
PT_HD void tri_leaf_step(const SceneView& sc, const TriQ& q, BoxTrav& tv, Stack& st, BoxOut& o) {
  const int count = leaf_count(tv.node);
  const int triBase = sc.nSpheres + sc.nQuads;
  bool done = false;
  for (int base = 0; base < count && !done; base += 4) {
    LeafChunk ch;
    leaf_fetch4(sc, tv.node, base, ch);
    // One copy of the 23-axis test per leaf step, not four (pt_frustum.h's form): slot 0 is tested and the chunk moved down one slot,
    // every index a constant, so the chunk stays in registers.
    PT_TRI_NOUNROLL
    for (int j = 0; j < 4; j++) {
      if (base + j < count && !done) {
        if (tri_tri(ch.p0[0], ch.e0[0], ch.e1[0], q)) done = box_take<MODE>(o, triBase + ch.prim[0]);
      }
      ch.p0[0] = ch.p0[1]; ch.p0[1] = ch.p0[2]; ch.p0[2] = ch.p0[3];
      ch.e0[0] = ch.e0[1]; ch.e0[1] = ch.e0[2]; ch.e0[2] = ch.e0[3];
      ch.e1[0] = ch.e1[1]; ch.e1[1] = ch.e1[2]; ch.e1[2] = ch.e1[3];
      ch.prim[0] = ch.prim[1]; ch.prim[1] = ch.prim[2]; ch.prim[2] = ch.prim[3];
    }
  }
  if (done) tv.node = kTravDone;
  else box_pop(tv, st);
}

// One traversal step for a lane with tv.node != kTravDone (if-if form, as box_step).
template <int MODE, bool N64, class Stack>
PT_HD void tri_step(const SceneView& sc, const TriQ& q, BoxTrav& tv, Stack& st, BoxOut& o) {
  if (tv.node >= 0) box_node_step<N64>(sc, q.box, tv, st);
  else tri_leaf_step<MODE>(sc, q, tv, st, o);
}

}  // namespace pt
