// pt_box.h -- box overlap queries: the primitives that meet an axis-aligned box (include/moptix.h "box queries").
//
// A query is six floats  lox loy loz hix hiy hiz.  Valid: all six finite and lo <= hi on every axis (lo == hi allowed: a point, a segment,
// a rectangle).  An invalid box overlaps nothing, decided before any traversal.  Boxes and primitives are closed sets: touching counts.
// S(box) is the set of primitive ids (spheres, then quads, then triangles by original face id) whose predicate below holds; every primitive
// counts, whatever its material.  S is a function of the box and the device records alone: tree, leaf size, builder, node format, grid
// size and scheduling play no part.
//
// The predicates, every operation in order (pt_math.h: AC1 dot, AC2 cross, AC3 v / s = v * (1 / s), AC4 no contraction).
//   triangle (v0, v1, v2)   of the Tri48 record: v0 = p0, v1 = p0 + e0, v2 = p0 - e1, the triangle point_tri sees.  The 13-axis separating
//                    axis test in three steps; any step may reject, every rejection is a strict comparison, so a NaN or an equality
//                    rejects nothing.  A zero-area triangle needs no special case: its zero axes reject nothing.
//                      A  tmin / tmax = the per-axis min / max of v0, v1, v2 by comparisons; reject if tmax < lo or tmin > hi on an axis
//                      B  c = lo * 0.5 + hi * 0.5;  h = hi * 0.5 - lo * 0.5;  u_i = v_i - c;  f0 = u1 - u0, f1 = u2 - u1, f2 = u0 - u2.
//                         For j = 0, 1, 2 (f = f_j), the axes cross(e_x, f), cross(e_y, f), cross(e_z, f) in this order, each as its
//                         two-term expression, p_i over the non-zero terms for i = 0, 1, 2:
//                           e_x:  p_i = u_i.z * f.y - u_i.y * f.z;   r = h.y * |f.z| + h.z * |f.y|
//                           e_y:  p_i = u_i.x * f.z - u_i.z * f.x;   r = h.x * |f.z| + h.z * |f.x|
//                           e_z:  p_i = u_i.y * f.x - u_i.x * f.y;   r = h.x * |f.y| + h.y * |f.x|
//                         (two products, one subtraction / one sum).  Reject if min p > r or max p < -r.
//                      C  n = cross(f0, f1);  d = dot(n, u0);  r = dot(h, |n|);  reject if |d| > r
//   sphere           the surface, as in the point queries: dmin2 = point_box_d2(centre, box);  m = max(|c - lo|, |hi - c|) per axis by a
//                    comparison, dmax2 = dot(m, m);  r2 = radius * radius;  overlap iff dmin2 <= r2 and dmax2 >= r2.  A box wholly
//                    inside the ball meets nothing.
//   quad             the four corners of point_quad's parametrisation, c_ab = (anchor + E1 * a) + E2 * b at a, b in {0, 1} with
//                    E1 = v1 / dot(v1, v1), E2 = v2 / dot(v2, v2); the triangles (c00, c10, c11) and (c00, c11, c01) through the triangle
//                    predicate on their three vertices; the quad overlaps if either does.
//
// The walk.  One box per lane; a stack entry is one child reference; no ordering, no distances.  The node step enters a child iff its box
// and the query box overlap by exact comparisons, lo_c <= hi_q and hi_c >= lo_q on all three axes; empty references are skipped.  Leaves
// are fetched with leaf_fetch4 as the point walk fetches them.  Spheres and quads are tested brute force in front of the walk, in
// point_begin's order.
//
// Why the walk's answer is the loop's over every primitive, with no grazing exception and no slack.
//   * Step A is a conjunct of the triangle predicate: a triangle in S has tmin <= hi_q and tmax >= lo_q on every axis, where tmin / tmax
//     are the exact min / max of the COMPUTED vertices v0, v1, v2.
//   * v0 = p0 is the vertex the builder boxed.  v1 = fl(p0 + fl(p1 - p0)) and v2 = fl(p0 - fl(p0 - p2)) are two roundings from p1 and p2:
//     each within 2^-24 (|p0| + |p_k - p0|) + 2^-24 |v_k| <= 1.2e-7 x (|v| + the scene's largest extent) of the boxed vertex, per axis.
//   * Every triangle's box is padded per plane by padAbs + 1e-6 |v| with padAbs = 1e-5 x the scene's largest extent + 1e-30 (pt_lbvh.h
//     pad_lo / pad_hi), eight and eighty times that error, and the refit reproduces the padding (pt_refit.h).  So the padded box of the
//     boxed vertices contains the computed vertices: leafLo <= tmin and tmax <= leafHi.
//   * Boxes only grow towards the root (min / max are exact) and into the 64-byte form (its planes contain the 128-byte node's).
//   * Hence for a triangle in S every ancestor's box has lo_c <= tmin <= hi_q and hi_c >= tmax >= lo_q: it passes the node step's exact
//     comparisons, the leaf is reached and the predicate evaluated on the same record by the same operations.  A triangle outside S is
//     rejected wherever it is tested.  Equality passes on both sides, so touching is found.
// Not covered, as for the point queries: scenes smaller than 1e-30 units.
// Used by the box kernel (boxkernel.hip) and by its CPU mirror (tests/boxsim/boxsim.cpp); nothing else includes it.
#pragma once
#include "pt_point.h"

namespace pt {

enum { BOX_ANY = 0, BOX_COUNT = 1, BOX_LIST = 2 };      // BOX_LIST is the list entries' mode: not a value of the C ABI's mode argument

struct Box6 { v3 lo, hi; };

// b: the query's six floats.  false = an invalid box.
PT_HD bool box_valid(const float b[6]) {
  bool ok = true;
  for (int k = 0; k < 6; k++) ok = ok & point_finite(b[k]);
  for (int k = 0; k < 3; k++) ok = ok & (b[k] <= b[3 + k]);
  return ok;
}

PT_HD float box_min(float a, float b) { return b < a ? b : a; }
PT_HD float box_max(float a, float b) { return b > a ? b : a; }

// One edge-cross axis of step B: a and b are the two non-zero terms' coordinates of u0, u1, u2 (p_i = a_i * fb - b_i * fa).
PT_HD bool box_axis_separates(float a0, float b0, float a1, float b1, float a2, float b2, float fa, float fb, float ha, float hb) {
  const float p0 = a0 * fb - b0 * fa, p1 = a1 * fb - b1 * fa, p2 = a2 * fb - b2 * fa;
  const float r = ha * __builtin_fabsf(fb) + hb * __builtin_fabsf(fa);
  const float lo = box_min(box_min(p0, p1), p2), hi = box_max(box_max(p0, p1), p2);
  return (lo > r) | (hi < -r);
}

// The triangle predicate on three vertices.
PT_HD bool box_tri_verts(v3 v0, v3 v1, v3 v2, const Box6& q) {
  // A
  const v3 tmin = mk3(box_min(box_min(v0.x, v1.x), v2.x), box_min(box_min(v0.y, v1.y), v2.y), box_min(box_min(v0.z, v1.z), v2.z));
  const v3 tmax = mk3(box_max(box_max(v0.x, v1.x), v2.x), box_max(box_max(v0.y, v1.y), v2.y), box_max(box_max(v0.z, v1.z), v2.z));
  if ((tmax.x < q.lo.x) | (tmin.x > q.hi.x) | (tmax.y < q.lo.y) | (tmin.y > q.hi.y) | (tmax.z < q.lo.z) | (tmin.z > q.hi.z)) return false;
  // B
  const v3 c = q.lo * 0.5f + q.hi * 0.5f, h = q.hi * 0.5f - q.lo * 0.5f;
  const v3 u0 = v0 - c, u1 = v1 - c, u2 = v2 - c;
  const v3 f[3] = { u1 - u0, u2 - u1, u0 - u2 };
  bool sep = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 3; j++) {
    sep = sep | box_axis_separates(u0.z, u0.y, u1.z, u1.y, u2.z, u2.y, f[j].z, f[j].y, h.z, h.y);      // e_x: p = u.z f.y - u.y f.z
    sep = sep | box_axis_separates(u0.x, u0.z, u1.x, u1.z, u2.x, u2.z, f[j].x, f[j].z, h.x, h.z);      // e_y: p = u.x f.z - u.z f.x
    sep = sep | box_axis_separates(u0.y, u0.x, u1.y, u1.x, u2.y, u2.x, f[j].y, f[j].x, h.y, h.x);      // e_z: p = u.y f.x - u.x f.y
  }
  if (sep) return false;
  // C
  const v3 n = cross(f[0], f[1]);
  const float d = dot(n, u0);
  const float r = dot(h, mk3(__builtin_fabsf(n.x), __builtin_fabsf(n.y), __builtin_fabsf(n.z)));
  return !(__builtin_fabsf(d) > r);
}

// The triangle predicate on a Tri48 record's p0, e0, e1.
PT_HD bool box_tri(v3 p0, v3 e0, v3 e1, const Box6& q) { return box_tri_verts(p0, p0 + e0, p0 - e1, q); }

PT_HD bool box_sphere(v3 centre, float radius, const Box6& q) {
  const float dmin2 = point_box_d2(centre, q.lo.x, q.lo.y, q.lo.z, q.hi.x, q.hi.y, q.hi.z);
  const v3 a = centre - q.lo, b = q.hi - centre;
  const v3 m = mk3(box_max(__builtin_fabsf(a.x), __builtin_fabsf(b.x)), box_max(__builtin_fabsf(a.y), __builtin_fabsf(b.y)),
                   box_max(__builtin_fabsf(a.z), __builtin_fabsf(b.z)));
  const float dmax2 = dot(m, m);
  const float r2 = radius * radius;
  return (dmin2 <= r2) & (dmax2 >= r2);
}

PT_HD v3 box_quad_corner(v3 anchor, v3 E1, v3 E2, float a1, float a2) { return (anchor + E1 * a1) + E2 * a2; }

PT_HD bool box_quad(v3 v1, v3 v2, v3 anchor, const Box6& q) {
  const v3 E1 = v1 / dot(v1, v1), E2 = v2 / dot(v2, v2);
  const v3 c00 = box_quad_corner(anchor, E1, E2, 0.0f, 0.0f), c10 = box_quad_corner(anchor, E1, E2, 1.0f, 0.0f);
  const v3 c11 = box_quad_corner(anchor, E1, E2, 1.0f, 1.0f), c01 = box_quad_corner(anchor, E1, E2, 0.0f, 1.0f);
  return box_tri_verts(c00, c10, c11, q) || box_tri_verts(c00, c11, c01, q);
}

// What a query collects.  any / count: the count alone.  list: the ids go to the box's own slice of the caller's prims while the total
// fits; nothing else is allocated, and a lane only ever re-reads what it stored itself.
struct BoxOut {
  int* slice;           // list: the box's slice; else unused
  long long cap;        // list: its capacity (a negative one reads as 0)
  int count;            // |S| so far
};

// A member of S.  true = the walk may stop (any).
template <int MODE>
PT_HD bool box_take(BoxOut& o, int prim) {
  if (MODE == BOX_LIST) { if ((long long)o.count < o.cap) o.slice[o.count] = prim; }
  o.count++;
  return MODE == BOX_ANY;
}

PT_HD void box_sift(int* a, int root, int end) {
  const int v = a[root];
  for (;;) {
    int child = 2 * root + 1;
    if (child >= end) break;
    if (child + 1 < end && a[child] < a[child + 1]) child++;
    if (v >= a[child]) break;
    a[root] = a[child]; root = child;
  }
  a[root] = v;
}
// Heap sort, ascending, in place: the ids are distinct, so the result is unique.
PT_HD void box_sort(int* a, int n) {
  for (int s = n / 2 - 1; s >= 0; s--) box_sift(a, s, n);
  for (int e = n - 1; e > 0; e--) { const int t = a[0]; a[0] = a[e]; a[e] = t; box_sift(a, 0, e); }
}

// The finished list: S ascending and -1 up to the capacity where it fits, else the whole slice -1.  Every byte of the slice is defined.
PT_HD void box_list_finish(BoxOut& o) {
  long long j = 0;
  if ((long long)o.count <= o.cap) { box_sort(o.slice, o.count); j = o.count; }
  for (; j < o.cap; j++) o.slice[j] = -1;
}

struct BoxTrav { int node, sp; };

// The brute-force lists in point_begin's order, then the set-up of the walk.  valid = box_valid's verdict.
template <int MODE>
PT_HD void box_begin(const SceneView& sc, const Box6& q, bool valid, BoxTrav& tv, BoxOut& o) {
  tv.sp = 0; tv.node = kTravDone;
  if (!valid) return;
  bool done = false;
  for (int i = 0; i < sc.nSpheres && !done; i++) {
    const DevSphere s = load_uniform(sc.spheres + i);
    if (box_sphere(s.center, s.radius, q)) done = box_take<MODE>(o, i);
  }
  for (int i = 0; i < sc.nQuads && !done; i++) {
    const DevQuad g = load_uniform(sc.quads + i);
    if (box_quad(g.v1, g.v2, g.anchor, q)) done = box_take<MODE>(o, sc.nSpheres + i);
  }
  tv.node = (done || sc.rootRef == kEmptyRef) ? kTravDone : sc.rootRef;
}

template <class Stack>
PT_HD void box_pop(BoxTrav& tv, Stack& st) {
  if (tv.sp > 0) { tv.sp--; tv.node = st.load(tv.sp); }
  else tv.node = kTravDone;
}

// One four-child node for a lane with tv.node >= 0: the first overlapping child is visited next, the others are pushed.  N64: the boxes
// come from the 64-byte node (pt_lbvh.h node64_plane), which contain the 128-byte node's.
template <bool N64, class Stack>
PT_HD void box_node_step(const SceneView& sc, const Box6& q, BoxTrav& tv, Stack& st) {
  float lo[3][4], hi[3][4];
  int ref[4];
  if (N64) {
    const Node64 n = load_const(at32(sc.nodes64, tv.node));
    const float o[3] = { n.ox, n.oy, n.oz }, s[3] = { n.sx, n.sy, n.sz };
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int a = 0; a < 3; a++)
      for (int c = 0; c < 4; c++) {
        lo[a][c] = node64_plane(o[a], s[a], (int)((n.q[a] >> (8 * c)) & 0xffu));
        hi[a][c] = node64_plane(o[a], s[a], (int)((n.q[3 + a] >> (8 * c)) & 0xffu));
      }
    for (int c = 0; c < 4; c++) ref[c] = n.ref[c];
  } else {
    const Node128 n = load_const(at32(sc.nodes, tv.node));
    lo[0][0] = n.lox.x; lo[0][1] = n.lox.y; lo[0][2] = n.lox.z; lo[0][3] = n.lox.w;
    lo[1][0] = n.loy.x; lo[1][1] = n.loy.y; lo[1][2] = n.loy.z; lo[1][3] = n.loy.w;
    lo[2][0] = n.loz.x; lo[2][1] = n.loz.y; lo[2][2] = n.loz.z; lo[2][3] = n.loz.w;
    hi[0][0] = n.hix.x; hi[0][1] = n.hix.y; hi[0][2] = n.hix.z; hi[0][3] = n.hix.w;
    hi[1][0] = n.hiy.x; hi[1][1] = n.hiy.y; hi[1][2] = n.hiy.z; hi[1][3] = n.hiy.w;
    hi[2][0] = n.hiz.x; hi[2][1] = n.hiz.y; hi[2][2] = n.hiz.z; hi[2][3] = n.hiz.w;
    for (int c = 0; c < 4; c++) ref[c] = n.ref[c];
  }
  int next = kTravDone;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int c = 3; c >= 0; c--) {
    const bool in = (ref[c] != kEmptyRef) & (lo[0][c] <= q.hi.x) & (hi[0][c] >= q.lo.x) & (lo[1][c] <= q.hi.y) & (hi[1][c] >= q.lo.y) &
                    (lo[2][c] <= q.hi.z) & (hi[2][c] >= q.lo.z);
    if (in) {
      if (next != kTravDone) { st.store(tv.sp, next); tv.sp++; }
      next = ref[c];
    }
  }
  if (next == kTravDone) box_pop(tv, st);
  else tv.node = next;
}

// One leaf for a lane with tv.node < 0 (and != kTravDone): the records are fetched as the point walk fetches them.
template <int MODE, class Stack>
PT_HD void box_leaf_step(const SceneView& sc, const Box6& q, BoxTrav& tv, Stack& st, BoxOut& o) {
  const int count = leaf_count(tv.node);
  const int triBase = sc.nSpheres + sc.nQuads;
  bool done = false;
  for (int base = 0; base < count && !done; base += 4) {
    LeafChunk ch;
    leaf_fetch4(sc, tv.node, base, ch);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 4; j++) {
      if (base + j < count && !done) {
        if (box_tri(ch.p0[j], ch.e0[j], ch.e1[j], q)) done = box_take<MODE>(o, triBase + ch.prim[j]);
      }
    }
  }
  if (done) tv.node = kTravDone;
  else box_pop(tv, st);
}

// One traversal step for a lane with tv.node != kTravDone (if-if form, as point_step).
template <int MODE, bool N64, class Stack>
PT_HD void box_step(const SceneView& sc, const Box6& q, BoxTrav& tv, Stack& st, BoxOut& o) {
  if (tv.node >= 0) box_node_step<N64>(sc, q, tv, st);
  else box_leaf_step<MODE>(sc, q, tv, st, o);
}

}  // namespace pt
