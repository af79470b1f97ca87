// pt_obb.h -- oriented box queries: the primitives that meet a rotated box (include/moptix.h "oriented box queries").
//
// A query is sixteen floats, 64 bytes:  cx cy cz  hx hy hz  a0.xyz  a1.xyz  a2.xyz  and one float that is not read.  c is the centre, h_j the
// half-extent along the box's own axis j, a_j that axis as a world-space direction.  The box is the closed set
//   { x : |dot(a_j, x - c)| <= h_j, j = 0, 1, 2 }.
// Valid (obb_valid; every comparison written so that a NaN fails it): floats 0..14 finite; h_j >= 0 (h_j == 0 allowed: a rectangle, a
// segment, a point); the axes orthonormal within kObbOrtho = 2^-10 in binary32 with AC1's dot, |dot(a_i, a_i) - 1| <= kObbOrtho and
// |dot(a_i, a_j)| <= kObbOrtho for i < j.  An invalid box meets nothing, decided before any traversal.
// S(obb) is the set of primitive ids (spheres, then quads, then triangles by original face id) whose predicate below holds; every primitive
// counts.  S is a function of the sixteen floats and the device records alone.
//
// What is computed once per query (obb_make), every operation in order (pt_math.h: AC1 dot = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), AC4
// every other operator one binary32 operation, no contraction):
//   b_j  = (|a_j.x|, |a_j.y|, |a_j.z|)
//   mc   = max(max(|c.x|, |c.y|), |c.z|);  mh = max(max(h.x, h.y), h.z)          (box_max: comparisons)
//   base = mc + mh
//   E_k  = (b_0.k * h.x + b_1.k * h.y) + b_2.k * h.z                              (products and sums, no fma)
//   g_w  = mh * kObbSkew + base * kObbMu                                          kObbSkew = 2^-6, kObbMu = 2^-16
//   wlo_k = c.k - (E_k + g_w);  whi_k = c.k + (E_k + g_w)                         the query's grown world box
//
// The predicates.
//   triangle (v0, v1, v2)   of the Tri48 record as box_tri sees it: v0 = p0, v1 = p0 + e0, v2 = p0 - e1.
//                      W  tmin / tmax = the per-axis min / max of v0, v1, v2 by comparisons; reject if tmax < wlo or tmin > whi on an
//                         axis (strict: a NaN or an equality rejects nothing)
//                      L  w_i = v_i - c;  u_i = (dot(a_0, w_i), dot(a_1, w_i), dot(a_2, w_i));
//                         then box_tri_verts(u_0, u_1, u_2, { -h, +h }) of pt_box.h exactly as it stands (its c is -h * 0.5 + h * 0.5 = 0
//                         and its half size h * 0.5 - (-h) * 0.5 = h).
//   sphere             m = (dot(a_0, s - c), dot(a_1, s - c), dot(a_2, s - c)) for the centre s, then box_sphere(m, radius, { -h, +h }): the
//                      surface, so a box wholly inside the ball meets nothing.  Exact up to the axes' departure from orthonormality: m is
//                      the centre in the box's frame only as far as the a_j are orthonormal (distances are off by up to 2^-9 of
//                      themselves at kObbOrtho), and up to the roundings of m.
//   quad               the four corners of box_quad (box_quad_corner on E1 = v1 / dot(v1, v1), E2 = v2 / dot(v2, v2)); the triangles
//                      (c00, c10, c11) and (c00, c11, c01) through the triangle predicate; the quad meets the box if either does.
//
// g_w and what W is for.  W makes the walk's world-axis test a conjunct of the predicate, the trick pt_box.h plays with its step A; it is
// meant never to decide anything else.  A point p that L places in the box up to L's own roundings d has local coordinates |m_j| <= h_j + d.
// With G = (dot(a_i, a_j)) within 2^-10 of the identity entry by entry, p - c = sum_j a_j (m_j + e_j) with |e_j| <= 2^-8 (mh + d), so
// |p.k - c.k| <= E_k + (sum_j |a_j.k|) (d + 2^-8 (mh + d)) <= E_k + 1.74 (2^-8 mh + 1.004 d), and 1.74 x 2^-8 = 0.0068 < kObbSkew = 0.0156: the
// skew term carries a factor two.  The roundings of E_k and c -+ (.) are below 2^-22 base; d is a few 2^-24 of the largest |u|, which
// base * kObbMu / 2 covers for every triangle whose vertices lie within 2^5 base of the centre.  For a triangle larger than that against the
// box W may reject where L alone would have accepted a graze; W is part of the definition, so nothing below depends on this paragraph.
//
// The walk.  One box per lane; a stack entry is one child reference; no ordering.  Spheres and quads are tested brute force in front of
// the walk, in point_begin's order.  Leaves are fetched with leaf_fetch4.  The node step enters a child [lo, hi] (empty references are
// skipped) iff both tests pass:
//   1  lo.k <= whi.k and hi.k >= wlo.k on the three world axes (exact comparisons; the box step W uses);
//   2  on each box axis j:  m = lo * 0.5 + hi * 0.5;  e = hi * 0.5 - lo * 0.5;  s = dot(a_j, m - c);  r = dot(b_j, e);
//      bm = the child's largest |plane| (max over the six by comparisons);  g = kObbMu * (base + bm);  pass iff |s| <= (h.j + r) + g.
// No cross-product axes: six axes are conservative and cheap.
//
// Why the walk's answer is the loop's over every primitive, bit for bit.  Take a triangle in S and any ancestor's box [lo, hi] of its leaf,
// in either node form, built or refitted.
//   * The box contains the computed vertices v0, v1, v2 exactly: pt_box.h's argument (the builder pads every triangle's box by padAbs +
//     1e-6 |v| per plane, eight and eighty times the two roundings that separate v1, v2 from the boxed vertices; the refit reproduces the
//     padding, pt_refit.h; boxes only grow towards the root, min / max being exact, and into the 64-byte form, whose planes contain the
//     128-byte node's).  So lo <= tmin and tmax <= hi per axis.
//   * Test 1.  W did not reject: tmax >= wlo and tmin <= whi.  Hence hi >= tmax >= wlo and lo <= tmin <= whi: test 1 passes, on the same
//     floats wlo, whi that W compared.
//   * Test 2.  Step A of box_tri_verts did not reject on local axis j: min_i u_i.j <= h.j and max_i u_i.j >= -h.j for the computed u.
//     Write P_i = a_j . (v_i - c) in real arithmetic.  u_i.j = fl(dot(a_j, fl(v_i - c))) has |u_i.j - P_i| <= err_u with
//       err_u <= 2^-24 sum_k |a_j.k| |v_i.k - c.k|           (the subtraction w_i = fl(v_i - c), one rounding per component)
//              + 3 x 2^-24 sum_k |a_j.k| |w_i.k| (1 + 2^-22)  (AC1's product and two fused sums, three roundings)
//             <= 4 x 2^-24 x 1.74 x (bm + mc) (1 + 2^-22)  <  2^-21 (bm + mc),
//     using sum_k |a_j.k| <= sqrt(3) |a_j| <= 1.74 and |v_i.k| <= bm because the box contains v_i.  So some P_i <= h.j + err_u and some
//     P_i >= -h.j - err_u.  The exact projection of the box onto a_j is [S - R, S + R] with S = a_j . (M - c), R = |a_j| . e_x, M and e_x
//     the exact centre and half size, and it contains every P_i: S - R <= h.j + err_u and S + R >= -h.j - err_u, i.e.
//     |S| <= h.j + R + err_u.
//     The node step computes m with |m - M| <= 2^-24 bm per axis (the halvings are exact, one rounded sum), e with |e - e_x| <= 2^-24 bm,
//     s with |s - S| <= 1.74 x 2^-24 bm + 2^-21 (bm + mc) and r with |r - R| <= 1.74 x 2^-24 bm + 3 x 1.74 x 2^-24 bm; the two rounded sums
//     of (h.j + r) + g lose at most 2^-23 (mh + 1.74 bm + g), and g itself is low by at most 3 x 2^-24 g.  The sum of all of it is below
//       2^-21 (bm + mc) x 2 + 2^-21 bm + 2^-22 (mh + bm)  <  2^-19 (base + bm),
//     and g = 2^-16 (base + bm) carries a factor 8 over that bound.  So |s| <= (h.j + r) + g holds in binary32: test 2 passes.
//   * Hence every ancestor is entered, the leaf is reached, and the predicate is evaluated on the same record by the same operations.  A
//     triangle outside S is rejected wherever it is tested.  A wider margin may cost time, never a bit.
// Not covered: scenes smaller than 1e-30 units (pt_box.h) or with coordinates above 2^100 (products that underflow or overflow are outside
// the bound on err_u), and centres so large that c -+ (E + g_w) or base is not finite -- there the comparisons fail and the box meets nothing
// or prunes what it should not.
// Used by the oriented box kernel (obbkernel.hip) and by its CPU mirror (tests/obbsim/obbsim.cpp); nothing else includes it.
#pragma once
#include "pt_box.h"

namespace pt {

constexpr float kObbOrtho = 0.0009765625f;              // 2^-10: how far the axes may be from orthonormal
constexpr float kObbSkew = 0.015625f;                   // 2^-6: the world box's growth per unit of the largest half-extent (g_w)
constexpr float kObbMu = 0.0000152587890625f;           // 2^-16: the node step's margin per unit of base + bm; a factor 8 over the bound above

struct Obb {
  v3 c, h;
  v3 a[3], b[3];          // the axes and their absolute values
  v3 wlo, whi;            // the grown world box
  float base;             // max |c| + max h
};

PT_HD v3 obb_abs3(v3 v) { return mk3(__builtin_fabsf(v.x), __builtin_fabsf(v.y), __builtin_fabsf(v.z)); }
PT_HD float obb_max3(v3 v) { return box_max(box_max(v.x, v.y), v.z); }

// f: the query's sixteen floats (the last is not read).  false = an invalid box.
PT_HD bool obb_valid(const float f[16]) {
  bool ok = true;
  for (int k = 0; k < 15; k++) ok = ok & point_finite(f[k]);
  for (int k = 3; k < 6; k++) ok = ok & (f[k] >= 0.0f);
  const v3 a0 = mk3(f[6], f[7], f[8]), a1 = mk3(f[9], f[10], f[11]), a2 = mk3(f[12], f[13], f[14]);
  const float d00 = dot(a0, a0), d11 = dot(a1, a1), d22 = dot(a2, a2), d01 = dot(a0, a1), d02 = dot(a0, a2), d12 = dot(a1, a2);
  ok = ok & (__builtin_fabsf(d00 - 1.0f) <= kObbOrtho) & (__builtin_fabsf(d11 - 1.0f) <= kObbOrtho) & (__builtin_fabsf(d22 - 1.0f) <= kObbOrtho);
  ok = ok & (__builtin_fabsf(d01) <= kObbOrtho) & (__builtin_fabsf(d02) <= kObbOrtho) & (__builtin_fabsf(d12) <= kObbOrtho);
  return ok;
}

PT_HD Obb obb_make(const float f[16]) {
  Obb q;
  q.c = mk3(f[0], f[1], f[2]); q.h = mk3(f[3], f[4], f[5]);
  q.a[0] = mk3(f[6], f[7], f[8]); q.a[1] = mk3(f[9], f[10], f[11]); q.a[2] = mk3(f[12], f[13], f[14]);
  for (int j = 0; j < 3; j++) q.b[j] = obb_abs3(q.a[j]);
  const float mc = obb_max3(obb_abs3(q.c)), mh = obb_max3(q.h);
  q.base = mc + mh;
  const v3 E = (q.b[0] * q.h.x + q.b[1] * q.h.y) + q.b[2] * q.h.z;
  const float gw = mh * kObbSkew + q.base * kObbMu;
  q.wlo = q.c - (E + gw);
  q.whi = q.c + (E + gw);
  return q;
}

PT_HD v3 obb_local(const Obb& q, v3 p) {
  const v3 w = p - q.c;
  return mk3(dot(q.a[0], w), dot(q.a[1], w), dot(q.a[2], w));
}

PT_HD Box6 obb_local_box(const Obb& q) { Box6 l; l.lo = -q.h; l.hi = q.h; return l; }

// The triangle predicate on three vertices.
PT_HD bool obb_tri_verts(v3 v0, v3 v1, v3 v2, const Obb& q) {
  // W
  const v3 tmin = mk3(box_min(box_min(v0.x, v1.x), v2.x), box_min(box_min(v0.y, v1.y), v2.y), box_min(box_min(v0.z, v1.z), v2.z));
  const v3 tmax = mk3(box_max(box_max(v0.x, v1.x), v2.x), box_max(box_max(v0.y, v1.y), v2.y), box_max(box_max(v0.z, v1.z), v2.z));
  if ((tmax.x < q.wlo.x) | (tmin.x > q.whi.x) | (tmax.y < q.wlo.y) | (tmin.y > q.whi.y) | (tmax.z < q.wlo.z) | (tmin.z > q.whi.z)) return false;
  // L
  return box_tri_verts(obb_local(q, v0), obb_local(q, v1), obb_local(q, v2), obb_local_box(q));
}

// The triangle predicate on a Tri48 record's p0, e0, e1.
PT_HD bool obb_tri(v3 p0, v3 e0, v3 e1, const Obb& q) { return obb_tri_verts(p0, p0 + e0, p0 - e1, q); }

PT_HD bool obb_sphere(v3 centre, float radius, const Obb& q) { return box_sphere(obb_local(q, centre), radius, obb_local_box(q)); }

PT_HD bool obb_quad(v3 v1, v3 v2, v3 anchor, const Obb& q) {
  const v3 E1 = v1 / dot(v1, v1), E2 = v2 / dot(v2, v2);
  const v3 c00 = box_quad_corner(anchor, E1, E2, 0.0f, 0.0f), c10 = box_quad_corner(anchor, E1, E2, 1.0f, 0.0f);
  const v3 c11 = box_quad_corner(anchor, E1, E2, 1.0f, 1.0f), c01 = box_quad_corner(anchor, E1, E2, 0.0f, 1.0f);
  return obb_tri_verts(c00, c10, c11, q) || obb_tri_verts(c00, c11, c01, q);
}

// What the mirror counts per query, where asked for: node steps taken and triangles put through the predicate.
struct ObbWork { long long nodeSteps, trisTested; };

// The brute-force lists in point_begin's order, then the set-up of the walk.  valid = obb_valid's verdict.
template <int MODE>
PT_HD void obb_begin(const SceneView& sc, const Obb& q, bool valid, BoxTrav& tv, BoxOut& o) {
  tv.sp = 0; tv.node = kTravDone;
  if (!valid) return;
  bool done = false;
  for (int i = 0; i < sc.nSpheres && !done; i++) {
    const DevSphere s = load_uniform(sc.spheres + i);
    if (obb_sphere(s.center, s.radius, q)) done = box_take<MODE>(o, i);
  }
  for (int i = 0; i < sc.nQuads && !done; i++) {
    const DevQuad g = load_uniform(sc.quads + i);
    if (obb_quad(g.v1, g.v2, g.anchor, q)) done = box_take<MODE>(o, sc.nSpheres + i);
  }
  tv.node = (done || sc.rootRef == kEmptyRef) ? kTravDone : sc.rootRef;
}

// Test 2 of the node step on box axis j for the child of centre m, half size e and largest |plane| bm.
PT_HD bool obb_axis_passes(const Obb& q, int j, float hj, v3 m, v3 e, float g) {
  const float s = dot(q.a[j], m - q.c), r = dot(q.b[j], e);
  return __builtin_fabsf(s) <= (hj + r) + g;
}

// One four-child node for a lane with tv.node >= 0: the first child that passes is visited next, the others are pushed.  N64: the boxes
// come from the 64-byte node (pt_lbvh.h node64_plane), which contain the 128-byte node's.
template <bool N64, class Stack>
PT_HD void obb_node_step(const SceneView& sc, const Obb& q, BoxTrav& tv, Stack& st) {
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
    bool in = (ref[c] != kEmptyRef) & (lo[0][c] <= q.whi.x) & (hi[0][c] >= q.wlo.x) & (lo[1][c] <= q.whi.y) & (hi[1][c] >= q.wlo.y) &
              (lo[2][c] <= q.whi.z) & (hi[2][c] >= q.wlo.z);
    const v3 l = mk3(lo[0][c], lo[1][c], lo[2][c]), u = mk3(hi[0][c], hi[1][c], hi[2][c]);
    const v3 m = l * 0.5f + u * 0.5f, e = u * 0.5f - l * 0.5f;
    const float bm = box_max(obb_max3(obb_abs3(l)), obb_max3(obb_abs3(u)));
    const float g = kObbMu * (q.base + bm);
    const bool p0 = obb_axis_passes(q, 0, q.h.x, m, e, g), p1 = obb_axis_passes(q, 1, q.h.y, m, e, g), p2 = obb_axis_passes(q, 2, q.h.z, m, e, g);
    in = in & p0 & p1 & p2;
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
PT_HD void obb_leaf_step(const SceneView& sc, const Obb& q, BoxTrav& tv, Stack& st, BoxOut& o, ObbWork* work) {
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
#if !defined(__HIP_DEVICE_COMPILE__)
        if (work) work->trisTested++;
#endif
        if (obb_tri(ch.p0[j], ch.e0[j], ch.e1[j], q)) done = box_take<MODE>(o, triBase + ch.prim[j]);
      }
    }
  }
  if (done) tv.node = kTravDone;
  else box_pop(tv, st);
}

// One traversal step for a lane with tv.node != kTravDone (if-if form, as box_step).  work: the mirror's counters, null on the device.
template <int MODE, bool N64, class Stack>
PT_HD void obb_step(const SceneView& sc, const Obb& q, BoxTrav& tv, Stack& st, BoxOut& o, ObbWork* work = nullptr) {
  if (tv.node >= 0) {
#if !defined(__HIP_DEVICE_COMPILE__)
    if (work) work->nodeSteps++;
#endif
    obb_node_step<N64>(sc, q, tv, st);
  } else {
    obb_leaf_step<MODE>(sc, q, tv, st, o, work);
  }
}

}  // namespace pt
