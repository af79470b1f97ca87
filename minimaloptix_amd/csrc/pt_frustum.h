// pt_frustum.h -- frustum queries: the primitives that meet a convex region bounded by six planes (include/moptix.h "frustum queries").
//
// A query is 24 floats, 96 bytes: six planes  nx ny nz d.  The region is the closed set { x : dot(n_j, x) + d_j >= 0, j = 0..5 }: normals
// point inwards (what Gribb-Hartmann extraction from a clip matrix gives) and need not be unit length.  Valid (frustum_valid): all 24
// floats finite.  An invalid query meets nothing, decided before any traversal.  A plane 0 0 0 d with d >= 0 constrains nothing (a wedge,
// a slab, a half-space, an unbounded pyramid need no special case: every test below passes it); with d < 0 it empties the region (every
// test below fails it); six zero planes meet every primitive.
// S(frustum) is the set of primitive ids (spheres, then quads, then triangles by original face id) whose predicate below holds; every
// primitive counts.  S is a function of the 24 floats and the device records alone.
//
// What is computed once per query (frustum_make), every operation in order (pt_math.h: AC1 dot = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)),
// AC4 every other operator one binary32 operation, no contraction):
//   nb_j  = (|n_j.x| + |n_j.y|) + |n_j.z|
//   len_j = sqrtf(dot(n_j, n_j))
// |n_j| = (|n_j.x|, |n_j.y|, |n_j.z|) and |d_j| are sign-bit clears, exact, written where they are used.
//
// The predicates.
//   triangle (v0, v1, v2)   of the Tri48 record as box_tri sees it: v0 = p0, v1 = p0 + e0, v2 = p0 - e1.
//                    s_ji = dot(n_j, v_i) + d_j, eighteen values (the dot, then one sum).
//                      R  reject if on some plane j all three s_ji < 0 (strict: a NaN or an equality rejects nothing)
//                      A  accept if some vertex i has s_ji >= 0 on all six planes
//                      E  each edge (a, b) of (0, 1), (1, 2), (2, 0) as a parameter interval: t0 = 0, t1 = 1; per plane j, in any order,
//                         with s_a = s_ja, s_b = s_jb: if s_a < 0 and s_b < 0 the edge fails; else if s_a < 0,
//                         t0 = max(t0, s_a / (s_a - s_b)); else if s_b < 0, t1 = min(t1, s_a / (s_a - s_b))  (one subtraction, one division,
//                         a comparison).  Accept if an edge did not fail and ends with t0 <= t1.
//                      V  what is left is a triangle whose edges all miss the region while its face may still cut through it.  In the
//                         triangle's own coordinates (x = v0 + u (v1 - v0) + v (v2 - v0)) plane j is c_j(u, v) = A_j u + B_j v + C_j with
//                         A_j = s_j1 - s_j0, B_j = s_j2 - s_j0, C_j = s_j0.  For each of the 15 pairs j < k:
//                           det = A_j * B_k - A_k * B_j;  skipped if det == 0 (or NaN: every comparison below fails);
//                           u = (B_j * C_k - B_k * C_j) / det;  v = (A_k * C_j - A_j * C_k) / det          (two products, one subtraction, one division)
//                           accept if u >= 0, v >= 0, u + v <= 1 and (A_m * u + B_m * v) + C_m >= 0 for the four planes m other than j, k.
//                         Else the triangle does not meet the region.
//                    Why V is complete in exact arithmetic: after E no edge of the triangle meets the region, so region and triangle's
//                    plane meet, if at all, in a convex polygon strictly inside the triangle: it is bounded, so it has a corner, and a
//                    corner is the crossing of two of the six lines c_j = 0 that satisfies the other four.  A zero-area triangle needs no
//                    special case: its edges carry it through E, and every det is zero.
//                    Two invariances follow from the structure and hold bit for bit.  The order of the six planes plays no part: R, A
//                    are OR / AND over planes, E's t0 and t1 are a max and a min over planes, and swapping j and k in V negates det and
//                    both numerators exactly.  Multiplying a plane's four floats by a power of two multiplies its s, A, B, C, det and
//                    the numerators by powers of two exactly, short of overflow and underflow: every quotient and comparison is the same.
//   sphere           the plane rule on the ball: s_j = dot(n_j, centre) + d_j >= -(radius * len_j) on all six planes.  This is what view
//                    culling asks ("can the ball be seen"); it is exact for half-spaces and slabs.  It is the BALL, not the surface the
//                    box queries test: a region wholly inside the ball meets it.  At the region's edges and corners it is conservative:
//                    a ball within `radius` of two planes but not of their common edge is reported.
//                    For the same reason two contradictory planes (an empty region) still report a ball that reaches across both.
//   quad             the four corners of box_quad (box_quad_corner on E1 = v1 / dot(v1, v1), E2 = v2 / dot(v2, v2)); the triangles
//                    (c00, c10, c11) and (c00, c11, c01) through the triangle predicate; the quad meets the region if either does.
//
// The walk.  One query per lane; a stack entry is one child reference; no ordering.  Spheres and quads are tested brute force in front of
// the walk, in point_begin's order.  Leaves are fetched with leaf_fetch4.  The node step enters a child [lo, hi] (empty references are
// skipped) iff on every plane j
//   m = lo * 0.5 + hi * 0.5;  e = hi * 0.5 - lo * 0.5;  bm = the child's largest |plane| (max over the six by comparisons);
//   g_j = kFrustumMu * (nb_j * bm + |d_j|);    (dot(n_j, m) + d_j) + dot(|n_j|, e)  >=  -g_j.
// No cross-product axes and no corner box of the region: large nodes near the region's corners are entered needlessly, which costs time
// and never a bit.  The region may be unbounded.
//
// Why the walk's answer is the loop's over every primitive, bit for bit.  Take a triangle in S, a plane j and any ancestor's box [lo, hi]
// of its leaf, in either node form, built or refitted.  Write eps = 2^-24 and T = nb_j bm + |d_j|.
//   * R is a conjunct of the predicate (A, E and V are only reached behind it): some computed vertex v_i has a computed s_ji >= 0.
//   * The box contains the computed vertices v0, v1, v2 exactly: pt_box.h's argument (the builder pads every triangle's box by padAbs +
//     1e-6 |v| per plane, eight and eighty times the two roundings that separate v1, v2 from the boxed vertices; the refit reproduces the
//     padding, pt_refit.h; boxes only grow towards the root, min / max being exact, and into the 64-byte form, whose planes contain the
//     128-byte node's).  So |v_i.k| <= bm on every axis.
//   * With P = n_j . v_i + d_j in real arithmetic, s_ji = fl(fl_dot(n_j, v_i) + d_j) has three roundings in AC1's dot, each at most eps
//     of sum_k |n_j.k| |v_i.k| <= nb_j bm (up to second order), and one in the sum, at most eps T: |s_ji - P| <= 4 eps T (1 + 2^-22).
//     Hence P >= -4 eps T (1 + 2^-22).
//   * The exact maximum of the plane function over the box is F = n_j . M + d_j + |n_j| . e_x, M and e_x the exact centre and half size,
//     and the box contains v_i: F >= P.
//   * The node step computes m with |m - M| <= eps bm per axis (the halvings are exact, one rounded sum) and e with |e - e_x| <= eps bm;
//     dot(n_j, m) is off n_j . M by at most eps nb_j bm for m and 3 eps nb_j bm for its own roundings; the sum with d_j loses at most
//     eps T; dot(|n_j|, e) is off |n_j| . e_x by at most 4 eps nb_j bm likewise; the last sum loses at most eps (2 nb_j bm + |d_j|).
//     Together at most 11 eps T (1 + 2^-22).  nb_j itself is two roundings from sum_k |n_j.k| and g_j two roundings from its real value
//     (the product with the power of two kFrustumMu is exact): factors 1 +- 2^-22, absorbed below.
//   * So the computed left side is at least F - 11 eps T >= -15 eps T (1 + 2^-21) > -2^-20 T, and g_j = 2^-16 T carries a factor 16 over
//     that bound (the oriented box step's margin carries 8).  The comparison holds in binary32 on every plane: the child is entered.
//   * Hence every ancestor is entered, the leaf is reached, and the predicate is evaluated on the same record by the same operations.  A
//     triangle outside S is rejected wherever it is tested.  A wider margin may cost time, never a bit.
// Not covered: scenes smaller than 1e-30 units (pt_box.h), and magnitudes whose products n_j.k * v.k, nb_j * bm or their sums overflow
// or underflow (coordinates or normals beyond about 2^60, or below 2^-60 beside a non-zero d_j): there the bounds on the roundings do
// not hold, and a plane scaled by a power of two is no longer scaled exactly.
// Used by the frustum kernel (frustumkernel.hip) and by its CPU mirror (tests/frustumsim/frustumsim.cpp); nothing else includes it.
#pragma once
#include "pt_box.h"

namespace pt {

constexpr float kFrustumMu = 0.0000152587890625f;       // 2^-16: the node step's margin per unit of nb_j * bm + |d_j|; a factor 16 over the bound above

#if defined(__HIP_DEVICE_COMPILE__)
#define PT_FRUSTUM_UNROLL _Pragma("unroll")
#define PT_FRUSTUM_NOUNROLL _Pragma("nounroll")
#else
#define PT_FRUSTUM_UNROLL
#define PT_FRUSTUM_NOUNROLL
#endif

struct Frustum {
  v3 n[6];
  float d[6];
  float nb[6];            // (|n.x| + |n.y|) + |n.z|
  float len[6];           // sqrtf(dot(n, n))
};

PT_HD v3 frustum_abs3(v3 v) { return mk3(__builtin_fabsf(v.x), __builtin_fabsf(v.y), __builtin_fabsf(v.z)); }

// f: the query's 24 floats.  false = an invalid query.
PT_HD bool frustum_valid(const float f[24]) {
  bool ok = true;
  PT_FRUSTUM_UNROLL
  for (int k = 0; k < 24; k++) ok = ok & point_finite(f[k]);
  return ok;
}

PT_HD Frustum frustum_make(const float f[24]) {
  Frustum q;
  PT_FRUSTUM_UNROLL
  for (int j = 0; j < 6; j++) {
    q.n[j] = mk3(f[4 * j], f[4 * j + 1], f[4 * j + 2]);
    q.d[j] = f[4 * j + 3];
    const v3 a = frustum_abs3(q.n[j]);
    q.nb[j] = (a.x + a.y) + a.z;
    q.len[j] = __builtin_sqrtf(dot(q.n[j], q.n[j]));
  }
  return q;
}

// The value itself, behind a barrier the device compiler cannot see through: without it the eighteen sign tests of R and A stay alive as
// wave masks for E to use again, two scalar registers each, and the kernel spills scalar registers.  No operation: the bits are x's.
PT_HD float frustum_again(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(x));
#endif
  return x;
}

// Which stage decided a triangle (the mirror reports it; the kernel does not ask).
enum { FRUSTUM_NONE = 0, FRUSTUM_R = 1, FRUSTUM_A = 2, FRUSTUM_E = 3, FRUSTUM_V = 4 };

// One edge of stage E on its six pairs of plane values.  The failed edge is carried in t0 itself (2 > any t1), so that the six planes
// leave two floats and no wave masks behind: t is in [0, 1] wherever it is used (|s_a - s_b| rounds to no less than |s_a|, |s_b|), so
// max(t0, 0) and min(t1, 1) change nothing and the answer is the description's.
PT_HD bool frustum_edge_meets(const float sa[6], const float sb[6]) {
  float t0 = 0.0f, t1 = 1.0f;
  PT_FRUSTUM_UNROLL
  for (int j = 0; j < 6; j++) {
    const bool na = sa[j] < 0.0f, nb = sb[j] < 0.0f;
    const float t = sa[j] / (sa[j] - sb[j]);
    t0 = box_max(t0, na ? (nb ? 2.0f : t) : 0.0f);
    t1 = box_min(t1, (nb & !na) ? t : 1.0f);
  }
  return t0 <= t1;
}

// The triangle predicate on three vertices; stage: which of R, A, E, V decided (FRUSTUM_NONE: none accepted, the answer is false).
PT_HD bool frustum_tri_stage(v3 v0, v3 v1, v3 v2, const Frustum& q, int& stage) {
  float s0[6], s1[6], s2[6];
  bool rej = false, in0 = true, in1 = true, in2 = true;
  PT_FRUSTUM_UNROLL
  for (int j = 0; j < 6; j++) {
    s0[j] = dot(q.n[j], v0) + q.d[j];
    s1[j] = dot(q.n[j], v1) + q.d[j];
    s2[j] = dot(q.n[j], v2) + q.d[j];
    rej = rej | ((s0[j] < 0.0f) & (s1[j] < 0.0f) & (s2[j] < 0.0f));
    in0 = in0 & (s0[j] >= 0.0f); in1 = in1 & (s1[j] >= 0.0f); in2 = in2 & (s2[j] >= 0.0f);
  }
  // R
  stage = FRUSTUM_R;
  if (rej) return false;
  // A
  stage = FRUSTUM_A;
  if (in0 | in1 | in2) return true;
  // E
  stage = FRUSTUM_E;
  PT_FRUSTUM_UNROLL
  for (int j = 0; j < 6; j++) { s0[j] = frustum_again(s0[j]); s1[j] = frustum_again(s1[j]); s2[j] = frustum_again(s2[j]); }
  const bool e01 = frustum_edge_meets(s0, s1), e12 = frustum_edge_meets(s1, s2), e20 = frustum_edge_meets(s2, s0);
  if (e01 || e12 || e20) return true;
  // V
  stage = FRUSTUM_V;
  float A[6], B[6];
  PT_FRUSTUM_UNROLL
  for (int j = 0; j < 6; j++) { A[j] = s1[j] - s0[j]; B[j] = s2[j] - s0[j]; }
  bool hit = false;
  PT_FRUSTUM_UNROLL
  for (int j = 0; j < 5; j++) {
    PT_FRUSTUM_UNROLL
    for (int k = j + 1; k < 6; k++) {
      const float det = A[j] * B[k] - A[k] * B[j];
      const float u = (B[j] * s0[k] - B[k] * s0[j]) / det, v = (A[k] * s0[j] - A[j] * s0[k]) / det;
      bool ok = (det != 0.0f) & (u >= 0.0f) & (v >= 0.0f) & (u + v <= 1.0f);
      PT_FRUSTUM_UNROLL
      for (int m = 0; m < 6; m++)
        if (m != j && m != k) ok = ok & ((A[m] * u + B[m] * v) + s0[m] >= 0.0f);
      hit = hit | ok;
    }
  }
  if (hit) return true;
  stage = FRUSTUM_NONE;
  return false;
}

PT_HD bool frustum_tri_verts(v3 v0, v3 v1, v3 v2, const Frustum& q) {
  int stage;
  return frustum_tri_stage(v0, v1, v2, q, stage);
}

// The triangle predicate on a Tri48 record's p0, e0, e1.
PT_HD bool frustum_tri(v3 p0, v3 e0, v3 e1, const Frustum& q) { return frustum_tri_verts(p0, p0 + e0, p0 - e1, q); }

PT_HD bool frustum_sphere(v3 centre, float radius, const Frustum& q) {
  bool in = true;
  PT_FRUSTUM_UNROLL
  for (int j = 0; j < 6; j++) in = in & (dot(q.n[j], centre) + q.d[j] >= -(radius * q.len[j]));
  return in;
}

PT_HD bool frustum_quad(v3 v1, v3 v2, v3 anchor, const Frustum& q) {
  const v3 E1 = v1 / dot(v1, v1), E2 = v2 / dot(v2, v2);
  const v3 c00 = box_quad_corner(anchor, E1, E2, 0.0f, 0.0f), c11 = box_quad_corner(anchor, E1, E2, 1.0f, 1.0f);
  bool meets = false;
  // one copy of the triangle function, not two: (c00, c10, c11), then (c00, c11, c01)
  PT_FRUSTUM_NOUNROLL
  for (int h = 0; h < 2 && !meets; h++) {
    const v3 c = box_quad_corner(anchor, E1, E2, h == 0 ? 1.0f : 0.0f, h == 0 ? 0.0f : 1.0f);
    meets = frustum_tri_verts(c00, h == 0 ? c : c11, h == 0 ? c11 : c, q);
  }
  return meets;
}

// What the mirror counts per query, where asked for: node steps taken and triangles put through the predicate.
struct FrustumWork { long long nodeSteps, trisTested; };

// The brute-force lists in point_begin's order, then the set-up of the walk.  valid = frustum_valid's verdict.
template <int MODE>
PT_HD void frustum_begin(const SceneView& sc, const Frustum& q, bool valid, BoxTrav& tv, BoxOut& o) {
  tv.sp = 0; tv.node = kTravDone;
  if (!valid) return;
  bool done = false;
  for (int i = 0; i < sc.nSpheres && !done; i++) {
    const DevSphere s = load_uniform(sc.spheres + i);
    if (frustum_sphere(s.center, s.radius, q)) done = box_take<MODE>(o, i);
  }
  for (int i = 0; i < sc.nQuads && !done; i++) {
    const DevQuad g = load_uniform(sc.quads + i);
    if (frustum_quad(g.v1, g.v2, g.anchor, q)) done = box_take<MODE>(o, sc.nSpheres + i);
  }
  tv.node = (done || sc.rootRef == kEmptyRef) ? kTravDone : sc.rootRef;
}

// The node step's test of the child of centre m, half size e and largest |plane| bm against the six planes.
PT_HD bool frustum_box_passes(const Frustum& q, v3 m, v3 e, float bm) {
  bool in = true;
  PT_FRUSTUM_UNROLL
  for (int j = 0; j < 6; j++) {
    const float g = kFrustumMu * (q.nb[j] * bm + __builtin_fabsf(q.d[j]));
    in = in & ((dot(q.n[j], m) + q.d[j]) + dot(frustum_abs3(q.n[j]), e) >= -g);
  }
  return in;
}

// One four-child node for a lane with tv.node >= 0: the first child that passes is visited next, the others are pushed.  N64: the boxes
// come from the 64-byte node (pt_lbvh.h node64_plane), which contain the 128-byte node's.
template <bool N64, class Stack>
PT_HD void frustum_node_step(const SceneView& sc, const Frustum& q, BoxTrav& tv, Stack& st) {
  float lo[3][4], hi[3][4];
  int ref[4];
  if (N64) {
    const Node64 n = load_const(at32(sc.nodes64, tv.node));
    const float o[3] = { n.ox, n.oy, n.oz }, s[3] = { n.sx, n.sy, n.sz };
    PT_FRUSTUM_UNROLL
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
  PT_FRUSTUM_UNROLL
  for (int c = 3; c >= 0; c--) {
    const v3 l = mk3(lo[0][c], lo[1][c], lo[2][c]), u = mk3(hi[0][c], hi[1][c], hi[2][c]);
    const v3 m = l * 0.5f + u * 0.5f, e = u * 0.5f - l * 0.5f;
    const v3 al = frustum_abs3(l), au = frustum_abs3(u);
    const float bm = box_max(box_max(box_max(al.x, al.y), al.z), box_max(box_max(au.x, au.y), au.z));
    const bool in = (ref[c] != kEmptyRef) & frustum_box_passes(q, m, e, bm);
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
PT_HD void frustum_leaf_step(const SceneView& sc, const Frustum& q, BoxTrav& tv, Stack& st, BoxOut& o, FrustumWork* work) {
  const int count = leaf_count(tv.node);
  const int triBase = sc.nSpheres + sc.nQuads;
  bool done = false;
  for (int base = 0; base < count && !done; base += 4) {
    LeafChunk ch;
    leaf_fetch4(sc, tv.node, base, ch);
    // One copy of the triangle function, not four: slot 0 is tested and the chunk moved down one slot, every index a constant, so the
    // chunk stays in registers.
    PT_FRUSTUM_NOUNROLL
    for (int j = 0; j < 4; j++) {
      if (base + j < count && !done) {
#if !defined(__HIP_DEVICE_COMPILE__)
        if (work) work->trisTested++;
#endif
        if (frustum_tri(ch.p0[0], ch.e0[0], ch.e1[0], q)) done = box_take<MODE>(o, triBase + ch.prim[0]);
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

// One traversal step for a lane with tv.node != kTravDone (if-if form, as box_step).  work: the mirror's counters, null on the device.
template <int MODE, bool N64, class Stack>
PT_HD void frustum_step(const SceneView& sc, const Frustum& q, BoxTrav& tv, Stack& st, BoxOut& o, FrustumWork* work = nullptr) {
  if (tv.node >= 0) {
#if !defined(__HIP_DEVICE_COMPILE__)
    if (work) work->nodeSteps++;
#endif
    frustum_node_step<N64>(sc, q, tv, st);
  } else {
    frustum_leaf_step<MODE>(sc, q, tv, st, o, work);
  }
}

}  // namespace pt
