// pt_sweep.h -- sphere sweep queries: the first contact of a moving sphere with the built scene (include/moptix.h "sweep queries").
//
// A query is eight floats  ox oy oz dx dy dz radius tmax  (the ray layout with radius in the tmin slot).  The sphere's centre is
// c(t) = o + d * t for t in [0, tmax], in units of |d|; d is used as given.  Invalid -- a miss, decided before any traversal: any of the
// eight non-finite, d zero in all three components, radius <= 0, tmax <= 0.
//   closest   the primitive least by (toi, primitive id) among those with a contact in [0, tmax] (toi = the per-primitive function below;
//             at exactly equal toi the lower id, rule D5; toi == tmax counts).  The record: t = toi, and p, u, v exactly what point_tri /
//             point_sphere / point_quad (pt_point.h) return for q = o + d * t (one product and one sum per component) on the winner: the
//             contact point.  The contact normal is (q - p) / radius.  A miss: t = tmax as given, prim = mat = -1, the rest 0.
//   any       1 iff the closest sweep on the same query reports a primitive; the walk stops at the first contact it accepts.
// Every primitive counts, whatever its material.  The answer is a function of the query and the device records alone: tree, leaf size,
// node format, grid size and scheduling play no part.
//
// The per-primitive time of contact, every operation in order (pt_math.h: AC1 dot, AC2 cross, AC3 v / s = v * (1 / s), AC4 no contraction;
// division and square root correctly rounded).  r2 = radius * radius, dd = dot(d, d), both once per query.
//   ball(m, e, ee, R2)   the ray from the origin of the frame along e (ee = dot(e, e)) against the ball of squared radius R2 about m,
//                    about the foot of the perpendicular:  tca = dot(m, e) / ee;  perp = m - e * tca;  disc = R2 - dot(perp, perp);
//                    none unless disc >= 0;  s = sqrt(disc / ee);  t = tca - s;  where t < 0: none unless tca + s >= 0 (the origin is
//                    inside), then t = 0.  Not |m|^2 - R2: that cancels at the scale of |m|^2, this at the scale of |m| ulps of perp.
//   vertex(a)        ball(a - o, d, dd, r2)
//   edge(a, ab)      the cylinder of radius `radius` about the line, in the plane across it:  den = dot(ab, ab), none unless den > 0;
//                    m = a - o;  dpar = dot(d, ab) / den;  mpar = dot(m, ab) / den;  dperp = d - ab * dpar;  mperp = m - ab * mpar;
//                    A = dot(dperp, dperp), none unless A > 0;  t = ball(mperp, dperp, A, r2);  the edge parameter s = dpar * t - mpar;
//                    accepted when 0 <= s <= 1
//   face             point_tri's scaled normal: ea = e0, eb = -e1, n = cross(ea, eb), m = its largest |component|, none unless m > 0 and
//                    finite; sc = 2^-floor(log2 m), ns = n * sc, nn = dot(ns, ns).  h = dot(ns, o - v0), g = dot(ns, d),
//                    rn = radius * sqrt(nn);  ha = |h|, ga = h < 0 ? -g : g (the rate of ha).  ha <= rn: t = 0.  Otherwise none unless
//                    ga < 0, and t = (ha - rn) / -ga: the plane offset by radius towards the origin's side.  Accepted by point_tri's inside
//                    test at w = (o + d * t) - v0:  bu = (dot(cross(w, eb), ns) * sc) / nn, bv = (dot(cross(ea, w), ns) * sc) / nn,
//                    bu >= 0 and bv >= 0 and bu + bv <= 1
//   triangle         of the Tri48 record (v0 = p0, v1 = p0 + e0, v2 = p0 - e1, the triangle every other query sees):  0 if point_tri's
//                    d2 at q = o is <= r2.  Otherwise the least t <= tmax over the candidates, in this order with a strict <, so the first
//                    of equal candidates stays:  face;  edge(v0, ea), edge(v0, eb), edge(v1, v2 - v1);  vertex(v0), vertex(v1), vertex(v2).
//                    A zero-area triangle needs no special case: the face drops out (m = 0, or a normal of no meaning whose inside test
//                    still places the contact in the triangle's plane strip -- on the line -- at distance radius), edges of zero length
//                    drop out (den = 0), the vertices always remain.
//   sphere           0 if point_sphere's d2 at q = o is <= r2.  m = centre - o.  Outside (dot(m, m) > R * R): ball(m, d, dd, Rs * Rs) with
//                    Rs = R + radius.  Inside: Ri = R - radius, none unless Ri > 0; tca, perp as in ball, disc = Ri * Ri - dot(perp, perp),
//                    none unless disc >= 0; t = tca + sqrt(disc / dd), a negative t reads as 0.  Accepted when t <= tmax.
//   quad             the corners c_ab of pt_box.h box_quad; the triangles (p0, e0, e1) = (c00, c10 - c00, c00 - c11) and
//                    (c00, c11 - c00, c00 - c01) through the triangle function; the lesser, the first at equality.
// Why no NaN comes out of finite input: every candidate reaches the result through comparisons alone (disc >= 0, den > 0, A > 0, ga < 0,
// 0 <= s <= 1, the inside test, t <= tmax), all of which a NaN fails; a t that is accepted is 0 or a finite number <= tmax.  The record's
// p, u, v are point_tri's at q = o + d * t, finite with q: that is, wherever the sweep's end point o + d * tmax is finite.
//
// The walk.  One sweep per lane; a stack entry is a child reference and the entry time of its box; children are visited nearest entry
// first; a popped entry is tested again against the bound as it is then.  The node step runs the slab test of the ray o + d * t against
// each child's box grown on every side by
//     g = radius + kSweepMu * ((radius + max|o|) + bm),   bm = the largest |plane| of the child's box,   kSweepMu = 2^-15
// with the planes' times (plane -+ g - o) * inv, inv = 1 / d per axis, or -+FLT_MAX where that is not finite (an axis the ray does not
// move along: the origin's side of each plane decides, and 0 * inv is 0, not NaN).  tn = the largest of the three near times and 0,
// tf = the least of the far times; the child is entered iff tn <= tf and tn <= tbest * kSweepTimeSlack (2^-19 over 1).
// What must hold for "the result is a loop over all primitives, bit for bit": for every triangle under a box with a computed
// toi = t^ <= tbest, the box passes.
//   * Every accepted candidate puts c(t^) within radius + e of the triangle of the COMPUTED vertices: a vertex contact by its ball, an
//     edge contact because its computed parameter lies in [0, 1], a face contact because the inside test is evaluated at c(t^) itself.
//     At grazing incidence t^ is ill-conditioned but the distance is not: dist^2 - radius^2 at t^ is the error of dot(perp, perp), whose
//     size is 2 |perp| <= 2 radius times the error of perp, so dist - radius is the error of perp, a few ulps of what it was computed
//     from.  Those quantities -- a - o, d * tca, o + d * t^ and their parts along and across an edge -- are all bounded by
//     K = |o| + |a| + radius in magnitude (an accepted contact lies within radius of the triangle, so |d| t^ <= |a - o| + radius), and each
//     of at most ~20 roundings on the way contributes 2^-24 K: e < 2^-19 K.  K <= sqrt(3) ((radius + max|o|) + bm) for a vertex a under the box.
//   * The computed vertices v1, v2 lie within 1.2e-7 (|v| + scene extent) of the boxed ones and the builder pads every triangle's box by
//     1e-5 x the scene's largest extent + 1e-6 |v| per plane (pt_lbvh.h pad_lo / pad_hi, reproduced by the refit): the box contains the
//     computed triangle (the argument of pt_box.h).  Boxes only grow towards the root and into the 64-byte form.
//   * So c(t^) lies inside the box grown by radius + e.  The computed plane time fl(fl(plane' - o) * fl(1 / d)) is the exact time of a plane
//     moved by at most 3 x 2^-24 |plane' - o| < 2^-22 (K + g): the computed slabs are the exact slabs of a box that contains the box grown by
//     g - 2^-22 (K + g) > radius + e.  Hence tn <= t^ <= tf exactly, and t^ <= tbest: the child is entered whatever the slack, which only
//     covers the order of two roundings nobody has to trust.  kSweepMu carries a factor 8 over sqrt(3) (2^-19 + 2^-21).
// A wider margin costs time, never a bit.  Not covered: scenes below 1e-14 units (the point queries' bound: d2 and r2 go subnormal),
// |d| outside 1e-15 .. 1e15 (dd leaves binary32), sweeps whose end point o + d * tmax is not finite.
// Used by the sweep kernel (sweepkernel.hip) and by its CPU mirror (tests/sweepsim/sweepsim.cpp); nothing else includes it.
#pragma once
#include "pt_box.h"

namespace pt {

enum { SWEEP_CLOSEST = 0, SWEEP_ANY = 1 };

struct alignas(16) SweepHit { float t; int prim, mat; float u, v; float p[3]; };
static_assert(sizeof(SweepHit) == 32, "SweepHit is moptix_sweep_hit: two 16-byte stores");

constexpr float kSweepMu = 1.0f / 32768.0f;
constexpr float kSweepTimeSlack = 1.0f + 1.0f / 524288.0f;
constexpr float kSweepInvMax = 3.40282347e38f;

// The query as the walk holds it.
struct SweepQ {
  v3 o, d;
  float radius, tmax;
  float r2, dd;         // radius * radius, dot(d, d)
  v3 inv;               // sweep_inv of d's components
  float grow;           // radius + kSweepMu * (radius + max|o|): the part of a box's margin that does not depend on the box
};

// s: the query's eight floats.  false = an invalid query.
PT_HD bool sweep_valid(const float s[8]) {
  bool ok = true;
  for (int k = 0; k < 8; k++) ok = ok & point_finite(s[k]);
  ok = ok & ((s[3] != 0.0f) | (s[4] != 0.0f) | (s[5] != 0.0f));
  return ok & (s[6] > 0.0f) & (s[7] > 0.0f);
}

PT_HD float sweep_inv(float d) {
  const float inv = 1.0f / d;
  return point_finite(inv) ? inv : __builtin_copysignf(kSweepInvMax, d);
}

PT_HD void sweep_query(const float s[8], SweepQ& q) {
  q.o = mk3(s[0], s[1], s[2]); q.d = mk3(s[3], s[4], s[5]); q.radius = s[6]; q.tmax = s[7];
  q.r2 = q.radius * q.radius; q.dd = dot(q.d, q.d);
  q.inv = mk3(sweep_inv(q.d.x), sweep_inv(q.d.y), sweep_inv(q.d.z));
  const float om = box_max(box_max(__builtin_fabsf(q.o.x), __builtin_fabsf(q.o.y)), __builtin_fabsf(q.o.z));
  q.grow = q.radius + kSweepMu * (q.radius + om);
}

PT_HD v3 sweep_centre(const SweepQ& q, float t) { return q.o + q.d * t; }

PT_HD bool sweep_ball(v3 m, v3 e, float ee, float R2, float& t) {
  const float tca = dot(m, e) / ee;
  const v3 perp = m - e * tca;
  const float disc = R2 - dot(perp, perp);
  if (!(disc >= 0.0f)) return false;
  const float s = __builtin_sqrtf(disc / ee);
  t = tca - s;
  if (t < 0.0f) {
    if (!(tca + s >= 0.0f)) return false;
    t = 0.0f;
  }
  return true;
}

// m = a - o
PT_HD bool sweep_edge(v3 m, v3 ab, v3 d, float r2, float& t) {
  const float den = dot(ab, ab);
  if (!(den > 0.0f)) return false;
  const float dpar = dot(d, ab) / den, mpar = dot(m, ab) / den;
  const v3 dperp = d - ab * dpar, mperp = m - ab * mpar;
  const float A = dot(dperp, dperp);
  if (!(A > 0.0f)) return false;
  if (!sweep_ball(mperp, dperp, A, r2, t)) return false;
  const float s = dpar * t - mpar;
  return (s >= 0.0f) & (s <= 1.0f);
}

PT_HD bool sweep_face(const SweepQ& q, v3 p0, v3 ea, v3 eb, float& t) {
  const v3 n = cross(ea, eb);
  const float m = fmaxf_(fmaxf_(__builtin_fabsf(n.x), __builtin_fabsf(n.y)), __builtin_fabsf(n.z));
  if (!((m > 0.0f) & point_finite(m))) return false;
  const float sc = i2f(0x7f000000 - (f2i(m) & 0x7f800000));
  const v3 ns = n * sc;
  const float nn = dot(ns, ns);
  const float h = dot(ns, q.o - p0), g = dot(ns, q.d);
  const float rn = q.radius * __builtin_sqrtf(nn);
  const float ha = __builtin_fabsf(h), ga = h < 0.0f ? -g : g;
  t = 0.0f;
  if (ha > rn) {
    if (!(ga < 0.0f)) return false;
    t = (ha - rn) / -ga;
  }
  const v3 w = sweep_centre(q, t) - p0;
  const float bu = (dot(cross(w, eb), ns) * sc) / nn, bv = (dot(cross(ea, w), ns) * sc) / nn;
  return (bu >= 0.0f) & (bv >= 0.0f) & (bu + bv <= 1.0f);
}

// a candidate of the triangle: the least so far, the first of equals; best starts out as tmax, which counts
PT_HD void sweep_take(bool ok, float t, bool& hit, float& best) {
  if (ok & (hit ? t < best : t <= best)) { hit = true; best = t; }
}

// The triangle's time of contact.  false = none in [0, tmax].
PT_HD bool sweep_tri(const SweepQ& q, v3 p0, v3 e0, v3 e1, float& toi) {
  PointCand k;
  point_tri(q.o, p0, e0, e1, k);
  if (k.d2 <= q.r2) { toi = 0.0f; return true; }
  const v3 ea = e0, eb = -e1;
  const v3 v1 = p0 + e0, v2 = p0 - e1;
  const v3 m0 = p0 - q.o, m1 = v1 - q.o, m2 = v2 - q.o;
  bool hit = false;
  float best = q.tmax, t = 0.0f;
  bool ok = sweep_face(q, p0, ea, eb, t);
  sweep_take(ok, t, hit, best);
  ok = sweep_edge(m0, ea, q.d, q.r2, t);
  sweep_take(ok, t, hit, best);
  ok = sweep_edge(m0, eb, q.d, q.r2, t);
  sweep_take(ok, t, hit, best);
  ok = sweep_edge(m1, v2 - v1, q.d, q.r2, t);
  sweep_take(ok, t, hit, best);
  ok = sweep_ball(m0, q.d, q.dd, q.r2, t);
  sweep_take(ok, t, hit, best);
  ok = sweep_ball(m1, q.d, q.dd, q.r2, t);
  sweep_take(ok, t, hit, best);
  ok = sweep_ball(m2, q.d, q.dd, q.r2, t);
  sweep_take(ok, t, hit, best);
  toi = best;
  return hit;
}

PT_HD bool sweep_sphere(const SweepQ& q, v3 centre, float R, float& toi) {
  PointCand k;
  point_sphere(q.o, centre, R, k);
  if (k.d2 <= q.r2) { toi = 0.0f; return true; }
  const v3 m = centre - q.o;
  float t;
  if (dot(m, m) > R * R) {
    const float Rs = R + q.radius;
    if (!sweep_ball(m, q.d, q.dd, Rs * Rs, t)) return false;
  } else {
    const float Ri = R - q.radius;
    if (!(Ri > 0.0f)) return false;
    const float tca = dot(m, q.d) / q.dd;
    const v3 perp = m - q.d * tca;
    const float disc = Ri * Ri - dot(perp, perp);
    if (!(disc >= 0.0f)) return false;
    t = tca + __builtin_sqrtf(disc / q.dd);
    if (t < 0.0f) t = 0.0f;
  }
  if (!(t <= q.tmax)) return false;
  toi = t;
  return true;
}

PT_HD bool sweep_quad(const SweepQ& q, v3 v1, v3 v2, v3 anchor, float& toi) {
  const v3 E1 = v1 / dot(v1, v1), E2 = v2 / dot(v2, v2);
  const v3 c00 = box_quad_corner(anchor, E1, E2, 0.0f, 0.0f), c10 = box_quad_corner(anchor, E1, E2, 1.0f, 0.0f);
  const v3 c11 = box_quad_corner(anchor, E1, E2, 1.0f, 1.0f), c01 = box_quad_corner(anchor, E1, E2, 0.0f, 1.0f);
  float ta = 0.0f, tb = 0.0f;
  const bool a = sweep_tri(q, c00, c10 - c00, c00 - c11, ta);
  const bool b = sweep_tri(q, c00, c11 - c00, c00 - c01, tb);
  if (b & (!a | (tb < ta))) { toi = tb; return true; }
  toi = ta;
  return a;
}

// The acceptance rule on a toi already within [0, tmax]: the first contact wins; at exactly equal toi the lower primitive id.
PT_HD bool sweep_accept(float t, int prim, float tbest, int bestPrim) {
  return (bestPrim < 0) | (t < tbest) | ((t == tbest) & (prim < bestPrim));
}

struct SweepTrav {
  float tbest;        // closest: toi of the best primitive so far, tmax while there is none; any: tmax throughout
  int bestPrim;       // -1 = none
  int bestTri;        // the best triangle's record index (the record is fetched again for the result)
  int node, sp;
};

PT_HD bool sweep_pruned(float tn, float tbest) { return tn > tbest * kSweepTimeSlack; }

template <class Stack>
PT_HD void sweep_pop(SweepTrav& tv, Stack& st) {
  while (tv.sp > 0) {
    tv.sp--;
    int ref; float tn;
    st.load(tv.sp, ref, tn);
    if (!sweep_pruned(tn, tv.tbest)) { tv.node = ref; return; }
  }
  tv.node = kTravDone;
}

// Start of a query: the sphere and quad lists brute force in point_begin's order, then the set-up of the walk.
template <bool ANY>
PT_HD void sweep_begin(const SceneView& sc, const SweepQ& q, bool valid, SweepTrav& tv) {
  tv.tbest = q.tmax; tv.bestPrim = -1; tv.bestTri = -1; tv.sp = 0; tv.node = kTravDone;
  if (!valid) return;
  bool done = false;
  for (int i = 0; i < sc.nSpheres && !done; i++) {
    const DevSphere s = load_uniform(sc.spheres + i);
    float t;
    if (sweep_sphere(q, s.center, s.radius, t) && sweep_accept(t, i, tv.tbest, tv.bestPrim)) { tv.bestPrim = i; if (ANY) done = true; else tv.tbest = t; }
  }
  for (int i = 0; i < sc.nQuads && !done; i++) {
    const DevQuad g = load_uniform(sc.quads + i);
    float t;
    if (sweep_quad(q, g.v1, g.v2, g.anchor, t) && sweep_accept(t, sc.nSpheres + i, tv.tbest, tv.bestPrim)) {
      tv.bestPrim = sc.nSpheres + i; if (ANY) done = true; else tv.tbest = t;
    }
  }
  tv.node = (done || sc.rootRef == kEmptyRef) ? kTravDone : sc.rootRef;
}

// The entry time of the ray into a child's box grown by g, or a negative number where it misses the grown box.
PT_HD float sweep_slab(const SweepQ& q, float lox, float loy, float loz, float hix, float hiy, float hiz) {
  const float bm = box_max(box_max(box_max(__builtin_fabsf(lox), __builtin_fabsf(hix)), box_max(__builtin_fabsf(loy), __builtin_fabsf(hiy))),
                           box_max(__builtin_fabsf(loz), __builtin_fabsf(hiz)));
  const float g = q.grow + kSweepMu * bm;
  const float x0 = ((lox - g) - q.o.x) * q.inv.x, x1 = ((hix + g) - q.o.x) * q.inv.x;
  const float y0 = ((loy - g) - q.o.y) * q.inv.y, y1 = ((hiy + g) - q.o.y) * q.inv.y;
  const float z0 = ((loz - g) - q.o.z) * q.inv.z, z1 = ((hiz + g) - q.o.z) * q.inv.z;
  float tn = fmaxf_(fmaxf_(fminf_(x0, x1), fminf_(y0, y1)), fminf_(z0, z1));
  const float tf = fminf_(fminf_(fmaxf_(x0, x1), fmaxf_(y0, y1)), fmaxf_(z0, z1));
  tn = tn > 0.0f ? tn : 0.0f;
  return tn <= tf ? tn : -1.0f;
}

// One four-child node for a lane with tv.node >= 0: the child entered first is visited next, the others are pushed last to first with
// their entry times beside them.  N64: the boxes come from the 64-byte node (pt_lbvh.h node64_plane), which contain the 128-byte node's.
template <bool N64, class Stack>
PT_HD void sweep_node_step(const SceneView& sc, const SweepQ& q, SweepTrav& tv, Stack& st) {
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
  unsigned long long k[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int c = 0; c < 4; c++) {
    const float tn = sweep_slab(q, lo[0][c], lo[1][c], lo[2][c], hi[0][c], hi[1][c], hi[2][c]);
    const bool in = (ref[c] != kEmptyRef) & (tn >= 0.0f) & !sweep_pruned(tn, tv.tbest);
    k[c] = in ? (((unsigned long long)(uint32_t)f2i(tn) << 32) | (unsigned)c) : kPointFar;
  }
  point_order(k[0], k[1]); point_order(k[2], k[3]); point_order(k[0], k[2]); point_order(k[1], k[3]); point_order(k[1], k[2]);
  if (k[0] == kPointFar) { sweep_pop(tv, st); return; }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 3; j >= 1; j--)
    if (k[j] != kPointFar) {
      const int c = (int)(k[j] & 3u);
      st.store(tv.sp, c == 0 ? ref[0] : c == 1 ? ref[1] : c == 2 ? ref[2] : ref[3], i2f((int32_t)(k[j] >> 32)));
      tv.sp++;
    }
  const int c0 = (int)(k[0] & 3u);
  tv.node = c0 == 0 ? ref[0] : c0 == 1 ? ref[1] : c0 == 2 ? ref[2] : ref[3];
}

PT_HD v3 sweep_pick(const v3 (&a)[4], int j) {
  return mk3(j == 0 ? a[0].x : j == 1 ? a[1].x : j == 2 ? a[2].x : a[3].x, j == 0 ? a[0].y : j == 1 ? a[1].y : j == 2 ? a[2].y : a[3].y,
             j == 0 ? a[0].z : j == 1 ? a[1].z : j == 2 ? a[2].z : a[3].z);
}

// One leaf for a lane with tv.node < 0 (and != kTravDone): the records are fetched as the point walk fetches them.
template <bool ANY, class Stack>
PT_HD void sweep_leaf_step(const SceneView& sc, const SweepQ& q, SweepTrav& tv, Stack& st) {
  const int first = leaf_first(tv.node), count = leaf_count(tv.node);
  const int triBase = sc.nSpheres + sc.nQuads;
  bool done = false;
  for (int base = 0; base < count && !done; base += 4) {
    LeafChunk ch;
    leaf_fetch4(sc, tv.node, base, ch);
    // One copy of the triangle function, not four: the slot is picked by selects on the loop counter, so the chunk stays in registers.
    for (int j = 0; j < 4; j++) {
      if (base + j < count && !done) {
        const v3 p0 = sweep_pick(ch.p0, j), e0 = sweep_pick(ch.e0, j), e1 = sweep_pick(ch.e1, j);
        const int prim = triBase + (j == 0 ? ch.prim[0] : j == 1 ? ch.prim[1] : j == 2 ? ch.prim[2] : ch.prim[3]);
        float t;
        if (sweep_tri(q, p0, e0, e1, t) && sweep_accept(t, prim, tv.tbest, tv.bestPrim)) {
          tv.bestPrim = prim; tv.bestTri = first + base + j;
          if (ANY) done = true; else tv.tbest = t;
        }
      }
    }
  }
  if (done) tv.node = kTravDone;
  else sweep_pop(tv, st);
}

// One traversal step for a lane with tv.node != kTravDone (if-if form, as point_step).
template <bool ANY, bool N64, class Stack>
PT_HD void sweep_step(const SceneView& sc, const SweepQ& q, SweepTrav& tv, Stack& st) {
  if (tv.node >= 0) sweep_node_step<N64>(sc, q, tv, st);
  else sweep_leaf_step<ANY>(sc, q, tv, st);
}

// The finished closest sweep's record: the winner's closest-point function at the centre of contact.
PT_HD void sweep_hit(const SceneView& sc, const SweepQ& q, const SweepTrav& tv, SweepHit& h) {
  h.t = q.tmax; h.prim = -1; h.mat = -1; h.u = 0.f; h.v = 0.f; h.p[0] = 0.f; h.p[1] = 0.f; h.p[2] = 0.f;
  if (tv.bestPrim < 0) return;
  const v3 c = sweep_centre(q, tv.tbest);
  PointCand k;
  if (tv.bestPrim < sc.nSpheres) {
    const DevSphere s = sc.spheres[tv.bestPrim];
    point_sphere(c, s.center, s.radius, k);
    h.mat = sc.sphereMat[tv.bestPrim];
  } else if (tv.bestPrim < sc.nSpheres + sc.nQuads) {
    const DevQuad* g = sc.quads + (tv.bestPrim - sc.nSpheres);
    point_quad(c, g->v1, g->v2, g->anchor, k);
    h.mat = g->mat;
  } else {
    const Tri48 t = load_const(at32(sc.tris, tv.bestTri));
    point_tri(c, t.p0, t.e0, t.e1, k);
    h.mat = t.mat;
  }
  h.t = tv.tbest; h.prim = tv.bestPrim; h.u = k.u; h.v = k.v;
  h.p[0] = k.c.x; h.p[1] = k.c.y; h.p[2] = k.c.z;
}

}  // namespace pt
