// pt_point.h -- closest-point queries against the built scene: the nearest surface point to q (include/moptix.h "point queries").
//
// A query is four floats  x y z maxDist;  r2 = maxDist * maxDist (one multiply; +inf = no limit).
//   closest   the primitive least by (d2, primitive id) among those with d2 < r2, d2 = the per-primitive function below; at exactly equal
//             d2 the lower id (rule D5).  The answer is a function of q and the device records alone: tree, leaf size, builder, node
//             format, grid size and scheduling play no part.  Every primitive counts, whatever its material.
//   any       1 iff the closest query on the same point reports a primitive; the walk stops at the first primitive it accepts.
//   invalid   x, y or z non-finite, maxDist NaN or maxDist <= 0: a miss, decided before any traversal.
//
// The per-primitive functions, every operation in order (pt_math.h: AC1 dot, AC2 cross, AC3 v / s = v * (1 / s), AC4 no contraction; division
// and square root correctly rounded).  Each returns the nearest point c of the primitive, its parameters and d2 = dot(q - c, q - c).
//   clamp01(x)       x > 0 ? (x < 1 ? x : 1) : 0, by comparisons and selects: -0 and NaN (inf / inf after an overflow) become +0.  Not
//                    fmin / fmax: which zero max(+0, -0) returns is the one thing the host's and the device's differ in, and the sign
//                    would show in u, v and p
//   segment(a, ab)   den = dot(ab, ab);  t = den > 0 ? clamp01(dot(q - a, ab) / den) : 0;  c = a + ab * t
//   triangle         of the Tri48 record: v0 = p0, v1 = p0 + e0, v2 = p0 - e1, the triangle the ray test sees.  The minimum over up to four
//                    candidates, taken in this order with a strict <, so the first of equal candidates stays:
//                      1  segment(v0, e0)            (u, v) = (t, 0)
//                      2  segment(v0, -e1)           (u, v) = (0, t)
//                      3  segment(v1, v2 - v1)       (u, v) = (1 - t, t)
//                      4  the plane projection.  ea = e0, eb = -e1, n = cross(ea, eb), m = the largest |component| of n; it applies when
//                         m > 0 and finite.  sc = 2^-floor(log2 m) (exact, from m's exponent bits), ns = n * sc (largest component in
//                         [1, 2)), nn = dot(ns, ns), w = q - v0, bu = (dot(cross(w, eb), ns) * sc) / nn, bv = (dot(cross(ea, w), ns) * sc) / nn
//                         -- the barycentrics of step 2 of moptix_denoise_temporal, with the normal scaled by a power of two first:
//                         dot(n, n) itself is a fourth power of the edge length and leaves binary32 for edges beyond 4e9 or below 1e-10
//                         units.  Inside when bu >= 0 and bv >= 0 and bu + bv <= 1 (any NaN fails);  c = (v0 + ea * bu) + eb * bv,
//                         (u, v) = (bu, bv)
//                    A zero-area triangle needs no special case: collinear vertices give m = 0 or barycentrics of no meaning whose point
//                    still lies on the line, and the three segments' minimum is the distance to their union, the longest segment;
//                    coincident vertices give den = 0 three times, t = 0, the point v0.  No NaN comes out of finite input.
//   sphere           the surface: w = q - centre, l2 = dot(w, w), dir = l2 > 0 ? w * (1 / sqrt(l2)) : (1, 0, 0), c = centre + dir * radius
//   quad             quad_test's parametrisation: w = q - anchor, a1 = clamp01(dot(v1, w)), a2 = clamp01(dot(v2, w)),
//                    E1 = v1 / dot(v1, v1), E2 = v2 / dot(v2, v2) (the edges setQuadParams inverted), c = (anchor + E1 * a1) + E2 * a2
//
// The traversal is ordered by the squared distance from q to a child's box and pruned by the best d2 so far (point_node_step); it is used
// by the point kernel (pointkernel.hip) and by its CPU mirror (tests/hostsim/pointsim.cpp); nothing of the render path includes it.
#pragma once
#include "pt_path.h"
#include "pt_lbvh.h"

namespace pt {

enum { POINT_CLOSEST = 0, POINT_ANY = 1 };

struct alignas(16) PointHit { float dist; int prim, mat; float u, v; float p[3]; };
static_assert(sizeof(PointHit) == 32, "PointHit is moptix_point_hit: two 16-byte stores");

struct PointCand { float d2; v3 c; float u, v; };

PT_HD bool point_finite(float x) { return (f2i(x) & 0x7f800000) != 0x7f800000; }
PT_HD float point_d2(v3 q, v3 c) { const v3 d = q - c; return dot(d, d); }

PT_HD float point_clamp01(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }

PT_HD float point_segment(v3 q, v3 a, v3 ab, v3& c) {
  const float den = dot(ab, ab);
  const float t = den > 0.0f ? point_clamp01(dot(q - a, ab) / den) : 0.0f;
  c = a + ab * t;
  return t;
}

PT_HD void point_tri(v3 q, v3 p0, v3 e0, v3 e1, PointCand& best) {
  const v3 ea = e0, eb = -e1;
  const v3 v1 = p0 + e0, v2 = p0 - e1;
  v3 c;
  float t = point_segment(q, p0, ea, c);
  best.d2 = point_d2(q, c); best.c = c; best.u = t; best.v = 0.0f;
  t = point_segment(q, p0, eb, c);
  float d2 = point_d2(q, c);
  if (d2 < best.d2) { best.d2 = d2; best.c = c; best.u = 0.0f; best.v = t; }
  t = point_segment(q, v1, v2 - v1, c);
  d2 = point_d2(q, c);
  if (d2 < best.d2) { best.d2 = d2; best.c = c; best.u = 1.0f - t; best.v = t; }
  const v3 n = cross(ea, eb);
  const float m = fmaxf_(fmaxf_(__builtin_fabsf(n.x), __builtin_fabsf(n.y)), __builtin_fabsf(n.z));
  if ((m > 0.0f) & point_finite(m)) {
    const float sc = i2f(0x7f000000 - (f2i(m) & 0x7f800000));      // 2^-floor(log2 m), exact (2^127 for a subnormal m)
    const v3 ns = n * sc;                                           // the normal with its largest component in [1, 2)
    const float nn = dot(ns, ns);
    const v3 w = q - p0;
    const float bu = (dot(cross(w, eb), ns) * sc) / nn, bv = (dot(cross(ea, w), ns) * sc) / nn;
    if ((bu >= 0.0f) & (bv >= 0.0f) & (bu + bv <= 1.0f)) {
      c = (p0 + ea * bu) + eb * bv;
      d2 = point_d2(q, c);
      if (d2 < best.d2) { best.d2 = d2; best.c = c; best.u = bu; best.v = bv; }
    }
  }
}

PT_HD void point_sphere(v3 q, v3 center, float radius, PointCand& out) {
  const v3 w = q - center;
  const float l2 = dot(w, w);
  const v3 dir = l2 > 0.0f ? w * (1.0f / __builtin_sqrtf(l2)) : mk3(1.0f, 0.0f, 0.0f);
  out.c = center + dir * radius;
  out.d2 = point_d2(q, out.c); out.u = 0.0f; out.v = 0.0f;
}

PT_HD void point_quad(v3 q, v3 v1, v3 v2, v3 anchor, PointCand& out) {
  const v3 w = q - anchor;
  const float a1 = point_clamp01(dot(v1, w)), a2 = point_clamp01(dot(v2, w));
  const v3 E1 = v1 / dot(v1, v1), E2 = v2 / dot(v2, v2);
  out.c = (anchor + E1 * a1) + E2 * a2;
  out.d2 = point_d2(q, out.c); out.u = a1; out.v = a2;
}

// The acceptance rule: d2 inside the current bound wins; at exactly equal d2 the lower primitive id wins (bestPrim < 0: the bound is
// still r2 itself, which is exclusive).
PT_HD bool point_accept(float d2, int prim, float bestD2, int bestPrim) {
  return (d2 < bestD2) | ((d2 == bestD2) & (bestPrim >= 0) & (prim < bestPrim));
}

// p: the query's four floats.  false = an invalid query.
PT_HD bool point_valid(const float p[4]) {
  bool ok = p[3] > 0.0f;                                  // NaN > 0 is false; +inf passes
  for (int k = 0; k < 3; k++) ok = ok & point_finite(p[k]);
  return ok;
}

struct PointTrav {
  float bestD2;       // closest: d2 of the best primitive so far, r2 while there is none; any: r2 throughout
  int bestPrim;       // -1 = none
  int bestTri;        // the best triangle's record index (the record is fetched again for the result)
  int node, sp;
};

// The prune.  A child box is dropped when  boxD2 > bestD2 * kPointPruneSlack  (strictly: at an equal distance a lower primitive id may
// hide), a popped entry likewise.  What must hold for "the result is a loop over all primitives, bit for bit": for every triangle under a
// box, computed boxD2 <= computed d2(q, triangle), up to the slack.
//   * Near the surface the errors are absolute.  The computed nearest point is within a few ulps of |v| of the triangle (v1 = p0 + e0 and
//     v2 = p0 - e1 are each one rounding away from the vertices the builder boxed; the candidate is a convex combination evaluated in three
//     roundings): below 5e-7 |v|.  Every triangle box is padded by padAbs + 1e-6 |v| per plane (pt_lbvh.h pad_lo / pad_hi, reproduced by the
//     refit; padAbs = 1e-5 x the scene's largest extent + 1e-30), and boxes only grow towards the root and into the 64-byte form.  So per axis
//     |q - c| exceeds the distance from q to the box by more than half the padding, wherever that distance is not 0.
//   * Far from the surface the errors are relative: boxD2 and d2 are each three subtractions, three squares and two sums, below 5 ulps
//     apart from their exact values, and the padding (absolute) stops paying for that once q is some fifty scene extents away.  Hence
//     the slack, 2^-19 (32 ulps) on bestD2 in the prune comparison only -- never in point_accept.  A wider margin costs time, never a bit.
// Not covered: scenes smaller than 1e-14 units, where d2 is subnormal and neither argument holds.
constexpr float kPointPruneSlack = 1.0f + 1.0f / 524288.0f;
PT_HD bool point_pruned(float boxD2, float bestD2) { return boxD2 > bestD2 * kPointPruneSlack; }

PT_HD float point_box_d2(v3 q, float lox, float loy, float loz, float hix, float hiy, float hiz) {
  const v3 d = mk3(fmaxf_(fmaxf_(lox - q.x, q.x - hix), 0.0f), fmaxf_(fmaxf_(loy - q.y, q.y - hiy), 0.0f), fmaxf_(fmaxf_(loz - q.z, q.z - hiz), 0.0f));
  return dot(d, d);
}

template <class Stack>
PT_HD void point_pop(PointTrav& tv, Stack& st) {
  while (tv.sp > 0) {
    tv.sp--;
    int ref; float d2;
    st.load(tv.sp, ref, d2);
    if (!point_pruned(d2, tv.bestD2)) { tv.node = ref; return; }      // re-tested against the bound as it is now, before any fetch
  }
  tv.node = kTravDone;
}

// Start of a query: the sphere and quad lists brute force, then the set-up of the walk.
template <bool ANY>
PT_HD void point_begin(const SceneView& sc, v3 q, float r2, bool valid, PointTrav& tv) {
  tv.bestD2 = r2; tv.bestPrim = -1; tv.bestTri = -1; tv.sp = 0; tv.node = kTravDone;
  if (!valid) return;
  bool done = false;
  for (int i = 0; i < sc.nSpheres && !done; i++) {
    const DevSphere s = load_uniform(sc.spheres + i);
    PointCand k;
    point_sphere(q, s.center, s.radius, k);
    if (point_accept(k.d2, i, tv.bestD2, tv.bestPrim)) { tv.bestPrim = i; if (ANY) done = true; else tv.bestD2 = k.d2; }
  }
  for (int i = 0; i < sc.nQuads && !done; i++) {
    const DevQuad g = load_uniform(sc.quads + i);
    PointCand k;
    point_quad(q, g.v1, g.v2, g.anchor, k);
    if (point_accept(k.d2, sc.nSpheres + i, tv.bestD2, tv.bestPrim)) { tv.bestPrim = sc.nSpheres + i; if (ANY) done = true; else tv.bestD2 = k.d2; }
  }
  tv.node = (done || sc.rootRef == kEmptyRef) ? kTravDone : sc.rootRef;
}

// A child of the node step: the box distance's bits above the child slot (a non-negative float's bits order like the float), so that
// sorting the keys orders by distance and breaks ties by slot; kPointFar = not entered.
constexpr unsigned long long kPointFar = ~0ull;
PT_HD void point_order(unsigned long long& a, unsigned long long& b) { if (b < a) { const unsigned long long x = a; a = b; b = x; } }

// One four-child node for a lane with tv.node >= 0: the nearest surviving child is visited next, the others are pushed far to near with
// their box distances beside them.  N64: the boxes come from the 64-byte node (plane = fma(q, step, corner), pt_lbvh.h node64_plane), which
// contain the 128-byte node's: lower bounds only get smaller, so more boxes are entered and no result changes.
template <bool N64, class Stack>
PT_HD void point_node_step(const SceneView& sc, v3 q, PointTrav& tv, Stack& st) {
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
    const float bd = point_box_d2(q, lo[0][c], lo[1][c], lo[2][c], hi[0][c], hi[1][c], hi[2][c]);
    const bool in = (ref[c] != kEmptyRef) & !point_pruned(bd, tv.bestD2);
    k[c] = in ? (((unsigned long long)(uint32_t)f2i(bd) << 32) | (unsigned)c) : kPointFar;
  }
  point_order(k[0], k[1]); point_order(k[2], k[3]); point_order(k[0], k[2]); point_order(k[1], k[3]); point_order(k[1], k[2]);
  if (k[0] == kPointFar) { point_pop(tv, st); return; }
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

// One leaf for a lane with tv.node < 0 (and != kTravDone): the records are fetched as the ray traversal fetches them.
template <bool ANY, class Stack>
PT_HD void point_leaf_step(const SceneView& sc, v3 q, PointTrav& tv, Stack& st) {
  const int first = leaf_first(tv.node), count = leaf_count(tv.node);
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
        PointCand k;
        point_tri(q, ch.p0[j], ch.e0[j], ch.e1[j], k);
        if (point_accept(k.d2, triBase + ch.prim[j], tv.bestD2, tv.bestPrim)) {
          tv.bestPrim = triBase + ch.prim[j]; tv.bestTri = first + base + j;
          if (ANY) done = true; else tv.bestD2 = k.d2;
        }
      }
    }
  }
  if (done) tv.node = kTravDone;
  else point_pop(tv, st);
}

// One traversal step for a lane with tv.node != kTravDone.
template <bool ANY, bool N64, class Stack>
PT_HD void point_step(const SceneView& sc, v3 q, PointTrav& tv, Stack& st) {
  if (tv.node >= 0) point_node_step<N64>(sc, q, tv, st);
  else point_leaf_step<ANY>(sc, q, tv, st);
}

// The finished closest query's record: the winner's function is evaluated once more for its point and parameters (the same operations on
// the same record, so the same d2).
PT_HD void point_hit(const SceneView& sc, v3 q, float maxDist, const PointTrav& tv, PointHit& h) {
  h.dist = maxDist; h.prim = -1; h.mat = -1; h.u = 0.f; h.v = 0.f; h.p[0] = 0.f; h.p[1] = 0.f; h.p[2] = 0.f;
  if (tv.bestPrim < 0) return;
  PointCand k;
  if (tv.bestPrim < sc.nSpheres) {
    const DevSphere s = sc.spheres[tv.bestPrim];
    point_sphere(q, s.center, s.radius, k);
    h.mat = sc.sphereMat[tv.bestPrim];
  } else if (tv.bestPrim < sc.nSpheres + sc.nQuads) {
    const DevQuad* g = sc.quads + (tv.bestPrim - sc.nSpheres);
    point_quad(q, g->v1, g->v2, g->anchor, k);
    h.mat = g->mat;
  } else {
    const Tri48 t = load_const(at32(sc.tris, tv.bestTri));
    point_tri(q, t.p0, t.e0, t.e1, k);
    h.mat = t.mat;
  }
  h.dist = __builtin_sqrtf(tv.bestD2); h.prim = tv.bestPrim; h.u = k.u; h.v = k.v;
  h.p[0] = k.c.x; h.p[1] = k.c.y; h.p[2] = k.c.z;
}

}  // namespace pt
