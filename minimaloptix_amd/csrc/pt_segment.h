// pt_segment.h -- segment queries against the built scene: the nearest surface point to a segment (include/moptix.h "segment queries").
//
// A query is eight floats  ax ay az bx by bz maxDist pad;  pad is ignored;  r2 = maxDist * maxDist (one multiply; +inf = no limit).
//   closest   the primitive least by (d2, primitive id) among those with d2 < r2, d2 = the per-primitive function below; at exactly equal
//             d2 the lower id (rule D5).  The answer is a function of the query and the device records alone: tree, leaf size, builder,
//             node format, grid size and scheduling play no part.  Every primitive counts, whatever its material.
//   any       1 iff the closest query on the same segment reports a primitive; the walk stops at the first primitive it accepts.
//   invalid   any of the six coordinates non-finite, maxDist NaN or maxDist <= 0: a miss, decided before any traversal.
// The record: dist = sqrt(d2), s in [0, 1] the parameter of the nearest point a + (b - a) * s ON THE SEGMENT, p the nearest point ON THE
// PRIMITIVE, feature the candidate that won (below).  A miss: dist = maxDist as given, prim = mat = -1, the rest 0.
//
// The per-primitive functions, every operation in order (pt_math.h: AC1 dot, AC2 cross, AC3 v / s = v * (1 / s), AC4 no contraction; division
// and square root correctly rounded).  ab = b - a, once per query; clamp01, point_d2, point_tri, point_sphere are pt_point.h's.
//   segseg(a, ab, c, e)   the closest pair between the segments a + ab * s and c + e * t, s and t in [0, 1]:
//                    r = a - c;  A = dot(ab, ab);  E = dot(e, e);  F = dot(e, r).
//                      A <= 0 and E <= 0 (both of zero length; "<= 0" is "not > 0" throughout):  s = 0, t = 0
//                      A <= 0:                  s = 0;  t = clamp01(F / E)
//                      otherwise C = dot(ab, r), and
//                        E <= 0:                t = 0;  s = clamp01(-C / A)
//                        otherwise B = dot(ab, e);  den = A * E - B * B;  s = den > 0 ? clamp01((B * F - C * E) / den) : 0;  tn = B * s + F;
//                                  tn < 0:      t = 0;  s = clamp01(-C / A)
//                                  tn > E:      t = 1;  s = clamp01((B - C) / A)
//                                  otherwise    t = clamp01(tn / E)
//                    x = a + ab * s;  y = c + e * t;  d2 = point_d2(x, y).  Only clamp01 and comparisons decide: clamp01 maps NaN and -0 to +0
//                    and a NaN fails every comparison, so s and t are numbers in [0, 1] whatever overflowed on the way.
//   triangle         of the Tri48 record: v0 = p0, v1 = p0 + e0, v2 = p0 - e1, ea = e0, eb = -e1 -- what point_tri sees.  The minimum over six
//                    candidates, taken in this order with a strict <, so the first of equal candidates stays:
//                      0  point_tri(a, ...)                       s = 0, p its point                        feature 0 (end a)
//                      1  point_tri(b, ...), b as given           s = 1                                      feature 1 (end b)
//                      2  segseg(a, ab, v0, ea)                   s, p = y                                   feature 2 (edge 0)
//                      3  segseg(a, ab, v0, eb)                                                              feature 3 (edge 1)
//                      4  segseg(a, ab, v1, v2 - v1)                                                         feature 4 (edge 2)
//                      5  the crossing: tri_test(a, ab, 0, 1, p0, e0, e1, ...) (pt_geom.h, the ray queries' own test) accepts at t:
//                         d2 = 0, s = t, p = a + ab * t                                                      feature 5
//                    so "distance 0" is "the closest ray query on (a, b - a, 0, 1) can report this triangle".
//                    A zero-length segment (a == b, so ab = 0 exactly) returns point_tri(a)'s d2 and point bit for bit: candidate 1 is
//                    candidate 0 again; A = 0 in 2-4, whose s = 0, x = a + 0 and t = clamp01(dot(e, a - c) / dot(e, e)) are point_segment's
//                    own operations on the same edges in the same order, so each can only tie with candidate 0, which is their minimum
//                    or less; candidate 5 sees 1 / dot(n, 0) = inf and cross(0, inf) = NaN, which fails tri_test's comparisons.
//                    A zero-area triangle needs no special case: point_tri needs none, segseg handles zero-length edges (E <= 0) and
//                    parallel ones (den <= 0) in branches of their own, and tri_test's 1 / 0 fails its comparisons as above.
//   sphere           the surface.  m = centre - a;  A = dot(ab, ab);  tca = dot(m, ab) / A;  sc = A > 0 ? clamp01(tca) : 0;  x = a + ab * sc, the
//                    segment's point nearest the centre;  lx = point_d2(x, centre), la = point_d2(a, centre), lb = point_d2(b, centre),
//                    R2 = R * R.
//                      lx > R2                  outside:  point_sphere(x, ...);  s = sc;  feature 0 (sc == 0), 1 (sc == 1), 2 (the foot of the
//                                               perpendicular inside the segment)
//                      la < R2 and lb < R2      inside:  point_sphere at the end further from the centre (b if lb > la, else a);  s = 0 or 1;
//                                               feature 0 or 1
//                      otherwise                the segment meets the surface:  d2 = 0, at the first root of the quadratic solved about the
//                                               foot of the perpendicular (pt_sweep.h ball):  perp = m - ab * tca;
//                                               disc = R2 - dot(perp, perp), a negative or NaN disc reads as 0;  h = sqrt(disc / A);
//                                               t = la > R2 ? tca - h : la < R2 ? tca + h : 0 (a outside: the way in; a inside: the
//                                               way out; a on the surface: a);  s = A > 0 ? clamp01(t) : 0;  p = a + ab * s;  feature 5
//                    For a == b this is point_sphere(a) unless a lies on the sphere to the bit (la == R2).
//   quad             the corners c_ab of pt_box.h box_quad; the triangles (p0, e0, e1) = (c00, c10 - c00, c00 - c11) and
//                    (c00, c11 - c00, c00 - c01) through the triangle function; the lesser d2, the first at equality.  feature 0, 1 and 5 as
//                    for a triangle; 2-4 the edges of the first triangle, 6-8 the edges of the second (its 2-4 plus 4; 6 cannot win: the
//                    diagonal is the first triangle's edge 1 on the same operands, and the first of equals stays).  (The point
//                    queries measure a quad by point_quad's clamped coordinates: on a quad a zero-length segment is not the point query.)
// Acceptance is point_accept.
//
// The walk is the point walk (pt_point.h) with the segment in place of q: a stack of (reference, lower bound), children visited nearest
// first, a popped entry tested again against the bound as it then is.  The lower bound of a child is the squared distance between its box
// and the segment's own axis-aligned box, grown once per query on every side by
//     g = kSegmentMu * M,   M = the largest |coordinate| of a and b,   kSegmentMu = 2^-21:
// per axis  gap = max(lo - (max(a, b) + g), (min(a, b) - g) - hi, 0),  bound = dot(gap, gap);  the prune is point_pruned, slack included.
// What must hold for "the result is a loop over all primitives, bit for bit": for every triangle under a box, computed bound <= computed
// d2 of the triangle, up to the slack.
//   * The new fact: every d2 is point_d2(x, y) with x = a + ab * s COMPUTED, and a + (b - a) * 1 != b in general: x can leave the segment's
//     box.  By how much: fl(b - a) is off by 2^-24 x 2M, the product with s <= 1 by another 2^-24 x 2M, the sum by 2^-24 x M (1 + 2^-22):
//     below 5.1 x 2^-24 M per axis.  The grown planes are themselves one rounding each, 2^-24 M (1 + 2^-21).  6.2 x 2^-24 < 2^-21: x lies
//     inside the grown box G, exactly.  (Candidates 0, 1 use a and b as given, the crossing has d2 = 0 and is dealt with below.)  This is
//     the wider margin, and it is in the prune alone: near the surface the builder's padding (1e-5 scene extents) would pay for the
//     excursion only while M stays below some twenty scene extents, far away the slack only while the distance is a quarter of M or more,
//     and a long segment with one far end and its nearest point at the surface is inside neither.  g costs boxes entered, never a bit.
//     For a == b the bound is point_box_d2 of a box of half-width g about a, not of a itself: a zero-length segment's walk enters a few
//     more boxes than the point walk does, and returns the same bits.
//   * With x in G the rest is pt_point.h's argument with x for q: the per-axis gap between G and a box is at most that between x and the
//     box; y is a convex combination of the computed vertices evaluated in three roundings (point_tri's own point for candidates 0, 1),
//     within 5e-7 |v| of the triangle the builder boxed, and every triangle box is padded by padAbs + 1e-6 |v| per plane (pt_lbvh.h
//     pad_lo / pad_hi, reproduced by the refit: the argument holds for a refitted tree as it does for a built one), boxes only grow
//     towards the root and into the 64-byte form (node64_plane rounds outwards): per axis |x - y| exceeds the gap by more than half the
//     padding wherever the gap is not 0.  Far from the surface bound and d2 are each three subtractions, three squares and two sums,
//     below 5 ulps apart from their exact values: kPointPruneSlack (32 ulps), in the prune comparison only.
//   * The crossing.  tri_test accepts with 0 < t < 1 and barycentrics in [0, 1]: the ray (a, ab) over (0, 1) is one the ray queries' walk
//     follows into every box above this triangle (pt_path.h: the slab test's error is far inside the padding), so the segment passes
//     through the box, its own box overlaps it on every axis, and the signs of lo - hi' and lo' - hi are exact: gap = 0, bound = 0, and
//     0 > bestD2 * slack never holds.  A crossing is as well covered as a ray hit is, no better.
//     How good that is, in one number: tri_test decides from t = dot(n, p0 - a) / dot(n, ab) and two barycentrics of the same form, and
//     each numerator and denominator carries rounding noise of at most  nu = 2^-19 (|ab| + max|v - a|)  in space (some ten roundings of
//     2^-24 relative each on products of those lengths; 2^-19 leaves a factor 3).  A segment further than nu from the triangle's plane at
//     its nearer end, and not straddling it, is never given a crossing.  One that comes within nu of the plane meets it at a point
//     known to  nu / sin(angle between segment and plane)  only: a crossing may be reported, or missed, for a meeting point that far
//     outside or inside the triangle's outline, and dist is off by up to as much -- a micro-unit at a steep angle, 2^-10 (|ab| + max|v - a|)
//     at 0.1 degree.  For a segment IN the plane (sin = 0) the test divides noise by noise: any triangle of that plane may be reported as
//     crossed, dist = 0 with feature 5, however far beside the segment it lies, and the walk, which prunes by distance, may or may not
//     reach it -- there the answer can depend on the tree.  tests/test_segment_cpu.py asserts exactly this bound against binary64, row
//     by row, and "the true distance or a crossing" in the plane; profiles/r34_segment.txt section 3 has the figures.
// Not covered: scenes smaller than 1e-14 units (d2 subnormal, the point queries' bound), coordinates beyond 1e18 (A, E and den leave
// binary32: segseg still returns numbers in [0, 1] and no NaN, but the walk's argument no longer holds), and segments in the plane of a
// triangle or quad, as above: a caller who feeds edges of a flat region (edge_proximity on a planar patch) should lift them off the
// plane by more than nu, or ignore feature 5 on primitives the edge is coplanar with.
// Used by the segment kernel (segmentkernel.hip) and by its CPU mirror (tests/segmentsim/segmentsim.cpp); nothing else includes it.
#pragma once
#include "pt_sweep.h"

// The node step's second test (below, segment_slab_miss).  1: on; 0: the interval-box bound alone, the walk profiles/r34_segment.txt
// section 4 times it against.
#ifndef PT_SEGMENT_SLAB
#define PT_SEGMENT_SLAB 1
#endif

namespace pt {

enum { SEGMENT_CLOSEST = 0, SEGMENT_ANY = 1 };
enum { SEG_END_A = 0, SEG_END_B = 1, SEG_EDGE0 = 2, SEG_EDGE1 = 3, SEG_EDGE2 = 4, SEG_CROSSING = 5, SEG_QUAD_SECOND = 4 };

struct alignas(16) SegmentHit { float dist; int prim, mat; float s; float p[3]; int feature; };
static_assert(sizeof(SegmentHit) == 32, "SegmentHit is moptix_segment_hit: two 16-byte stores");

constexpr float kSegmentMu = 1.0f / 2097152.0f;

// The query as the walk holds it.
struct SegQ {
  v3 a, b, ab;
  v3 lo, hi;            // the segment's box grown by kSegmentMu x the largest |coordinate|
  float maxDist, r2;
  v3 inv;               // sweep_inv of ab's components
  float om;             // the largest |coordinate| of a
};

struct SegCand { float d2; v3 c; float s; int feature; };

// q: the query's eight floats.  false = an invalid query.
PT_HD bool segment_valid(const float q[8]) {
  bool ok = q[6] > 0.0f;                                  // NaN > 0 is false; +inf passes
  for (int k = 0; k < 6; k++) ok = ok & point_finite(q[k]);
  return ok;
}

PT_HD void segment_query(const float q[8], SegQ& s) {
  s.a = mk3(q[0], q[1], q[2]); s.b = mk3(q[3], q[4], q[5]); s.ab = s.b - s.a;
  s.maxDist = q[6]; s.r2 = s.maxDist * s.maxDist;
  float m = 0.0f;
  for (int k = 0; k < 6; k++) m = box_max(m, __builtin_fabsf(q[k]));
  const float g = kSegmentMu * m;
  s.lo = mk3(box_min(s.a.x, s.b.x) - g, box_min(s.a.y, s.b.y) - g, box_min(s.a.z, s.b.z) - g);
  s.hi = mk3(box_max(s.a.x, s.b.x) + g, box_max(s.a.y, s.b.y) + g, box_max(s.a.z, s.b.z) + g);
  s.inv = mk3(sweep_inv(s.ab.x), sweep_inv(s.ab.y), sweep_inv(s.ab.z));
  s.om = box_max(box_max(__builtin_fabsf(s.a.x), __builtin_fabsf(s.a.y)), __builtin_fabsf(s.a.z));
}

// The closest pair between a + ab * s and c + e * t.  Returns d2; x is left out: the record keeps s and y.
PT_HD float segment_segseg(v3 a, v3 ab, v3 c, v3 e, float& s, v3& y) {
  const v3 r = a - c;
  const float A = dot(ab, ab), E = dot(e, e), F = dot(e, r);
  float t;
  if (!(A > 0.0f)) {
    s = 0.0f;
    t = E > 0.0f ? point_clamp01(F / E) : 0.0f;
  } else {
    const float C = dot(ab, r);
    if (!(E > 0.0f)) {
      t = 0.0f; s = point_clamp01(-C / A);
    } else {
      const float B = dot(ab, e);
      const float den = A * E - B * B;
      s = den > 0.0f ? point_clamp01((B * F - C * E) / den) : 0.0f;
      const float tn = B * s + F;
      if (tn < 0.0f)    { t = 0.0f; s = point_clamp01(-C / A); }
      else if (tn > E)  { t = 1.0f; s = point_clamp01((B - C) / A); }
      else              t = point_clamp01(tn / E);
    }
  }
  const v3 x = a + ab * s;
  y = c + e * t;
  return point_d2(x, y);
}

PT_HD void segment_take(float d2, v3 c, float s, int feature, SegCand& best) {
  if (d2 < best.d2) { best.d2 = d2; best.c = c; best.s = s; best.feature = feature; }
}

PT_HD void segment_tri(const SegQ& q, v3 p0, v3 e0, v3 e1, SegCand& best) {
  PointCand k;
  point_tri(q.a, p0, e0, e1, k);
  best.d2 = k.d2; best.c = k.c; best.s = 0.0f; best.feature = SEG_END_A;
  point_tri(q.b, p0, e0, e1, k);
  segment_take(k.d2, k.c, 1.0f, SEG_END_B, best);
  const v3 ea = e0, eb = -e1;
  const v3 v1 = p0 + e0, v2 = p0 - e1;
  float s; v3 y;
  float d2 = segment_segseg(q.a, q.ab, p0, ea, s, y);
  segment_take(d2, y, s, SEG_EDGE0, best);
  d2 = segment_segseg(q.a, q.ab, p0, eb, s, y);
  segment_take(d2, y, s, SEG_EDGE1, best);
  d2 = segment_segseg(q.a, q.ab, v1, v2 - v1, s, y);
  segment_take(d2, y, s, SEG_EDGE2, best);
  v3 n; float t, be, ga;
  if (tri_test(q.a, q.ab, 0.0f, 1.0f, p0, e0, e1, n, t, be, ga)) segment_take(0.0f, q.a + q.ab * t, t, SEG_CROSSING, best);
}

PT_HD void segment_sphere(const SegQ& q, v3 centre, float R, SegCand& out) {
  const v3 m = centre - q.a;
  const float A = dot(q.ab, q.ab);
  const float tca = dot(m, q.ab) / A;
  const float sc = A > 0.0f ? point_clamp01(tca) : 0.0f;
  const v3 x = q.a + q.ab * sc;
  const float lx = point_d2(x, centre), la = point_d2(q.a, centre), lb = point_d2(q.b, centre);
  const float R2 = R * R;
  PointCand k;
  if (lx > R2) {
    point_sphere(x, centre, R, k);
    out.d2 = k.d2; out.c = k.c; out.s = sc; out.feature = sc == 0.0f ? SEG_END_A : sc == 1.0f ? SEG_END_B : SEG_EDGE0;
  } else if ((la < R2) & (lb < R2)) {
    const bool atB = lb > la;
    point_sphere(atB ? q.b : q.a, centre, R, k);
    out.d2 = k.d2; out.c = k.c; out.s = atB ? 1.0f : 0.0f; out.feature = atB ? SEG_END_B : SEG_END_A;
  } else {
    const v3 perp = m - q.ab * tca;
    float disc = R2 - dot(perp, perp);
    disc = disc > 0.0f ? disc : 0.0f;
    const float h = __builtin_sqrtf(disc / A);
    const float t = la > R2 ? tca - h : la < R2 ? tca + h : 0.0f;
    out.s = A > 0.0f ? point_clamp01(t) : 0.0f;
    out.d2 = 0.0f; out.c = q.a + q.ab * out.s; out.feature = SEG_CROSSING;
  }
}

PT_HD void segment_quad(const SegQ& q, v3 v1, v3 v2, v3 anchor, SegCand& out) {
  const v3 E1 = v1 / dot(v1, v1), E2 = v2 / dot(v2, v2);
  const v3 c00 = box_quad_corner(anchor, E1, E2, 0.0f, 0.0f), c10 = box_quad_corner(anchor, E1, E2, 1.0f, 0.0f);
  const v3 c11 = box_quad_corner(anchor, E1, E2, 1.0f, 1.0f), c01 = box_quad_corner(anchor, E1, E2, 0.0f, 1.0f);
  segment_tri(q, c00, c10 - c00, c00 - c11, out);
  SegCand k;
  segment_tri(q, c00, c11 - c00, c00 - c01, k);
  if (k.d2 < out.d2) {
    out = k;
    if ((k.feature >= SEG_EDGE0) & (k.feature <= SEG_EDGE2)) out.feature = k.feature + SEG_QUAD_SECOND;
  }
}

// The squared distance between the segment's grown box and a child's box.
PT_HD float segment_box_d2(const SegQ& q, float lox, float loy, float loz, float hix, float hiy, float hiz) {
  const v3 d = mk3(fmaxf_(fmaxf_(lox - q.hi.x, q.lo.x - hix), 0.0f), fmaxf_(fmaxf_(loy - q.hi.y, q.lo.y - hiy), 0.0f),
                   fmaxf_(fmaxf_(loz - q.hi.z, q.lo.z - hiz), 0.0f));
  return dot(d, d);
}

// The second test of a child: true where the ray a + ab * t, t in [0, 1], misses the child's box grown on every side by
// g = r + kSweepMu * ((r + max|a|) + bm), r = sqrt(bestD2), bm = the largest |plane| of the box -- sweep_slab's margin (pt_sweep.h) with r
// for the radius.  The interval box is a loose bound for a long diagonal segment: most of it is empty of the segment.  Why a missed box
// holds nothing that counts: a primitive under it with computed d2 <= bestD2 has its nearest pair (x, y), y within the padded box (the
// argument above) and x = a + ab * s computed, s in [0, 1] -- or a or b as given, or the crossing point -- within
// sqrt(d2) (1 + 2^-22) <= r (1 + 2^-21) of y and within 5.1 x 2^-24 M of the exact ray at s.  So the exact ray is inside the box grown by
// r (1 + 2^-21) + 2^-21 M at some s in [0, 1], and the computed plane times are the exact times of planes moved by less than
// 2^-22 (|plane| + g + max|a|) (pt_sweep.h, third point): both are far inside kSweepMu = 2^-15 of the same magnitudes.  Prune only.
PT_HD bool segment_slab_miss(const SegQ& q, float r, float lox, float loy, float loz, float hix, float hiy, float hiz) {
  const float bm = box_max(box_max(box_max(__builtin_fabsf(lox), __builtin_fabsf(hix)), box_max(__builtin_fabsf(loy), __builtin_fabsf(hiy))),
                           box_max(__builtin_fabsf(loz), __builtin_fabsf(hiz)));
  const float g = r + kSweepMu * ((r + q.om) + bm);
  const float x0 = ((lox - g) - q.a.x) * q.inv.x, x1 = ((hix + g) - q.a.x) * q.inv.x;
  const float y0 = ((loy - g) - q.a.y) * q.inv.y, y1 = ((hiy + g) - q.a.y) * q.inv.y;
  const float z0 = ((loz - g) - q.a.z) * q.inv.z, z1 = ((hiz + g) - q.a.z) * q.inv.z;
  float tn = fmaxf_(fmaxf_(fminf_(x0, x1), fminf_(y0, y1)), fminf_(z0, z1));
  float tf = fminf_(fminf_(fmaxf_(x0, x1), fmaxf_(y0, y1)), fmaxf_(z0, z1));
  tn = tn > 0.0f ? tn : 0.0f;
  tf = tf < 1.0f ? tf : 1.0f;
  return !(tn <= tf);
}

// Start of a query: the sphere and quad lists brute force in point_begin's order, then the set-up of the walk (PointTrav, point_pop and
// point_pruned are the point walk's own).
template <bool ANY>
PT_HD void segment_begin(const SceneView& sc, const SegQ& q, bool valid, PointTrav& tv) {
  tv.bestD2 = q.r2; tv.bestPrim = -1; tv.bestTri = -1; tv.sp = 0; tv.node = kTravDone;
  if (!valid) return;
  bool done = false;
  for (int i = 0; i < sc.nSpheres && !done; i++) {
    const DevSphere s = load_uniform(sc.spheres + i);
    SegCand k;
    segment_sphere(q, s.center, s.radius, k);
    if (point_accept(k.d2, i, tv.bestD2, tv.bestPrim)) { tv.bestPrim = i; if (ANY) done = true; else tv.bestD2 = k.d2; }
  }
  for (int i = 0; i < sc.nQuads && !done; i++) {
    const DevQuad g = load_uniform(sc.quads + i);
    SegCand k;
    segment_quad(q, g.v1, g.v2, g.anchor, k);
    if (point_accept(k.d2, sc.nSpheres + i, tv.bestD2, tv.bestPrim)) { tv.bestPrim = sc.nSpheres + i; if (ANY) done = true; else tv.bestD2 = k.d2; }
  }
  tv.node = (done || sc.rootRef == kEmptyRef) ? kTravDone : sc.rootRef;
}

// One four-child node for a lane with tv.node >= 0: point_node_step with the box-to-box bound.
template <bool N64, class Stack>
PT_HD void segment_node_step(const SceneView& sc, const SegQ& q, PointTrav& tv, Stack& st) {
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
#if PT_SEGMENT_SLAB
  const float reach = __builtin_sqrtf(tv.bestD2);          // +inf while there is no bound: the second test is then skipped
  const bool slab = point_finite(reach);
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int c = 0; c < 4; c++) {
    const float bd = segment_box_d2(q, lo[0][c], lo[1][c], lo[2][c], hi[0][c], hi[1][c], hi[2][c]);
    bool in = (ref[c] != kEmptyRef) & !point_pruned(bd, tv.bestD2);
#if PT_SEGMENT_SLAB
    in = in & !(slab && segment_slab_miss(q, reach, lo[0][c], lo[1][c], lo[2][c], hi[0][c], hi[1][c], hi[2][c]));
#endif
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

PT_HD v3 segment_pick(const v3 (&a)[4], int j) {
  return mk3(j == 0 ? a[0].x : j == 1 ? a[1].x : j == 2 ? a[2].x : a[3].x, j == 0 ? a[0].y : j == 1 ? a[1].y : j == 2 ? a[2].y : a[3].y,
             j == 0 ? a[0].z : j == 1 ? a[1].z : j == 2 ? a[2].z : a[3].z);
}

// One leaf for a lane with tv.node < 0 (and != kTravDone): the records are fetched as the point walk fetches them.
template <bool ANY, class Stack>
PT_HD void segment_leaf_step(const SceneView& sc, const SegQ& q, PointTrav& tv, Stack& st) {
  const int first = leaf_first(tv.node), count = leaf_count(tv.node);
  const int triBase = sc.nSpheres + sc.nQuads;
  bool done = false;
  for (int base = 0; base < count && !done; base += 4) {
    LeafChunk ch;
    leaf_fetch4(sc, tv.node, base, ch);
    // One copy of the triangle function, not four (sweepkernel.hip): the slot is picked by selects on the loop counter, so the chunk
    // stays in registers.
    for (int j = 0; j < 4; j++) {
      if (base + j < count && !done) {
        const v3 p0 = segment_pick(ch.p0, j), e0 = segment_pick(ch.e0, j), e1 = segment_pick(ch.e1, j);
        const int prim = triBase + (j == 0 ? ch.prim[0] : j == 1 ? ch.prim[1] : j == 2 ? ch.prim[2] : ch.prim[3]);
        SegCand k;
        segment_tri(q, p0, e0, e1, k);
        if (point_accept(k.d2, prim, tv.bestD2, tv.bestPrim)) {
          tv.bestPrim = prim; tv.bestTri = first + base + j;
          if (ANY) done = true; else tv.bestD2 = k.d2;
        }
      }
    }
  }
  if (done) tv.node = kTravDone;
  else point_pop(tv, st);
}

// One traversal step for a lane with tv.node != kTravDone (if-if form, as point_step).
template <bool ANY, bool N64, class Stack>
PT_HD void segment_step(const SceneView& sc, const SegQ& q, PointTrav& tv, Stack& st) {
  if (tv.node >= 0) segment_node_step<N64>(sc, q, tv, st);
  else segment_leaf_step<ANY>(sc, q, tv, st);
}

// The finished closest query's record: the winner's function is evaluated once more for its point, parameter and feature (the same
// operations on the same record, so the same d2).
PT_HD void segment_hit(const SceneView& sc, const SegQ& q, const PointTrav& tv, SegmentHit& h) {
  h.dist = q.maxDist; h.prim = -1; h.mat = -1; h.s = 0.f; h.p[0] = 0.f; h.p[1] = 0.f; h.p[2] = 0.f; h.feature = 0;
  if (tv.bestPrim < 0) return;
  SegCand k;
  if (tv.bestPrim < sc.nSpheres) {
    const DevSphere s = sc.spheres[tv.bestPrim];
    segment_sphere(q, s.center, s.radius, k);
    h.mat = sc.sphereMat[tv.bestPrim];
  } else if (tv.bestPrim < sc.nSpheres + sc.nQuads) {
    const DevQuad* g = sc.quads + (tv.bestPrim - sc.nSpheres);
    segment_quad(q, g->v1, g->v2, g->anchor, k);
    h.mat = g->mat;
  } else {
    const Tri48 t = load_const(at32(sc.tris, tv.bestTri));
    segment_tri(q, t.p0, t.e0, t.e1, k);
    h.mat = t.mat;
  }
  h.dist = __builtin_sqrtf(tv.bestD2); h.prim = tv.bestPrim; h.s = k.s; h.feature = k.feature;
  h.p[0] = k.c.x; h.p[1] = k.c.y; h.p[2] = k.c.z;
}

}  // namespace pt
