// pt_sign.h -- the sign of a point query's distance by angle-weighted pseudonormals (Baerentzen and Aanaes), MOPTIX_POINT_SIGNED of
// include/moptix.h "point queries".
//
// The signed query is the closest query (pt_point.h) with one more decision at its end: is q on the inner side of the winner.  That is
// a function of q, the winner's device record and the winner's row of the sign table alone, so the signed answer is still what a loop
// over every primitive gives, bit for bit.  Every operation in order (pt_math.h: AC1 dot, AC2 cross, AC3 normalize, AC4 no contraction;
// division and square root correctly rounded):
//
//   atan2_ac(y, x)     for y >= 0, ONE specified binary32 algorithm in the manner of sincos_ac:
//                        ax = |x|;  hi = ax > y ? ax : y;  lo = ax > y ? y : ax;  hi == 0 -> 0
//                        t = lo / hi                                         in [0, 1]
//                        t > 0.41421356 (tan pi/8):  r = (t - 1) / (t + 1), base = pi/4;  else r = t, base = 0
//                        z = r * r;  p = fma(fma(fma(8.05374449538e-2, z, -1.38776856032e-1), z, 1.99777106478e-1), z, -3.33329491539e-1)
//                        a = base + fma(p * z, r, r)                         (the classic single-precision kernel, degree 4 in z)
//                        y > ax -> a = pi/2 - a;   x < 0 -> a = pi - a
//                      Measured against binary64 atan2 of the same binary32 inputs (tests/test_sign_cpu.py: a log-uniform grid of
//                      magnitudes 1e-6 .. 1e3 in both arguments, both signs of x, and y = 0, x = 0, y = x): max absolute error 2.5e-7.
//                      Out of its range: y < 0, NaN, both arguments infinite.
//   face normal        n = cross(p1 - p0, p2 - p0), m = its largest |component|.  m == 0 or non-finite: the face is DEGENERATE, un = 0 and
//                      its three angles are 0.  Else sc = 2^-floor(log2 m) (exact, from m's exponent bits, as point_tri scales its
//                      normal: dot(n, n) itself leaves binary32 for long and short edges), ns = n * sc, un = ns * (1 / sqrt(dot(ns, ns)))
//   corner angle       of corner k with a = p(k+1) - p(k), b = p(k+2) - p(k) (indices mod 3): atan2_ac(length(cross(a, b)), dot(a, b))
//   vertex sum         from (+0, +0, +0), over the welded vertex's corners in ascending (face id, corner):  sum = sum + un(face) * angle
//   edge sum           from (+0, +0, +0), over the edge's faces in ascending face id:  sum = sum + un(face)
//                      Plain adds in that order, no atomics: the words depend on positions and topology alone.  A degenerate face adds
//                      zeros, which changes no word (a sum that starts at +0 never becomes -0).  The sums are not normalised: only the
//                      sign of s below is used.
//   feature            point_tri_feature repeats point_tri's operations on the winner's record and reports WHICH candidate won (the first
//                      of equal ones) and, for a segment, its clamped parameter t:
//                        1  segment(v0, e0)        t == 0 vertex 0,  t == 1 vertex 1,  else edge 01
//                        2  segment(v0, -e1)       t == 0 vertex 0,  t == 1 vertex 2,  else edge 02
//                        3  segment(v1, v2 - v1)   t == 0 vertex 1,  t == 1 vertex 2,  else edge 12
//                        4  the projection         face
//                      Not from the reported (u, v): (1 - t) + t is not always 1, and a point that is on an edge by the arithmetic can
//                      have barycentrics that say otherwise.
//   sign               c = the reported nearest point, N = the feature's row of the winner's record, s = dot(q - c, N);
//                      dist = s < 0 ? -sqrt(d2) : +sqrt(d2): s == 0 (q == c included) and NaN give +.
//                      sphere: inside iff dot(w, w) < radius * radius, w = q - centre.  quad: always + (an open surface).
//
// The stated range: edges whose cross products, and their squared lengths, stay finite and normal in binary32 -- edge lengths
// between about 1e-9 and 1e9 units.  Meshes that span many decades beyond that are not a use case of the sign.
//
// The table: one 96-byte record per ORIGINAL face id (not per sorted slot: it survives a rebuild of the tree) -- SignRecord below.
// Compiled for the device (signkernel.hip) and for the CPU mirror (tests/hostsim/signsim.cpp).
#pragma once
#include "pt_point.h"

namespace pt {

enum { POINT_SIGNED = 2 };

// rows of a SignRecord, and the codes point_tri_feature returns
enum { SIGN_V0 = 0, SIGN_V1 = 1, SIGN_V2 = 2, SIGN_E01 = 3, SIGN_E02 = 4, SIGN_E12 = 5, SIGN_FACE = 6 };

struct alignas(16) SignRecord { v3 n[7]; float pad[3]; };      // v0 v1 v2 e01 e02 e12, the unit face normal, padding
static_assert(sizeof(SignRecord) == 96, "SignRecord is six 16-byte rows");

// what the per-face pass leaves for the gathers: the unit normal and the three corner angles
struct alignas(16) SignFace { v3 un; float pad0; float angle[3]; float pad1; };
static_assert(sizeof(SignFace) == 32, "SignFace is two 16-byte rows");

constexpr float kSignTanPi8 = 0.41421356f;
constexpr float kSignPi4 = 0.78539816339744830962f, kSignPi2 = 1.57079632679489661923f;

PT_HD float atan2_ac(float y, float x) {
  const float ax = __builtin_fabsf(x);
  const bool swap = y > ax;
  const float hi = swap ? y : ax, lo = swap ? ax : y;
  if (hi == 0.0f) return 0.0f;
  const float t = lo / hi;
  const bool red = t > kSignTanPi8;
  const float r = red ? (t - 1.0f) / (t + 1.0f) : t;
  const float z = r * r;
  const float p = fma_(fma_(fma_(8.05374449538e-2f, z, -1.38776856032e-1f), z, 1.99777106478e-1f), z, -3.33329491539e-1f);
  float a = (red ? kSignPi4 : 0.0f) + fma_(p * z, r, r);
  if (swap) a = kSignPi2 - a;
  if (x < 0.0f) a = kPi - a;
  return a;
}

PT_HD float sign_corner_angle(v3 a, v3 b) { return atan2_ac(length(cross(a, b)), dot(a, b)); }

// p: the face's nine floats p0 p1 p2.  dead: the topology already counts the face as degenerate (two corners welded together).
PT_HD SignFace sign_face(const float* p, bool dead) {
  SignFace f;
  f.un = mk3(0.f, 0.f, 0.f); f.pad0 = 0.f; f.angle[0] = 0.f; f.angle[1] = 0.f; f.angle[2] = 0.f; f.pad1 = 0.f;
  const v3 p0 = mk3(p[0], p[1], p[2]), p1 = mk3(p[3], p[4], p[5]), p2 = mk3(p[6], p[7], p[8]);
  const v3 n = cross(p1 - p0, p2 - p0);
  const float m = fmaxf_(fmaxf_(__builtin_fabsf(n.x), __builtin_fabsf(n.y)), __builtin_fabsf(n.z));
  if (dead || !((m > 0.0f) & point_finite(m))) return f;
  const float sc = i2f(0x7f000000 - (f2i(m) & 0x7f800000));
  f.un = normalize(n * sc);
  f.angle[0] = sign_corner_angle(p1 - p0, p2 - p0);
  f.angle[1] = sign_corner_angle(p2 - p1, p0 - p1);
  f.angle[2] = sign_corner_angle(p0 - p2, p1 - p2);
  return f;
}

// The gathers over the CSR lists of the topology (corner = 3 * face + k).
PT_HD v3 sign_vertex_sum(const SignFace* faces, const int* corners, int first, int end) {
  v3 s = mk3(0.f, 0.f, 0.f);
  for (int i = first; i < end; i++) {
    const int c = corners[i], f = c / 3, k = c - 3 * f;
    s = s + faces[f].un * faces[f].angle[k];
  }
  return s;
}
PT_HD v3 sign_edge_sum(const SignFace* faces, const int* edgeFaces, int first, int end) {
  v3 s = mk3(0.f, 0.f, 0.f);
  for (int i = first; i < end; i++) s = s + faces[edgeFaces[i]].un;
  return s;
}

// vertexN, edgeN: the sums, one 16-byte row each (w = 0).  ids: the face's three welded vertex ids and three edge ids (01, 02, 12); ids[0] < 0: a degenerate face of the topology, whose
// record is zero.  A face whose normal is degenerate NOW has un = 0 and a zero record as well.
PT_HD SignRecord sign_record(const int* ids, const SignFace& f, const v4* vertexN, const v4* edgeN) {
  SignRecord r;
  for (int k = 0; k < 7; k++) r.n[k] = mk3(0.f, 0.f, 0.f);
  r.pad[0] = 0.f; r.pad[1] = 0.f; r.pad[2] = 0.f;
  if (ids[0] < 0 || !length_is_nonzero(f.un)) return r;
  for (int k = 0; k < 3; k++) { r.n[SIGN_V0 + k] = xyz(vertexN[ids[k]]); r.n[SIGN_E01 + k] = xyz(edgeN[ids[3 + k]]); }
  r.n[SIGN_FACE] = f.un;
  return r;
}

PT_HD int sign_segment_feature(float t, int va, int vb, int edge) { return t == 0.0f ? va : (t == 1.0f ? vb : edge); }

// point_tri's operations, in its order, with its comparisons; returns the feature the nearest point lies on.
PT_HD int point_tri_feature(v3 q, v3 p0, v3 e0, v3 e1) {
  const v3 ea = e0, eb = -e1;
  const v3 v1 = p0 + e0, v2 = p0 - e1;
  v3 c;
  float t = point_segment(q, p0, ea, c);
  float best = point_d2(q, c);
  int feature = sign_segment_feature(t, SIGN_V0, SIGN_V1, SIGN_E01);
  t = point_segment(q, p0, eb, c);
  float d2 = point_d2(q, c);
  if (d2 < best) { best = d2; feature = sign_segment_feature(t, SIGN_V0, SIGN_V2, SIGN_E02); }
  t = point_segment(q, v1, v2 - v1, c);
  d2 = point_d2(q, c);
  if (d2 < best) { best = d2; feature = sign_segment_feature(t, SIGN_V1, SIGN_V2, SIGN_E12); }
  const v3 n = cross(ea, eb);
  const float m = fmaxf_(fmaxf_(__builtin_fabsf(n.x), __builtin_fabsf(n.y)), __builtin_fabsf(n.z));
  if ((m > 0.0f) & point_finite(m)) {
    const float sc = i2f(0x7f000000 - (f2i(m) & 0x7f800000));
    const v3 ns = n * sc;
    const float nn = dot(ns, ns);
    const v3 w = q - p0;
    const float bu = (dot(cross(w, eb), ns) * sc) / nn, bv = (dot(cross(ea, w), ns) * sc) / nn;
    if ((bu >= 0.0f) & (bv >= 0.0f) & (bu + bv <= 1.0f)) {
      c = (p0 + ea * bu) + eb * bv;
      d2 = point_d2(q, c);
      if (d2 < best) feature = SIGN_FACE;
    }
  }
  return feature;
}

// true = inside: s = dot(q - c, N) < 0
PT_HD bool point_sign(v3 q, v3 c, v3 N) { return dot(q - c, N) < 0.0f; }

// The finished signed query's record: point_hit, then the feature, one v3 of the winner's sign record, the sign.  table: one SignRecord
// per original face id (never read when no triangle wins).
PT_HD void point_hit_signed(const SceneView& sc, const SignRecord* table, v3 q, float maxDist, const PointTrav& tv, PointHit& h) {
  point_hit(sc, q, maxDist, tv, h);
  if (tv.bestPrim < 0) return;
  bool inside = false;
  if (tv.bestPrim < sc.nSpheres) {
    const DevSphere s = sc.spheres[tv.bestPrim];
    const v3 w = q - s.center;
    inside = dot(w, w) < s.radius * s.radius;
  } else if (tv.bestPrim >= sc.nSpheres + sc.nQuads) {
    const Tri48 t = load_const(at32(sc.tris, tv.bestTri));
    const int feature = point_tri_feature(q, t.p0, t.e0, t.e1);
    const v3 N = table[(size_t)t.prim].n[feature];
    inside = point_sign(q, mk3(h.p[0], h.p[1], h.p[2]), N);
  }
  if (inside) h.dist = -h.dist;
}

}  // namespace pt
