// pt_winding.h -- the generalised winding number of a point (Jacobson et al. 2013) with the order-1 far field of Barill et al. 2018,
// moptix_query_winding* of include/moptix.h "winding-number queries".
//
// w(q) = (1 / 4 pi) x the sum of the signed solid angles under which q sees every primitive: 1 inside and 0 outside a closed mesh
// wound outwards, and a smooth function of q for a mesh with holes, flipped or duplicated faces, where w > 0.5 is the classification.
// Every operation in order (pt_math.h: AC1 dot, AC2 cross, AC4 no contraction; division and square root correctly rounded):
//
//   query              16 bytes x y z beta, the point queries' row with beta in the maxDist slot.  beta = +inf or finite >= 1.  A
//                      non-finite coordinate, beta < 1 or a NaN beta: the result is the quiet NaN 0x7fc00000.
//   triangle           a, b, c = the vertices minus q (from a Tri48: p0, p0 + e0, p0 - e1), m = the largest |component| of the nine.
//                      m == 0 (or non-finite): 0.  Else all three times sc = 2^-floor(log2 m), exact, from m's exponent bits as
//                      sign_face scales its normal; then
//                        det = dot(a, cross(b, c))                                   det == 0 -> exactly 0 (q in the face's plane)
//                        la, lb, lc = length(a), length(b), length(c)
//                        den = (((la * lb) * lc + dot(a, b) * lc) + dot(b, c) * la) + dot(c, a) * lb
//                        omega = copysign(2 * atan2_ac(|det|, den), det)             (van Oosterom and Strackee; atan2_ac wants y >= 0)
//   quad               the two triangles of the box queries' split (pt_box.h box_quad): (c00, c10, c11) then (c00, c11, c01).  An open surface.
//   sphere             4 pi (the binary64 constant) when dot(w, w) < radius * radius, w = q - centre, else 0: the signed query's inside test.
//   cluster            a child reference of a node carries A (sum of its faces' areas), p (the area-weighted centroid), N (the sum of
//                      the faces' area vectors 1/2 cross(p1 - p0, p2 - p0)) and a radius r.  d = p - q, l2 = dot(d, d), br = beta * r.
//                      The child is APPROXIMATED iff l2 > br * br, and its term is then dot(N, d) / (l2 * sqrt(l2)).
//                      beta = +inf: never true -- inf > inf is false, and for r == 0 inf * 0 = NaN compares false.
//   moments            per face, in binary32: a = cross(e0, -e1) * 0.5, area = length(a), centroid = ((p0 + p1) + p2) * (1/3).  A leaf
//                      sums its faces in record order, a node child sums that node's children in use in slot order, from their STORED
//                      words; both in binary64: sA += area, sP += area * centroid, sN += a.  Stored: A = (float)sA,
//                      p = (float)sP / A per component (a binary32 division; A == 0: the centre lo * 0.5 + hi * 0.5 of the child's stored box),
//                      N = (float)sN, r = length(max(|lo - p|, |hi - p|) per axis) * (1 + 2^-20) with lo, hi the child's stored box
//                      in the Node128 and p the stored centroid.  The boxes are padded unions of the faces, so the ball (p, r) holds
//                      the whole cluster whatever rounding p suffered: the binary32 error of r is below 2^-22 of it, the factor covers it.
//                      32 bytes per child, one 128-byte record per node, indexed like the nodes.
//   sum                a binary64 accumulator; terms added as (double)term in this order: spheres in id order, quads in id order, the
//                      tree depth first with children in slot order 0..3 and a leaf's triangles in record order (an approximated
//                      child adds its one term where its subtree would have started).
//                      w = (float)(acc * (1 / 4 pi)), the constant in binary64.  No binary64 division or square root anywhere.
//
// TREE DEPENDENCE.  Unlike every other query of the library the value depends on the tree.  For a finite beta it does so through the
// approximation: which clusters exist, and so which are replaced by their dipole, is the builder's choice (leaf size, builder).
// For beta = +inf no cluster is approximated and the value depends on the tree only through the order of a binary64 sum of the same
// binary32 terms: differences of a few 1e-16 of the largest partial sum before the rounding to binary32, so almost always the same
// word, but not provably.  It does not depend on the node format: the walk reads the references from the Node128 array and the
// moments from the table, never a box.
//
// The stated range: p - q finite for every vertex (the triangle term scales itself, so its den cannot overflow); for the cluster
// term l2 * sqrt(l2) finite and normal -- distances |p - q| between about 1e-12 and 1e12 units -- and areas whose products with
// such distances stay finite; for the moments edges between about 1e-9 and 1e9 units, the range of pt_sign.h.
//
// Compiled for the device (windingkernel.hip) and for the CPU mirror (tests/windingsim/windingsim.cpp).
#pragma once
#include "pt_box.h"
#include "pt_sign.h"
#include "pt_refit.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define PT_WINDING_NOUNROLL _Pragma("nounroll")
#else
#define PT_WINDING_NOUNROLL
#endif

namespace pt {

struct alignas(16) WindingChild { float A; v3 p; v3 N; float r; };
static_assert(sizeof(WindingChild) == 32, "WindingChild is two 16-byte rows");
struct alignas(128) WindingNode { WindingChild c[4]; };
static_assert(sizeof(WindingNode) == 128, "WindingNode is one 128-byte record per node");

constexpr double kWinding4Pi = 12.566370614359172;       // 4 pi
constexpr double kWindingInv4Pi = 0.07957747154594767;   // 1 / (4 pi)
constexpr float kWindingRadiusUp = 1.00000095367431640625f;      // 1 + 2^-20

// p: the query's four floats.  false = an invalid query.
PT_HD bool winding_valid(const float p[4]) {
  bool ok = p[3] >= 1.0f;                                 // NaN >= 1 is false; +inf passes
  for (int k = 0; k < 3; k++) ok = ok & point_finite(p[k]);
  return ok;
}

PT_HD float winding_max3(v3 a) { return fmaxf_(fmaxf_(__builtin_fabsf(a.x), __builtin_fabsf(a.y)), __builtin_fabsf(a.z)); }

// The signed solid angle of the triangle (v0, v1, v2) seen from q.
PT_HD float winding_tri_verts(v3 q, v3 v0, v3 v1, v3 v2) {
  v3 a = v0 - q, b = v1 - q, c = v2 - q;
  const float m = fmaxf_(fmaxf_(winding_max3(a), winding_max3(b)), winding_max3(c));
  if (!((m > 0.0f) & point_finite(m))) return 0.0f;
  const float sc = i2f(0x7f000000 - (f2i(m) & 0x7f800000));      // 2^-floor(log2 m), exact (2^127 for a subnormal m)
  a = a * sc; b = b * sc; c = c * sc;
  const float det = dot(a, cross(b, c));
  if (det == 0.0f) return 0.0f;
  const float la = length(a), lb = length(b), lc = length(c);
  const float den = (((la * lb) * lc + dot(a, b) * lc) + dot(b, c) * la) + dot(c, a) * lb;
  return __builtin_copysignf(2.0f * atan2_ac(__builtin_fabsf(det), den), det);
}

// The triangle term on a Tri48 record's p0, e0, e1.
PT_HD float winding_tri(v3 q, v3 p0, v3 e0, v3 e1) { return winding_tri_verts(q, p0, p0 + e0, p0 - e1); }

// A quad's two terms, in the order of the sum.
PT_HD void winding_quad(v3 q, v3 v1, v3 v2, v3 anchor, double& acc) {
  const v3 E1 = v1 / dot(v1, v1), E2 = v2 / dot(v2, v2);
  const v3 c00 = box_quad_corner(anchor, E1, E2, 0.0f, 0.0f), c11 = box_quad_corner(anchor, E1, E2, 1.0f, 1.0f);
  // one copy of the triangle function, not two: (c00, c10, c11), then (c00, c11, c01)
  PT_WINDING_NOUNROLL
  for (int h = 0; h < 2; h++) {
    const v3 c = box_quad_corner(anchor, E1, E2, h == 0 ? 1.0f : 0.0f, h == 0 ? 0.0f : 1.0f);
    acc += (double)winding_tri_verts(q, c00, h == 0 ? c : c11, h == 0 ? c11 : c);
  }
}

PT_HD bool winding_sphere(v3 q, v3 centre, float radius) {
  const v3 w = q - centre;
  return dot(w, w) < radius * radius;
}

// Is the child approximated, and if so its term.
PT_HD bool winding_cluster(v3 q, float beta, const WindingChild& k, float& term) {
  const v3 d = k.p - q;
  const float l2 = dot(d, d);
  const float br = beta * k.r;
  if (!(l2 > br * br)) return false;
  term = dot(k.N, d) / (l2 * __builtin_sqrtf(l2));
  return true;
}

PT_HD float winding_result(double acc) { return (float)(acc * kWindingInv4Pi); }

// ---- the moments ----
struct WindingSums { double A, px, py, pz, nx, ny, nz; };

PT_HD void winding_sums_clear(WindingSums& s) { s.A = 0.0; s.px = 0.0; s.py = 0.0; s.pz = 0.0; s.nx = 0.0; s.ny = 0.0; s.nz = 0.0; }
PT_HD void winding_sums_add(WindingSums& s, float A, v3 p, v3 N) {
  s.A += (double)A;
  s.px += (double)A * (double)p.x; s.py += (double)A * (double)p.y; s.pz += (double)A * (double)p.z;
  s.nx += (double)N.x; s.ny += (double)N.y; s.nz += (double)N.z;
}
PT_HD void winding_sums_face(WindingSums& s, const Tri48& t) {
  const v3 a = cross(t.e0, -t.e1) * 0.5f;
  const v3 p1 = t.p0 + t.e0, p2 = t.p0 - t.e1;
  winding_sums_add(s, length(a), ((t.p0 + p1) + p2) * (1.0f / 3.0f), a);
}

// The record of child k of node nd: a leaf's from its triangle records, a node's from that node's finished record.
PT_HD WindingChild winding_child(const Node128& nd, int k, const Node128* nodes, const Tri48* tris, const WindingNode* table) {
  WindingSums s;
  winding_sums_clear(s);
  const int ref = nd.ref[k];
  if (ref < 0) {
    const int first = leaf_first(ref), count = leaf_count(ref);
    for (int i = 0; i < count; i++) winding_sums_face(s, tris[first + i]);
  } else {
    const Node128& ch = nodes[ref];
    const WindingNode& m = table[ref];
    for (int j = 0; j < 4; j++)
      if (ch.ref[j] != kEmptyRef) winding_sums_add(s, m.c[j].A, m.c[j].p, m.c[j].N);
  }
  const v3 lo = mk3(refit_row(nd.lox, k), refit_row(nd.loy, k), refit_row(nd.loz, k));
  const v3 hi = mk3(refit_row(nd.hix, k), refit_row(nd.hiy, k), refit_row(nd.hiz, k));
  WindingChild w;
  w.A = (float)s.A;
  if (w.A == 0.0f) w.p = lo * 0.5f + hi * 0.5f;
  else w.p = mk3((float)s.px / w.A, (float)s.py / w.A, (float)s.pz / w.A);
  w.N = mk3((float)s.nx, (float)s.ny, (float)s.nz);
  const v3 dl = lo - w.p, dh = hi - w.p;
  const v3 mx = mk3(fmaxf_(__builtin_fabsf(dl.x), __builtin_fabsf(dh.x)), fmaxf_(__builtin_fabsf(dl.y), __builtin_fabsf(dh.y)),
                    fmaxf_(__builtin_fabsf(dl.z), __builtin_fabsf(dh.z)));
  w.r = length(mx) * kWindingRadiusUp;
  return w;
}

// One node's record; the slots not in use are zero.
PT_HD WindingNode winding_node(const Node128& nd, const Node128* nodes, const Tri48* tris, const WindingNode* table) {
  WindingNode out;
  for (int k = 0; k < 4; k++) {
    if (nd.ref[k] != kEmptyRef) { out.c[k] = winding_child(nd, k, nodes, tris, table); continue; }
    out.c[k].A = 0.f; out.c[k].p = mk3(0.f, 0.f, 0.f); out.c[k].N = mk3(0.f, 0.f, 0.f); out.c[k].r = 0.f;
  }
  return out;
}

// ---- the walk ----
// node: kTravDone, a leaf reference (< 0) whose triangles are due, or the entry 4 * node + slot (>= 0) of a child still to be decided
// -- which is also that child's index in the table read as an array of WindingChild.  The stack holds entries alone.
struct WindingTrav { int node, sp; double acc; };
// What the mirror counts per query, where asked for: clusters approximated, triangles evaluated.
struct WindingWork { long long clusters, tris; };

template <class Stack>
PT_HD void winding_pop(WindingTrav& tv, Stack& st) {
  if (tv.sp > 0) { tv.sp--; tv.node = st.load(tv.sp); }
  else tv.node = kTravDone;
}

// Node m is entered: its first child in use is decided next, the others are pushed, so that they come off in slot order.
template <class Stack>
PT_HD void winding_expand(const SceneView& sc, int m, WindingTrav& tv, Stack& st) {
  const i4r rf = load_const(reinterpret_cast<const i4r*>(&at32(sc.nodes, m)->ref[0]));
  const int ref[4] = { rf.x, rf.y, rf.z, rf.w };
  int next = kTravDone;
  for (int c = 3; c >= 0; c--) {
    if (ref[c] == kEmptyRef) continue;
    if (next != kTravDone) { st.store(tv.sp, next); tv.sp++; }
    next = 4 * m + c;
  }
  if (next == kTravDone) winding_pop(tv, st);
  else tv.node = next;
}

// Spheres and quads in id order, then the set-up of the walk.  valid = winding_valid's verdict.
template <class Stack>
PT_HD void winding_begin(const SceneView& sc, v3 q, bool valid, WindingTrav& tv, Stack& st) {
  tv.sp = 0; tv.node = kTravDone; tv.acc = 0.0;
  if (!valid) return;
  for (int i = 0; i < sc.nSpheres; i++) {
    const DevSphere s = load_uniform(sc.spheres + i);
    if (winding_sphere(q, s.center, s.radius)) tv.acc += kWinding4Pi;
  }
  for (int i = 0; i < sc.nQuads; i++) {
    const DevQuad g = load_uniform(sc.quads + i);
    winding_quad(q, g.v1, g.v2, g.anchor, tv.acc);
  }
  if (sc.rootRef == kEmptyRef) return;
  if (sc.rootRef < 0) tv.node = sc.rootRef;      // a root that is a leaf: exact, there is no record for the tree as a whole
  else winding_expand(sc, sc.rootRef, tv, st);
}

// One step for a lane with tv.node != kTravDone (if-if form).  table: the moments, one record per node.  work: the mirror's counters,
// null on the device.
template <class Stack>
PT_HD void winding_step(const SceneView& sc, const WindingNode* table, v3 q, float beta, WindingTrav& tv, Stack& st, WindingWork* work = nullptr) {
  if (tv.node >= 0) {
    const WindingChild k = load_const(at32(reinterpret_cast<const WindingChild*>(table), tv.node));
    float term;
    if (winding_cluster(q, beta, k, term)) {
#if !defined(__HIP_DEVICE_COMPILE__)
      if (work) work->clusters++;
#endif
      tv.acc += (double)term;
      winding_pop(tv, st);
    } else {
      const int ref = load_const(&at32(sc.nodes, tv.node >> 2)->ref[tv.node & 3]);
      if (ref < 0) tv.node = ref;
      else winding_expand(sc, ref, tv, st);
    }
  }
  if (tv.node < 0) {
    const int first = leaf_first(tv.node), count = leaf_count(tv.node);
    PT_WINDING_NOUNROLL
    for (int i = 0; i < count; i++) {
      const Tri48 t = load_const(at32(sc.tris, first + i));
#if !defined(__HIP_DEVICE_COMPILE__)
      if (work) work->tris++;
#endif
      tv.acc += (double)winding_tri(q, t.p0, t.e0, t.e1);
    }
    winding_pop(tv, st);
  }
}

// The whole query: p the row's four floats.
template <class Stack>
PT_HD float winding_query(const SceneView& sc, const WindingNode* table, const float p[4], Stack& st, WindingWork* work = nullptr, int* deepest = nullptr) {
  if (!winding_valid(p)) return i2f(0x7fc00000);
  const v3 q = mk3(p[0], p[1], p[2]);
  WindingTrav tv;
  winding_begin(sc, q, true, tv, st);
  while (tv.node != kTravDone) {
#if !defined(__HIP_DEVICE_COMPILE__)
    if (deepest && tv.sp > *deepest) *deepest = tv.sp;
#endif
    winding_step(sc, table, q, p[3], tv, st, work);
  }
  return winding_result(tv.acc);
}

}  // namespace pt
