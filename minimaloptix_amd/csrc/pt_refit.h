// pt_refit.h -- the per-triangle and per-node code of the in-place refit (refitkernel.hip; CPU mirror: tests/refitsim).
//
// A refit keeps the tree's topology and the order of the triangle records and rewrites what depends on the positions, defined
// without reference to any schedule (include/moptix.h "mesh updates and refit"):
//   scene box      min / max over the faces' raw boxes; padAbs = 1e-5 * its largest extent + 1e-30 (lbvh.hip k_leaves)
//   triangle       Tri48 { p0, e0 = p1 - p0, e1 = p0 - p2; mat, prim, shadow kept }, TriShade from the face's normals, and the padded
//                  box pad_lo / pad_hi(raw box, padAbs) -- from the three positions, not from p0, e0, e1
//   leaf child     min / max over its triangles' PADDED boxes (pad, then union: pad_lo is not provably monotone in binary32)
//   node child     min / max over that node's child boxes
//   Node64         compress_node(Node128)
// min / max are exact, so the words do not depend on the order of evaluation, and a refit over unchanged positions gives the words
// the builder wrote: the builder's box of a Karras node is the union of the padded boxes in its range, however it was parenthesised.
#pragma once
#include "pt_lbvh.h"

namespace pt {

// raw and padded box of one sorted triangle slot, two 16-byte rows
struct alignas(16) RefitBox { float lox, loy, loz, pad0, hix, hiy, hiz, pad1; };
static_assert(sizeof(RefitBox) == 32, "RefitBox is two float4 rows");

PT_HD float refit_pad_abs(v3 slo, v3 shi) {      // k_leaves' padAbs, operation for operation
  const float ex = shi.x - slo.x, ey = shi.y - slo.y, ez = shi.z - slo.z;
  return 1e-5f * fmaxf_(fmaxf_(ex, ey), ez) + 1e-30f;
}

// The records of the triangle in one sorted slot from its face's new positions p (9 floats) and normals q (9 floats, read only when
// hasNrm); raw: the unpadded box.
PT_HD void refit_triangle(const float* p, const float* q, bool hasNrm, const Tri48& old, Tri48& t, TriShade& sh, RefitBox& raw) {
  const v3 p0 = mk3(p[0], p[1], p[2]), p1 = mk3(p[3], p[4], p[5]), p2 = mk3(p[6], p[7], p[8]);
  t.p0 = p0; t.e0 = p1 - p0; t.e1 = p0 - p2; t.mat = old.mat; t.prim = old.prim; t.shadow = old.shadow;
  sh.n0 = mk3(0, 0, 0); sh.n1 = sh.n0; sh.n2 = sh.n0; sh.hasNormals = 0; sh.pad1 = 0; sh.pad2 = 0;
  if (hasNrm) { sh.n0 = mk3(q[0], q[1], q[2]); sh.n1 = mk3(q[3], q[4], q[5]); sh.n2 = mk3(q[6], q[7], q[8]); sh.hasNormals = 1; }
  v3 l, h;
  tri_bounds(p0, p1, p2, l, h);
  raw.lox = l.x; raw.loy = l.y; raw.loz = l.z; raw.pad0 = 0.f; raw.hix = h.x; raw.hiy = h.y; raw.hiz = h.z; raw.pad1 = 0.f;
}

PT_HD RefitBox refit_pad(const RefitBox& r, float padAbs) {
  RefitBox b;
  b.lox = pad_lo(r.lox, padAbs); b.loy = pad_lo(r.loy, padAbs); b.loz = pad_lo(r.loz, padAbs); b.pad0 = 0.f;
  b.hix = pad_hi(r.hix, padAbs); b.hiy = pad_hi(r.hiy, padAbs); b.hiz = pad_hi(r.hiz, padAbs); b.pad1 = 0.f;
  return b;
}

// component k of the six box rows of a node
PT_HD float& refit_row(v4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
PT_HD float refit_row(const v4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// The box of one child reference: a leaf's from the raw boxes of its triangles (padded here), a node's from that node's child boxes
// (the child must have been refitted already).
PT_HD RefitBox refit_child_box(int ref, const RefitBox* raw, float padAbs, const Node128* nodes) {
  RefitBox b;
  b.lox = b.loy = b.loz = 3.0e38f; b.hix = b.hiy = b.hiz = -3.0e38f; b.pad0 = 0.f; b.pad1 = 0.f;
  if (ref < 0) {
    const int first = leaf_first(ref), count = leaf_count(ref);
    for (int i = 0; i < count; i++) {
      const RefitBox t = refit_pad(raw[first + i], padAbs);
      b.lox = fminf_(b.lox, t.lox); b.loy = fminf_(b.loy, t.loy); b.loz = fminf_(b.loz, t.loz);
      b.hix = fmaxf_(b.hix, t.hix); b.hiy = fmaxf_(b.hiy, t.hiy); b.hiz = fmaxf_(b.hiz, t.hiz);
    }
  } else {
    const Node128 c = nodes[ref];
    for (int k = 0; k < 4; k++) {
      if (c.ref[k] == kEmptyRef) continue;
      b.lox = fminf_(b.lox, refit_row(c.lox, k)); b.loy = fminf_(b.loy, refit_row(c.loy, k)); b.loz = fminf_(b.loz, refit_row(c.loz, k));
      b.hix = fmaxf_(b.hix, refit_row(c.hix, k)); b.hiy = fmaxf_(b.hiy, refit_row(c.hiy, k)); b.hiz = fmaxf_(b.hiz, refit_row(c.hiz, k));
    }
  }
  return b;
}

// One node: the boxes of its children in use; refs, count, padding and the unused slots stay as they are.
PT_HD void refit_node(Node128& nd, const RefitBox* raw, float padAbs, const Node128* nodes) {
  for (int k = 0; k < 4; k++) {
    if (nd.ref[k] == kEmptyRef) continue;
    const RefitBox b = refit_child_box(nd.ref[k], raw, padAbs, nodes);
    refit_row(nd.lox, k) = b.lox; refit_row(nd.loy, k) = b.loy; refit_row(nd.loz, k) = b.loz;
    refit_row(nd.hix, k) = b.hix; refit_row(nd.hiy, k) = b.hiy; refit_row(nd.hiz, k) = b.hiz;
  }
}

// ---- the quality signal: the tree's surface-area cost, in binary64 ----
// half the surface area of a box given in binary32 (the factor 2 cancels in the ratio)
PT_HD double refit_area(float lox, float loy, float loz, float hix, float hiy, float hiz) {
  const double dx = (double)hix - (double)lox, dy = (double)hiy - (double)loy, dz = (double)hiz - (double)loz;
  return (dx * dy + dy * dz) + dz * dx;
}
// a node's term: area(child box) x (1 for a node child, the triangle count for a leaf child) over its children in use
PT_HD double refit_node_cost(const Node128& nd) {
  double s = 0.0;
  for (int k = 0; k < 4; k++) {
    if (nd.ref[k] == kEmptyRef) continue;
    const double a = refit_area(refit_row(nd.lox, k), refit_row(nd.loy, k), refit_row(nd.loz, k), refit_row(nd.hix, k), refit_row(nd.hiy, k), refit_row(nd.hiz, k));
    s += a * (nd.ref[k] < 0 ? (double)leaf_count(nd.ref[k]) : 1.0);
  }
  return s;
}
// the divisor: the area of the union of the root's child boxes
PT_HD double refit_root_area(const Node128& root) {
  float l[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, h[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
  for (int k = 0; k < 4; k++) {
    if (root.ref[k] == kEmptyRef) continue;
    l[0] = fminf_(l[0], refit_row(root.lox, k)); l[1] = fminf_(l[1], refit_row(root.loy, k)); l[2] = fminf_(l[2], refit_row(root.loz, k));
    h[0] = fmaxf_(h[0], refit_row(root.hix, k)); h[1] = fmaxf_(h[1], refit_row(root.hiy, k)); h[2] = fmaxf_(h[2], refit_row(root.hiz, k));
  }
  return refit_area(l[0], l[1], l[2], h[0], h[1], h[2]);
}

// ---- the plan: levels of the emitted four-wide tree (its ref[] words; the builders number nodes differently) ----
// order: node indices level by level from the root (breadth first, children in slot order); levelFirst[L] .. levelFirst[L + 1]: level L's
// part of it.  Host only.  Returns false when the references do not form a tree over nNodes nodes.
template <class IntVec>
inline bool refit_plan_levels(const Node128* nodes, int nNodes, IntVec& order, IntVec& levelFirst) {
  order.clear(); levelFirst.clear();
  if (nNodes <= 0) return true;
  order.push_back(0); levelFirst.push_back(0);
  size_t begin = 0;
  while (begin < order.size()) {
    const size_t end = order.size();
    levelFirst.push_back((int)end);
    for (size_t i = begin; i < end; i++)
      for (int k = 0; k < 4; k++) {
        const int r = nodes[order[i]].ref[k];
        if (r == kEmptyRef || r < 0) continue;
        if (r >= nNodes || order.size() >= (size_t)nNodes) return false;
        order.push_back(r);
      }
    begin = end;
  }
  return order.size() == (size_t)nNodes;
}

}  // namespace pt
