// pt_pointmulti.h -- K-nearest point queries: the K nearest primitives to a point, in order (include/moptix.h "K-nearest point queries").
//
// The near set S of a valid query is every pair (d2, prim) over the primitive records with d2 < r2, d2 = pt_point.h's per-primitive
// function: one pair per primitive, a sphere included.  Every primitive counts, whatever its material.  The answer is the K least elements
// of S by (d2, prim), rule D5's total order, and |S| or min(K, |S|): a function of the query and the records alone.
//   NearList             keeps the K least candidates, sorted, as 16-byte keys (d2, prim, triangle record or -1, 0) in the query's own slice
//                        of the output: K keys fill the first half of the K records.  Only the count, the total and the K-th key live in
//                        registers, so K costs neither registers nor LDS, and a lane only ever re-reads what it stored itself.
//   pointmulti_begin     the sphere and quad loops in point_begin's order, feeding the list, then the set-up of the walk.
//   pointmulti_leaf_step point_tri per record, "d2 < r2", then the list's acceptance: count < K, or (d2, prim) below the K-th key.
//   node step            pt_point.h's point_node_step and point_pop, unchanged.  They prune against tv.bestD2, which is the K-th d2 once the
//                        list is full and r2 before (always r2 under ALL, which counts every primitive within maxDist, and with K = 0).
//   pointmulti_finish    turns the keys into records in place, from the last to the first (record j covers keys 2j and 2j + 1, both read
//                        before), through point_hit on a PointTrav per key: the bits are the closest mode's by construction, the miss
//                        records behind the count too.  (u, v, p) are not kept in the key: the same function on the same record gives them
//                        again, bit for bit.
// Why the prune's proof (pt_point.h, kPointPruneSlack) covers the K-th bound.  A primitive that belongs among the K least has d2 <= dK,
// the K-th d2 at any moment of the walk (dK only shrinks), so its boxes have boxD2 <= d2 * slack <= dK * slack by that proof and are not
// dropped.  The prune is strict, so it admits a box at exactly the bound, where a candidate with equal d2 and a lower prim may sit.
// Hence no grazing exception: tree, leaf size, builder, node format, grid and scheduling play no part in the answer.
// The slice is read and written as Word4 only (pt_word4.h), keys and records alike, so nothing is accessed through two types.
// Used by the point kernel (pointkernel.hip pt_pointquery_multi) and by its CPU mirror (tests/pointmultisim/pointmultisim.cpp).
#pragma once
#include "pt_point.h"
#include "pt_word4.h"

namespace pt {

enum { POINT_MULTI_COUNT_ALL = 1 };
constexpr int kPointMultiMaxNear = 64;

struct NearList {
  Word4* e;         // the query's K records; while walking, its K keys (d2, prim, tri, 0), ascending
  int K;            // 0 = count only (ALL)
  int count;        // keys kept: min(K, total)
  int total;        // |S| so far
  float dK; int primK;      // the K-th key, valid when full() and K > 0

  PT_HD void init(Word4* slice, int k) { e = slice; K = k; count = 0; total = 0; dK = 0.f; primK = -1; }
  PT_HD bool full() const { return count == K; }
  PT_HD bool accepts(float d2, int prim) const { return count < K || (K > 0 && key_less(d2, prim, dK, primK)); }
  // a member of S: counted, and kept if it is among the K least so far
  PT_HD void insert(float d2, int prim, int tri) {
    total++;
    if (!accepts(d2, prim)) return;
    int j = count < K ? count : K - 1;      // the slot that opens: the list grows, or its last key drops out
    while (j > 0) {
      const Word4 p = e[j - 1];
      if (!key_less(d2, prim, i2f((int32_t)p.x), (int32_t)p.y)) break;
      e[j] = p; j--;
    }
    e[j] = mkw4((uint32_t)f2i(d2), (uint32_t)prim, (uint32_t)tri, 0u);
    if (count < K) count++;
    if (count == K) { const Word4 l = e[K - 1]; dK = i2f((int32_t)l.x); primK = (int32_t)l.y; }
  }
};

// The bound the node step prunes against.
template <bool ALL>
PT_HD float pointmulti_bound(float r2, const NearList& nl) { return (!ALL && nl.K > 0 && nl.full()) ? nl.dK : r2; }

// The brute-force lists in point_begin's order, then the set-up of the walk.  valid = point_valid's verdict.
template <bool ALL>
PT_HD void pointmulti_begin(const SceneView& sc, v3 q, float r2, bool valid, PointTrav& tv, NearList& nl) {
  tv.bestD2 = r2; tv.bestPrim = -1; tv.bestTri = -1; tv.sp = 0; tv.node = kTravDone;
  if (!valid) return;
  for (int i = 0; i < sc.nSpheres; i++) {
    const DevSphere s = load_uniform(sc.spheres + i);
    PointCand k;
    point_sphere(q, s.center, s.radius, k);
    if (k.d2 < r2) nl.insert(k.d2, i, -1);
  }
  for (int i = 0; i < sc.nQuads; i++) {
    const DevQuad g = load_uniform(sc.quads + i);
    PointCand k;
    point_quad(q, g.v1, g.v2, g.anchor, k);
    if (k.d2 < r2) nl.insert(k.d2, sc.nSpheres + i, -1);
  }
  tv.bestD2 = pointmulti_bound<ALL>(r2, nl);
  tv.node = sc.rootRef == kEmptyRef ? kTravDone : sc.rootRef;
}

// One leaf for a lane with tv.node < 0 (and != kTravDone): every triangle within maxDist goes to the list.
template <bool ALL, class Stack>
PT_HD void pointmulti_leaf_step(const SceneView& sc, v3 q, float r2, PointTrav& tv, Stack& st, NearList& nl) {
  const int first = leaf_first(tv.node), count = leaf_count(tv.node);
  const int triBase = sc.nSpheres + sc.nQuads;
  for (int base = 0; base < count; base += 4) {
    LeafChunk ch;
    leaf_fetch4(sc, tv.node, base, ch);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 4; j++) {
      if (base + j < count) {
        PointCand k;
        point_tri(q, ch.p0[j], ch.e0[j], ch.e1[j], k);
        if (k.d2 < r2) nl.insert(k.d2, triBase + ch.prim[j], first + base + j);
      }
    }
  }
  tv.bestD2 = pointmulti_bound<ALL>(r2, nl);
  point_pop(tv, st);
}

// One traversal step for a lane with tv.node != kTravDone (if-if form, as point_step).
template <bool ALL, bool N64, class Stack>
PT_HD void pointmulti_step(const SceneView& sc, v3 q, float r2, PointTrav& tv, Stack& st, NearList& nl) {
  if (tv.node >= 0) point_node_step<N64>(sc, q, tv, st);
  else pointmulti_leaf_step<ALL>(sc, q, r2, tv, st, nl);
}

// The finished walk's records, in place of the keys: K moptix_point_hit records, the first nl.count from the keys, the rest miss records.
PT_HD void pointmulti_finish(const SceneView& sc, v3 q, float maxDist, const NearList& nl) {
  for (int j = nl.K - 1; j >= 0; j--) {
    PointTrav tv;
    tv.bestD2 = 0.f; tv.bestPrim = -1; tv.bestTri = -1; tv.sp = 0; tv.node = kTravDone;
    if (j < nl.count) {
      const Word4 k = nl.e[j];
      tv.bestD2 = i2f((int32_t)k.x); tv.bestPrim = (int32_t)k.y; tv.bestTri = (int32_t)k.z;
    }
    PointHit h;
    point_hit(sc, q, maxDist, tv, h);
    nl.e[2 * j] = mkw4((uint32_t)f2i(h.dist), (uint32_t)h.prim, (uint32_t)h.mat, (uint32_t)f2i(h.u));
    nl.e[2 * j + 1] = mkw4((uint32_t)f2i(h.v), (uint32_t)f2i(h.p[0]), (uint32_t)f2i(h.p[1]), (uint32_t)f2i(h.p[2]));
  }
}

}  // namespace pt
