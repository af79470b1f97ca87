// pt_multihit.h -- multi-hit ray queries: the first K hits along a ray, in order (include/moptix.h "multi-hit ray queries").
//
// The hit set H of a valid ray is every pair (t, prim) a primitive record's own test accepts inside (tmin, tmax): tri_test, quad_test,
// and each root of sphere_roots (a sphere entered and left gives two pairs with one prim, a tangent ray with t1 == t2 one).  Every
// primitive counts, whatever its material.  The answer is the K least elements of H by (t, prim), rule D5's total order, and |H| or
// min(K, |H|): a function of the ray and the records alone.
//   HitList          keeps the K least candidates, sorted, as 16-byte keys (t, prim, triangle record) in the ray's own slice of the output:
//                    K keys fill the first half of the K records.  Only the count and the K-th key live in registers, so K costs neither
//                    registers nor LDS, and a lane only ever re-reads what it stored itself.
//   multi_begin      the sphere and quad loops in trav_begin's order, feeding both roots, then the set-up of the BVH walk.
//   multi_leaf_step  tri_test against (tmin, tmax), then the list's acceptance: count < K, or (t, prim) below the K-th key.
//   node step        pt_path.h's trav_node_step, unchanged.  It prunes against tv.tbest, which is the K-th t once the list is full and
//                    tmax before (always tmax under ALL, which counts every hit and so cannot prune); its "<=" admits a box that starts
//                    exactly at the bound, which a candidate at the K-th t with a lower prim needs.
//   multi_finish     turns the keys into records in place, from the last to the first (record j covers keys 2j and 2j + 1, both read
//                    before), through query_hit on a Trav per key: the bits are the closest query's by construction.  A triangle's
//                    barycentrics are not kept in the key: tri_test on the same ray and record gives them again, bit for bit.
// The slice is read and written as Word4 only (pt_word4.h, with key_less, the order of two keys), keys and records alike, so nothing is
// accessed through two types.
// Used by the query kernel (querykernel.hip) and by its CPU mirror (tests/hostsim/multihitsim.cpp).
#pragma once
#include "pt_query.h"
#include "pt_word4.h"

namespace pt {

enum { MULTI_COUNT_ALL = 1 };
constexpr int kMultiMaxHits = 64;

struct HitList {
  Word4* e;         // the ray's K records; while walking, its K keys (t, prim, tri, 0), ascending
  int K;            // 0 = count only (ALL)
  int count;        // keys kept: min(K, total)
  int total;        // |H| so far
  float tK; int primK;      // the K-th key, valid when full() and K > 0

  PT_HD void init(Word4* slice, int k) { e = slice; K = k; count = 0; total = 0; tK = 0.f; primK = -1; }
  PT_HD bool full() const { return count == K; }
  PT_HD bool accepts(float t, int prim) const { return count < K || (K > 0 && key_less(t, prim, tK, primK)); }
  // a member of H: counted, and kept if it is among the K least so far
  PT_HD void insert(float t, int prim, int tri) {
    total++;
    if (!accepts(t, prim)) return;
    int j = count < K ? count : K - 1;      // the slot that opens: the list grows, or its last key drops out
    while (j > 0) {
      const Word4 p = e[j - 1];
      if (!key_less(t, prim, i2f((int32_t)p.x), (int32_t)p.y)) break;
      e[j] = p; j--;
    }
    e[j] = mkw4((uint32_t)f2i(t), (uint32_t)prim, (uint32_t)tri, 0u);
    if (count < K) count++;
    if (count == K) { const Word4 l = e[K - 1]; tK = i2f((int32_t)l.x); primK = (int32_t)l.y; }
  }
};

// The bound the node step prunes against.
template <bool ALL>
PT_HD float multi_bound(const PathState& ps, const HitList& hl) { return (!ALL && hl.K > 0 && hl.full()) ? hl.tK : ps.tmax; }

// The brute-force lists in trav_begin's order, then the set-up of the BVH walk.  valid = query_ray's verdict.
template <bool ALL>
PT_HD void multi_begin(const SceneView& sc, const PathState& ps, bool valid, Trav& tv, HitList& hl) {
  if (!valid) { query_miss(ps, tv); return; }
  tv.bestPrim = -1; tv.bestTri = -1; tv.beta = 0.f; tv.gamma = 0.f;
  tv.inv = mk3(slab_inv(ps.d.x), slab_inv(ps.d.y), slab_inv(ps.d.z));
  tv.noi = neg_o_inv(ps.o, tv.inv);
  tv.sp = 0; tv.started = 1;
  for (int i = 0; i < sc.nSpheres; i++) {
    const DevSphere s = load_uniform(sc.spheres + i);
    float t1, t2;
    if (sphere_roots(s.center, s.radius, ps.o, ps.d, t1, t2)) {
      if ((t1 > ps.tmin) & (t1 < ps.tmax)) hl.insert(t1, i, -1);
      if ((t2 > ps.tmin) & (t2 < ps.tmax) & (t2 != t1)) hl.insert(t2, i, -1);
    }
  }
  for (int i = 0; i < sc.nQuads; i++) {
    const DevQuad q = load_uniform(sc.quads + i);
    float t;
    if (quad_test(q.plane, q.v1, q.v2, q.anchor, ps.o, ps.d, ps.tmin, ps.tmax, t)) hl.insert(t, sc.nSpheres + i, -1);
  }
  tv.tbest = multi_bound<ALL>(ps, hl);
  tv.node = sc.rootRef == kEmptyRef ? kTravDone : sc.rootRef;
}

// One leaf for a lane with tv.node < 0: every triangle the ray meets inside (tmin, tmax) goes to the list.
template <bool ALL, class Stack>
PT_HD void multi_leaf_step(const SceneView& sc, const PathState& ps, Trav& tv, Stack& st, HitList& hl) {
  const int first = leaf_first(tv.node), count = leaf_count(tv.node);
  const int triBase = sc.nSpheres + sc.nQuads;
  for (int base = 0; base < count; base += 4) {
    LeafChunk ch;
    leaf_fetch4(sc, tv.node, base, ch);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 4; j++) {
      v3 n; float t, be, ga;
      if (base + j < count && tri_test(ps.o, ps.d, ps.tmin, ps.tmax, ch.p0[j], ch.e0[j], ch.e1[j], n, t, be, ga))
        hl.insert(t, triBase + ch.prim[j], first + base + j);
    }
  }
  tv.tbest = multi_bound<ALL>(ps, hl);
  trav_pop(tv, st);
}

// One traversal step for a lane with tv.node != kTravDone (if-if form, as query_step).
template <bool ALL, bool N64, class Stack>
PT_HD void multi_step(const SceneView& sc, const PathState& ps, Trav& tv, Stack& st, HitList& hl, Counters& ct) {
  if (tv.node >= 0) trav_node_step<false, N64>(sc, ps, tv, st, ct);
  else multi_leaf_step<ALL>(sc, ps, tv, st, hl);
}

// The finished walk's records, in place of the keys: K moptix_hit records, the first hl.count from the keys, the rest miss records.
PT_HD void multi_finish(const SceneView& sc, const PathState& ps, const HitList& hl) {
  for (int j = hl.K - 1; j >= 0; j--) {
    Trav tv;
    query_miss(ps, tv);
    if (j < hl.count) {
      const Word4 k = hl.e[j];
      tv.tbest = i2f((int32_t)k.x); tv.bestPrim = (int32_t)k.y; tv.bestTri = (int32_t)k.z;
      if (tv.bestTri >= 0) {
        const Tri48 tp = load_const(at32(sc.tris, tv.bestTri));
        v3 n; float t;
        tri_test(ps.o, ps.d, ps.tmin, ps.tmax, tp.p0, tp.e0, tp.e1, n, t, tv.beta, tv.gamma);
      }
    }
    QueryHit h;
    query_hit(sc, ps, tv, h);
    hl.e[2 * j] = mkw4((uint32_t)f2i(h.t), (uint32_t)h.prim, (uint32_t)h.mat, (uint32_t)f2i(h.u));
    hl.e[2 * j + 1] = mkw4((uint32_t)f2i(h.v), (uint32_t)f2i(h.ng[0]), (uint32_t)f2i(h.ng[1]), (uint32_t)f2i(h.ng[2]));
  }
}

}  // namespace pt
