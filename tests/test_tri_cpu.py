"""Triangle queries without a GPU: the CPU mirror of the triangle query kernel (tests/trisim/trisim.cpp: pt_tri.h compiled for the host, on
the host mirror of the builder's tree) against the definition -- a loop over every primitive record through its predicate --, against an
exact integer evaluation on a half-integer grid, against a binary64 distance and penetration on the scenes' query sets, and against
answers known from the geometry; Context.self_intersections behind the mirror; the shipped kernel's registers."""
import os
import re
import sys

import numpy as np
import pytest

import lbvh_cases
from common import M, HostsimHandle, REPO, hostsim_bvh
from point_helpers import point_case
from sign_helpers import mesh_scene, torus
from tri_helpers import (BOX_ANY, BOX_COUNT, Geometry, MirrorContext, csr, fractions_of, largest_intermediate, membership, mesh_hs, pair_scale,
                         penetration64, predicate, pushed_torus, quad_triangles, same_bits, scene_extent, tri_dist64, tri_sets,
                         tri_stack_depth, tri_tri_dist64, tri_tri_exact, tribrute, tribrute_list, trisim, trisim_list, valid_tris,
                         zero_area64, zero_area_exact)

K = M._capi
SMALL = ["torus", "cornell_quads", "spheres", "offset"]
NAMES = SMALL + ["case:" + n for n in lbvh_cases.CASE_NAMES]
IDS = [n.replace("case:", "") for n in NAMES]
COFFEE = "file:coffee"
# tau: the smallest value for which, on the four small scenes' query sets, every pair the mirror reports has d <= tau x s and every pair it
# does not report has p <= tau x s (d the binary64 distance between the two, p the binary64 penetration over the axis list, s the pair's
# scale: its largest |coordinate| plus its largest extent).  Measured by test_predicates_against_binary64, which prints it per scene:
# 1.12e-8 (the torus, a reported pair's d; 4.56e-9 on cornell_quads, 6.68e-9 on spheres, 0 on offset; profiles/r33_tri.txt section 4).  The
# test holds four times that, the sweep tests' margin.  The binary64 side starts from the scene's original vertices; the predicate takes the record's
# v1 = p0 + e0 and v2 = p0 - e1, each up to an ulp away from them, and rounds v - a once more.
TAU = 1.12e-8
TOL = 4 * TAU


def _small_scene(which):
    if which == "torus":
        return mesh_scene("torus")
    if which == "offset":
        return lbvh_cases.case_scene("offset")
    return M.HostScene(which, 64, 36)


class Case:
    """A scene with its geometry, its leaf-4 mirror handle, its query set and the definition's answer -- counts and the CSR list of
    exact capacities -- computed once and only read afterwards.  On coffee the loop over 168,196 primitives runs on a subsample: every
    24th query, and the special ones."""

    def __init__(self, name):
        self.name = name
        if name in SMALL:
            self.hs = _small_scene(name)
            self.geo = Geometry(self.hs)
            self.lo, self.hi = scene_extent(self.geo) if name in ("cornell_quads", "spheres") else self.geo.box()
            self.sim = HostsimHandle(self.hs, 4)
        else:
            pc = point_case(name)
            self.hs, self.geo, self.lo, self.hi, self.sim = pc.hs, pc.geo, pc.lo, pc.hi, pc.sim
        self.tris, self.parts = tri_sets(self.geo, self.lo, self.hi)
        n = len(self.tris)
        self.n_prims = self.geo.ns + self.geo.nq + self.geo.nt
        sp = self.parts["special"]
        self.rows = np.unique(np.concatenate([np.arange(0, n, 24), np.arange(sp.start, sp.stop)])) if name == COFFEE else np.arange(n)
        self._brute = None
        self._walk = ()

    def brute(self):
        """(counts, prims, offsets) of the definition on rows."""
        if self._brute is None:
            b = self.tris[self.rows]
            counts = tribrute(self.sim, b, "count")
            prims, c2 = tribrute_list(self.sim, b, csr(counts))
            assert same_bits(c2, counts) and same_bits((counts > 0).astype(np.int32), tribrute(self.sim, b, "any"))
            self._brute = (counts, prims, csr(counts))
        return self._brute

    def walk(self):
        """(any, counts, prims) of the leaf-4 walk of the 64-byte nodes on the full set."""
        if not self._walk:
            counts = trisim(self.sim, self.tris, "count")
            self._walk = (trisim(self.sim, self.tris, "any"), counts, trisim_list(self.sim, self.tris, csr(counts))[0])
        return self._walk


_made = {}


def case_of(name):
    if name not in _made:
        _made[name] = Case(name)
    return _made[name]


# ---- 1: the walk is the definition ----
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("leaf", [1, 4, 8])
@pytest.mark.parametrize("name", NAMES, ids=IDS)
def test_walk_equals_the_loop_over_every_primitive(name, leaf, fmt):
    """trisim_query's and trisim_list's bytes are trisim_brute's, whole buffers: any, count and the list at exact capacities, no query
    excluded."""
    c = case_of(name)
    want_c, want_p, want_off = c.brute()
    sim = HostsimHandle(c.hs, leaf)
    try:
        anyone, counts = trisim(sim, c.tris, "any", fmt), trisim(sim, c.tris, "count", fmt)
        assert anyone.dtype == np.int32 and counts.dtype == np.int32
        assert same_bits(counts[c.rows], want_c), np.where(counts[c.rows] != want_c)[0][:8]
        assert same_bits(anyone, (counts > 0).astype(np.int32))
        prims, lc = trisim_list(sim, c.tris[c.rows], want_off, fmt)
        assert same_bits(lc, want_c) and same_bits(prims, want_p)
    finally:
        sim.close()


def test_walk_equals_the_loop_on_coffee():
    """The benchmark scene, leaf 4, both node forms: the definition on Case.rows, any / count / list."""
    c = case_of(COFFEE)
    want_c, want_p, want_off = c.brute()
    for fmt in (64, 128):
        counts = trisim(c.sim, c.tris, "count", fmt)
        assert same_bits(counts[c.rows], want_c) and same_bits(trisim(c.sim, c.tris, "any", fmt), (counts > 0).astype(np.int32))
        prims, lc = trisim_list(c.sim, c.tris[c.rows], want_off, fmt)
        assert same_bits(lc, want_c) and same_bits(prims, want_p)


def test_tri_sets_have_every_kind_of_query():
    """What the sets are for: queries that meet nothing, one, a few and many primitives, in every part; the invalid ones are invalid."""
    c = case_of("case:counts_2049")
    counts = c.brute()[0]
    assert 1500 <= len(c.tris) <= 1700
    assert (counts == 0).sum() > 100 and (counts == 1).sum() > 10 and ((counts > 1) & (counts < 64)).sum() > 50
    for part in ("faces", "own", "random", "slivers", "segments", "points"):
        assert (counts[c.parts[part]] > 0).sum() >= 10, part
    assert not counts[c.parts["far"]].any()
    valid = valid_tris(c.tris)
    assert valid[:c.parts["invalid"].start].all() and not valid[c.parts["invalid"]].any()
    assert counts[c.parts["whole"]] > 0 and not counts[c.parts["invalid"]].any()
    t = c.tris.reshape(-1, 3, 3)
    assert zero_area64(t[c.parts["points"]]).all() and zero_area64(t[c.parts["segments"]])[:3].all()


# ---- 2: exact on a grid ----
def _ints(t):
    return [tuple(int(x) for x in v) for v in t]


def _structured_pairs():
    """(query, triangle, what the geometry says) in units of 1/2."""
    T = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]                                            # the triangle (0,0,0) (2,0,0) (0,2,0)
    return [
        ("shared vertex", [(0, 0, 0), (-4, 0, 2), (0, -4, 2)], T, True),
        ("shared edge", [(0, 0, 0), (4, 0, 0), (2, -2, 4)], T, True),
        ("shared edge, coplanar", [(0, 0, 0), (4, 0, 0), (2, -4, 0)], T, True),
        ("identical", T, T, True),
        ("coplanar overlapping", [(1, 1, 0), (6, 1, 0), (1, 6, 0)], T, True),
        ("coplanar, one inside the other", [(1, 1, 0), (2, 1, 0), (1, 2, 0)], T, True),
        ("coplanar touching at a vertex", [(4, 0, 0), (8, 0, 0), (8, 4, 0)], T, True),
        ("coplanar touching at an edge point", [(2, 2, 0), (6, 2, 0), (2, 6, 0)], T, True),
        ("coplanar touching along an edge", [(0, 0, 0), (0, 4, 0), (-4, 0, 0)], T, True),
        ("coplanar disjoint", [(5, 0, 0), (8, 0, 0), (8, 4, 0)], T, False),
        ("coplanar disjoint beyond the hypotenuse", [(3, 2, 0), (6, 2, 0), (3, 6, 0)], T, False),
        ("parallel planes", [(0, 0, 1), (4, 0, 1), (0, 4, 1)], T, False),
        ("piercing through the other's edge", [(2, 0, -2), (2, 0, 2), (2, -4, 0)], T, True),
        ("piercing the interior", [(1, 1, -2), (1, 1, 2), (8, 8, 2)], T, True),
        ("passing beside", [(6, 6, -2), (6, 6, 2), (8, 8, 2)], T, False),
        ("box overlaps, planes cross outside", [(3, 3, -1), (4, 4, 1), (4, 3, 1)], T, False),
        ("a segment through the interior", [(1, 1, -2), (1, 1, 2), (1, 1, 2)], T, True),
        ("a segment ending on the face", [(1, 1, 0), (1, 1, 4), (1, 1, 0)], T, True),
        ("a segment in the plane, across", [(-2, 1, 0), (6, 1, 0), (-2, 1, 0)], T, True),
        ("a segment in the plane, inside", [(1, 1, 0), (2, 1, 0), (2, 1, 0)], T, True),
        ("a segment in the plane, outside", [(3, 2, 0), (6, 2, 0), (6, 2, 0)], T, False),
        ("a segment above the face", [(1, 1, 1), (2, 1, 1), (2, 1, 1)], T, False),
        ("a collinear triple through an edge", [(2, -2, 0), (2, 0, 0), (2, 2, 0)], T, True),
        ("a point on the face", [(1, 1, 0)] * 3, T, True),
        ("a point on an edge", [(2, 2, 0)] * 3, T, True),
        ("a point on a vertex", [(0, 4, 0)] * 3, T, True),
        ("a point off the face, in the plane", [(3, 2, 0)] * 3, T, False),
        ("a point above the face", [(1, 1, 1)] * 3, T, False),
    ]


def test_predicate_is_exact_on_a_half_integer_grid():
    """Vertices on the half-integer grid with |coordinate| <= 2: every binary32 intermediate of the predicate is an integer multiple of 2^-4
    below 2^20 (largest_intermediate, on integers: asserted below 2^24), so the predicate is the exact SAT over its axes.  Where at least one
    of the two triangles has non-zero area it must equal tri_tri_exact, an integer evaluation without an axis list, on every pair,
    touching ones included; where both have zero area it must report every pair tri_tri_exact reports (one-sided).  120,000 random pairs --
    a third with one side drawn from a narrower grid, a sixth with a zero-area side --, every structured pair both ways and under the
    coordinate permutations and a reflection."""
    rng = np.random.default_rng(32)
    n = 120000
    Q, T = rng.integers(-4, 5, (n, 3, 3)), rng.integers(-4, 5, (n, 3, 3))
    Q[:n // 3] = rng.integers(-2, 3, (n // 3, 3, 3))                                # small queries: more contacts
    k = n // 3
    Q[k:k + n // 12, 2] = Q[k:k + n // 12, 1]                                       # segments
    Q[k + n // 12:k + n // 8] = Q[k + n // 12:k + n // 8, :1]                       # points
    T[k + n // 8:k + n // 6, 1] = T[k + n // 8:k + n // 6, 0]                       # zero-area primitives
    T[k:k + n // 48, 2] = T[k:k + n // 48, 0]                                       # both sides zero-area
    names, sq, st, sw = [], [], [], []
    perms = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1)]
    for label, q, t, want in _structured_pairs():
        for p in perms:
            for flip in (1, -1):
                for a, b in ((q, t), (t, q)):
                    names.append(label); sw.append(want)
                    sq.append(np.array(a)[:, p] * [flip, 1, 1]); st.append(np.array(b)[:, p] * [flip, 1, 1])
    Q, T = np.concatenate([np.array(sq), Q]), np.concatenate([np.array(st), T])
    assert np.abs(Q).max() <= 8 and np.abs(T).max() <= 8                            # the structured pairs reach |coordinate| 4
    worst = largest_intermediate(Q, T)
    assert worst < 2 ** 24, worst
    got = predicate("tri", (T * 0.5).reshape(-1, 9), (Q * 0.5).reshape(-1, 9))
    want = np.array([tri_tri_exact(_ints(q), _ints(t)) for q, t in zip(Q, T)])
    assert np.array_equal(want[:len(sw)], np.array(sw)), [names[i] for i in np.where(want[:len(sw)] != np.array(sw))[0]]
    both = np.array([zero_area_exact(_ints(q)) and zero_area_exact(_ints(t)) for q, t in zip(Q, T)])
    differ = (got != want) & ~both
    assert not differ.any(), (np.where(differ)[0][:8], [names[i] for i in np.where(differ[:len(sw)])[0]][:8])
    assert not (want & ~got & both).any(), np.where(want & ~got & both)[0][:8]
    print("tri exact grid: %d pairs (%d structured), largest intermediate %d (< 2^24), %d meet, %d with both sides of zero area (%d of them "
          "meet, %d reported)" % (len(Q), len(sw), worst, want.sum(), both.sum(), (want & both).sum(), (got & both).sum()))
    assert 0.1 < want.mean() < 0.9 and both.sum() > 1000 and (want & both).sum() > 10


# ---- 3: binary64 on real geometry ----
def _measure(hs, geo, tris):
    """(worst d / s over reported pairs, worst p / s over unreported pairs, pairs, reported) of the definition's loop on valid queries
    against every primitive.  Triangles and quads: d = tri_tri_dist64, p = penetration64 (a quad: the lesser d, the larger p of its two
    triangles); spheres: d = max(dmin - r, r - dmax, 0), p = min(r - dmin, dmax - r).  Reported pairs of two zero-area triangles are left
    out: for them the predicate is a superset by contract.  An unreported pair without any axis of non-zero length (two points, collinear
    segments) has p = -d where the two are apart and +inf, a failure, where they are not."""
    tris = tris[valid_tris(tris)]
    q = tris.reshape(-1, 3, 3).astype(np.float64)
    n_prims = geo.ns + geo.nq + geo.nt
    counts = tribrute(hs, tris, "count")
    prims, _ = tribrute_list(hs, tris, csr(counts))
    got = membership(prims, csr(counts), n_prims)
    qi, pi = np.meshgrid(np.arange(len(q)), np.arange(n_prims), indexing="ij")
    qi, pi = qi.ravel(), pi.ravel()
    rep = got.ravel()
    d = np.zeros(len(qi)); p = np.zeros(len(qi)); s = np.ones(len(qi)); skip = np.zeros(len(qi), bool)
    for i in range(geo.ns):
        m = pi == i
        dmin = tri_dist64(np.repeat(geo.centre[i][None], m.sum(), axis=0), q[qi[m]])[0]
        dmax = np.linalg.norm(q[qi[m]] - geo.centre[i], axis=2).max(axis=1)
        r = geo.radius[i]
        d[m], p[m] = np.maximum(np.maximum(dmin - r, r - dmax), 0.0), np.minimum(r - dmin, dmax - r)
        ball = np.concatenate([q[qi[m]], np.broadcast_to(np.array([geo.centre[i] - r, geo.centre[i] + r]), (m.sum(), 2, 3))], axis=1)
        s[m] = np.abs(ball).max(axis=(1, 2)) + (ball.max(axis=1) - ball.min(axis=1)).max(axis=1)
    for i in range(geo.nq):
        m = pi == geo.ns + i
        two = quad_triangles(geo, i)
        ta, tb = np.broadcast_to(two[0], (m.sum(), 3, 3)), np.broadcast_to(two[1], (m.sum(), 3, 3))
        d[m] = np.minimum(tri_tri_dist64(q[qi[m]], ta), tri_tri_dist64(q[qi[m]], tb))
        p[m] = np.maximum(penetration64(q[qi[m]], ta), penetration64(q[qi[m]], tb))
        s[m] = np.maximum(pair_scale(q[qi[m]], ta), pair_scale(q[qi[m]], tb))
    m = pi >= geo.ns + geo.nq
    if m.any():
        t = geo.tri[pi[m] - geo.ns - geo.nq]
        far = ~rep[m]                                          # the distance is needed for reported pairs only
        dd = np.zeros(m.sum())
        dd[~far] = tri_tri_dist64(q[qi[m]][~far], t[~far])
        pp = penetration64(q[qi[m]], t)
        none = np.isinf(pp)                                    # two points, or collinear segments: no axis at all.  Apart: fine; else a miss
        if none.any():
            dn = tri_tri_dist64(q[qi[m]][none], t[none])
            pp[none] = np.where(dn > 0, -dn, np.inf)
        d[m], p[m], s[m] = dd, pp, pair_scale(q[qi[m]], t)
        skip[m] = zero_area64(q[qi[m]]) & zero_area64(t)
    use_rep, use_not = rep & ~skip, ~rep
    worst_d = float((d[use_rep] / s[use_rep]).max()) if use_rep.any() else 0.0
    worst_p = float((p[use_not] / s[use_not]).max()) if use_not.any() else 0.0
    return worst_d, worst_p, len(qi), int(rep.sum())


@pytest.mark.parametrize("which", SMALL)
def test_predicates_against_binary64(which):
    """Every valid query of the scene's set against every primitive, the mirror's S from the definition's loop over the records: a reported
    pair must have d <= TOL x s, an unreported one p <= TOL x s, with TOL four times the measured tau (printed here per scene)."""
    c = case_of(which)
    worst_d, worst_p, pairs, reported = _measure(c.hs, c.geo, c.tris)
    print("tri64 %-14s %d pairs, %d reported: worst d / s of a reported pair %.3g, worst p / s of an unreported pair %.3g: tau %.3g" % (
        which, pairs, reported, worst_d, worst_p, max(worst_d, worst_p)))
    assert reported > 500 and pairs - reported > 1000
    assert worst_d <= TOL and worst_p <= TOL, (worst_d, worst_p)


# ---- 4: the contract ----
def test_invalid_queries_meet_nothing():
    c = case_of("torus")
    whole = c.tris[c.parts["whole"]]
    assert trisim(c.sim, whole[None], "count")[0] > 0
    bad = []
    for k in range(9):
        for v in (np.nan, np.inf, -np.inf):
            r = whole.copy(); r[k] = v; bad.append(r)
    bad = np.concatenate([np.array(bad, np.float32), c.tris[c.parts["invalid"]]])
    assert not valid_tris(bad).any()
    for fmt in (64, 128):
        assert not trisim(c.sim, bad, "any", fmt).any() and not trisim(c.sim, bad, "count", fmt).any()
        prims, counts = trisim_list(c.sim, bad, np.arange(len(bad) + 1) * 3, fmt)
        assert not counts.any() and (prims == -1).all()
    assert not tribrute(c.sim, bad, "count").any()
    spheres = M.HostScene("spheres", 64, 36)                            # the brute-force lists in front of the walk too
    assert not trisim(spheres, bad, "count").any()


def test_empty_batch():
    hs = M.HostScene("spheres", 64, 36)
    assert len(trisim(hs, np.zeros((0, 9), np.float32), "count")) == 0
    prims, counts = trisim_list(hs, np.zeros((0, 9), np.float32), [0])
    assert len(prims) == 0 and len(counts) == 0
    assert K.device_lib().moptix_query_tris(None, None, 0, 0, None) == K.ERR_INVALID      # no context; with one, n == 0 is MOPTIX_OK (GPU tests)


def test_a_query_equal_to_a_face_finds_it_and_every_face_sharing_a_vertex():
    ts = mesh_scene("torus")
    v, f = torus()
    tri = v.astype(np.float32)[f]
    for k in (0, 100, 333, 575):
        sharing = np.where((f[:, :, None] == f[k][None, None, :]).any(axis=(1, 2)))[0]
        assert k in sharing and len(sharing) >= 12
        for order in ((0, 1, 2), (1, 2, 0), (2, 1, 0)):
            q = tri[k][list(order)].reshape(1, 9)
            count = trisim(ts, q, "count")
            prims, lc = trisim_list(ts, q, csr(count))
            assert same_bits(lc, count) and set(sharing) <= set(prims.tolist()), (k, order)


def test_coincident_triangles_list_in_face_order():
    from pointmulti_helpers import duplicates_scene
    hs = duplicates_scene()
    tri = Geometry(hs).tri
    assert hs.sizes.nSpheres == 0 and hs.sizes.nQuads == 0
    ctr = tri[0].mean(axis=0)
    cut = np.stack([tri[0], 0.5 * (tri[0] - ctr) + ctr + 0.0]).reshape(2, 9)      # the face itself, and a smaller copy inside it
    for leaf in (1, 4, 8):
        sim = HostsimHandle(hs, leaf)
        try:
            for fmt in (64, 128):
                prims, counts = trisim_list(sim, cut, [0, 100, 200], fmt)
                assert (counts >= 100).all() and np.array_equal(prims[:100], np.arange(100)) and np.array_equal(prims[100:], np.arange(100))
        finally:
            sim.close()


def test_triangle_inside_a_sphere_or_inside_the_torus_tube_meets_nothing():
    hs = M.HostScene("spheres", 64, 36)
    geo = Geometry(hs)
    i = int(np.argmin(geo.radius))
    ctr, r = geo.centre[i], geo.radius[i]
    assert not [j for j in range(geo.ns) if j != i and np.linalg.norm(geo.centre[j] - ctr) < geo.radius[j]]
    shape = np.array([[0.5, 0.0, 0.1], [-0.3, 0.4, 0.0], [-0.2, -0.4, -0.2]])
    inside = (ctr + 0.9 * r * shape).reshape(1, 9)                                   # the furthest vertex is 0.46 r from the centre
    assert trisim(hs, inside, "count")[0] == 0 and tribrute(hs, inside, "count")[0] == 0
    through = (ctr + 3.0 * r * shape).reshape(1, 9)                                  # its vertices are outside, its middle inside
    prims, counts = trisim_list(hs, through, [0, 4])
    assert counts[0] >= 1 and i in prims[:counts[0]]
    # the torus (R = 1, r = 0.4 about the z axis): a triangle in the tube's interior meets no face, one through the tube's wall does
    ts = mesh_scene("torus")
    tube = (np.array([1.0, 0.0, 0.0]) + 0.2 * shape).reshape(1, 9)
    hole = (0.3 * shape).reshape(1, 9)
    wall = np.array([[1.0, 0.0, 0.0], [1.6, 0.1, 0.0], [1.6, -0.1, 0.1]]).reshape(1, 9)
    assert trisim(ts, tube, "count")[0] == 0 and trisim(ts, hole, "any")[0] == 0 and trisim(ts, wall, "count")[0] > 0


@pytest.mark.parametrize("name", SMALL + ["case:degenerate", "case:mixed"], ids=SMALL + ["degenerate", "mixed"])
def test_any_count_and_list_agree(name):
    """any == (count > 0); lists ascend, hold distinct ids in range and have the count's length; a larger capacity is padded with -1, a
    smaller one is -1 throughout with the true count, a zero capacity writes nothing."""
    c = case_of(name)
    anyone, counts, prims = c.walk()
    assert np.array_equal(anyone, (counts > 0).astype(np.int32))
    off = csr(counts)
    assert (prims >= 0).all() and (prims < c.n_prims).all()
    inner = np.ones(len(prims), bool); inner[off[:-1][counts > 0]] = False          # not the first id of a slice
    assert (np.diff(prims)[inner[1:]] > 0).all()
    sel = np.arange(len(c.tris))
    b, n = c.tris[sel], counts[sel].astype(np.int64)
    for fmt in (64, 128):
        for label, cap in (("larger", n + 3), ("smaller", np.maximum(n - 1, 0)), ("zero", np.zeros_like(n)), ("fixed 4", np.full_like(n, 4))):
            o = csr(cap)
            p, got = trisim_list(c.sim, b, o, fmt)
            assert same_bits(got, counts[sel]), label
            assert not (p == -7).any(), label                                         # every byte of every slice is defined
            for i in np.where(cap > 0)[0][::max(1, len(sel) // 200)]:
                s = p[o[i]:o[i + 1]]
                if n[i] <= cap[i]:
                    assert np.array_equal(s[:n[i]], prims[off[sel[i]]:off[sel[i] + 1]]) and (s[n[i]:] == -1).all(), (label, i)
                else:
                    assert (s == -1).all(), (label, i)


@pytest.mark.parametrize("name", [COFFEE, "case:mixed", "case:geometric"], ids=["coffee", "mixed", "geometric"])
def test_stack_depth_is_within_the_trees_bound(name):
    c = case_of(name)
    depth = hostsim_bvh(c.sim)[4]
    for fmt in (64, 128):
        for mode in ("any", "count"):
            d = tri_stack_depth(c.sim, c.tris, mode, fmt)
            assert d <= 3 * depth + 1, (fmt, mode, d, depth)
            if name == COFFEE and mode == "count":
                assert d > 16, d              # more than the kernel keeps in LDS: its overflow columns are in use on this set


def test_symbols_and_host_side_argument_checks():
    names = {"moptix_query_tris", "moptix_query_tris_device", "moptix_query_tris_list", "moptix_query_tris_list_device"}
    header = open(os.path.join(REPO, "include", "moptix.h")).read()
    assert names <= set(re.findall(r"\bint (moptix_[a-z0-9_]+)\s*\(", header))
    assert "Not offered: query triangles" not in header and "moptix_query_tris*" in header
    assert names <= set(K.DEVICE_SYMBOLS) and K.BOX_ANY == BOX_ANY == 0 and K.BOX_COUNT == BOX_COUNT == 1
    lib = K.device_lib()
    assert all(hasattr(lib, n) for n in names)
    assert "query_tris" in dir(M.Context) and "self_intersections" in dir(M.Context)
    assert lib.moptix_query_tris(None, None, 0, 0, None) == K.ERR_INVALID
    assert lib.moptix_query_tris_device(None, None, 0, 0, None) == K.ERR_INVALID
    assert lib.moptix_query_tris_list(None, None, 0, None, None, None) == K.ERR_INVALID
    assert lib.moptix_query_tris_list_device(None, None, 0, None, None, None) == K.ERR_INVALID
    blank = object.__new__(M.Context)                                  # mode, max_prims and the shape are refused before the context is looked at
    b = np.zeros((4, 9), np.float32)
    for kw in (dict(mode="closest"), dict(mode="count", max_prims=4), dict(mode="list", max_prims=-1)):
        with pytest.raises(ValueError):
            M.Context.query_tris(blank, b, **kw)
    for bad in (b.reshape(-1), b[:, :8], np.zeros((4, 6), np.float32), np.zeros((4, 3, 4), np.float32)):
        with pytest.raises(ValueError):
            M.Context.query_tris(blank, bad)
    for v, f in ((np.zeros((4, 2), np.float32), np.zeros((2, 3), np.int64)), (np.zeros((4, 3), np.float32), np.zeros((2, 4), np.int64)),
                 (np.zeros((4, 3), np.float32), np.zeros((2, 3), np.float32))):
        with pytest.raises(ValueError):
            M.Context.self_intersections(blank, v, f)


# ---- 5: self_intersections, the Python-level pairing behind the mirror ----
def test_self_intersections_of_a_closed_torus_are_none():
    v, f = torus()
    ctx = MirrorContext(M, mesh_scene("torus"))
    pairs = ctx.self_intersections(v.astype(np.float32), f)
    assert pairs.shape == (0, 2) and pairs.dtype == np.int64
    assert ctx.self_intersections(v.astype(np.float32), f, max_prims=64).shape == (0, 2)
    with pytest.raises(ValueError):
        ctx.self_intersections(v.astype(np.float32), f, max_prims=4)      # a face meets itself and at least twelve neighbours


def test_self_intersections_of_a_pushed_torus_are_the_exact_ones():
    """One vertex of the outer equator pushed through the hole into the opposite wall: the pairs are exactly those tri_tri_exact finds on
    the same binary32 vertices among the pairs of faces without a common vertex index; sorted, unique, i < j, no neighbours."""
    v, f = pushed_torus(2.2)
    ctx = MirrorContext(M, mesh_hs(v, f))
    pairs = ctx.self_intersections(v, f)
    exact = [fractions_of(v[face]) for face in f]
    lo, hi = v[f].min(axis=1), v[f].max(axis=1)
    want = []
    for i in range(len(f)):
        near = np.where((lo[i] <= hi).all(axis=1) & (hi[i] >= lo).all(axis=1))[0]
        for j in near[near > i]:
            if not set(f[i]) & set(f[j]) and tri_tri_exact(exact[i], exact[j]):
                want.append((i, int(j)))
    want = np.array(sorted(want), np.int64).reshape(-1, 2)
    print("self_intersections: %d pairs on the pushed torus" % len(want))
    assert len(want) >= 8
    assert np.array_equal(pairs, want), (pairs[:8], want[:8])
    assert (pairs[:, 0] < pairs[:, 1]).all() and len(np.unique(pairs, axis=0)) == len(pairs)
    assert not any(set(f[i]) & set(f[j]) for i, j in pairs)
    one_way = set()                                                      # either direction alone is within the symmetric result
    prims, off = ctx.query_tris(v[f], "list")
    for i in range(len(f)):
        one_way |= {(min(i, int(j)), max(i, int(j))) for j in prims[off[i]:off[i + 1]] if not set(f[i]) & set(f[int(j)])}
    assert one_way == set(map(tuple, pairs.tolist()))
    assert np.array_equal(ctx.self_intersections(v, f, max_prims=64), pairs)
    assert np.array_equal(ctx.self_intersections(v.astype(np.float64), f.astype(np.int32)), pairs)      # other dtypes of the same mesh


# ---- 6: the shipped kernel's registers ----
def test_triangle_kernel_resources_are_pinned():
    """tools/kernel_resources.py on the six pt_triquery<MODE, N64> instantiations of the shipped library: no spilled vector registers, no
    private segment, and the VGPR counts of profiles/r33_tri.txt section 1 (at most 128: four waves per SIMD)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from kernel_resources import kernel_resources
    res = kernel_resources(os.path.join(REPO, "minimaloptix_amd", "lib", "libmoptix.so"))
    got = {}
    for k, v in res.items():
        m = re.search(r"pt_triqueryILi(\d)ELb(\d)E", k)
        if m:
            got[(int(m.group(1)), int(m.group(2)))] = v
    assert sorted(got) == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)], sorted(res)[:5]
    for key, r in got.items():
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (key, r)
        assert r["group_segment_fixed_size"] == 16384, (key, r)
    assert {k: r["vgpr_count"] for k, r in got.items()} == {(0, 0): 109, (0, 1): 107, (1, 0): 109, (1, 1): 109, (2, 0): 120, (2, 1): 120}
