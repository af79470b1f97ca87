"""Frustum queries without a GPU: the CPU mirror of the frustum kernel (tests/frustumsim/frustumsim.cpp: pt_frustum.h compiled for the
host, on the host mirror of the builder's tree) against the definition -- a loop over every primitive record through its predicate --,
against exact rationals (Sutherland-Hodgman on the float inputs), against the box queries on the six planes of a box, against the
renderer's own primary rays, and against answers known from the geometry."""
import copy
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import box_helpers
import lbvh_cases
from aov_helpers import camera_rays
from common import M, HostsimHandle, MovedScene, REPO, hostsim_bvh
from frustum_helpers import (A, BOX_ANY, BOX_COUNT, E, R, STAGES, V, Geometry, aabb_planes, box_planes, csr, frustum_sets, frustum_stack_depth,
                             frustum_work, frustumbrute, frustumbrute_list, frustumsim, frustumsim_list, membership, pack, pair_scale,
                             perspective, predicate, predicate_pairs, random_rotations, same_bits, scale_planes, scene_camera, scene_extent,
                             smallest_tau, through, tiles, tri_region_exact, valid_frusta)
from point_helpers import point_case
from query_helpers import SCENES, querysim
from refit_helpers import RefitSim, moved_faces
from sign_helpers import mesh_scene

K = M._capi
NAMES = [k for k, _ in SCENES] + ["case:" + n for n in lbvh_cases.CASE_NAMES]
IDS = [n.replace("file:", "").replace("case:", "") for n in NAMES]
COFFEE = "file:coffee"
# The smallest tau at which "exact on the region shrunk by tau => predicate" and "predicate => exact on the region grown by tau" both hold
# for the mirror on predicate_pairs' 5,400 pairs, relative to the pair's scale (frustum_helpers.pair_scale), measured by
# test_predicate_against_exact_rationals, is 5.71e-8: 195 pairs differ from the exact verdict at tau = 0, every one a touching pair that
# stage A accepts on a rounded s >= 0 (profiles/r31_frustum.txt section 5).  TAU is 4 x that, the box, oriented box and sweep tests' margin.
TAU_MEASURED = 5.71e-8
TAU = 4 * TAU_MEASURED


class Case:
    """A scene of the point tests (point_helpers.point_case: the scene, its geometry, its box, its leaf-4 mirror handle) with its frustum
    set and the definition's answer -- counts and the CSR list of exact capacities -- computed once and only read afterwards.  On coffee
    the loop over 168,196 primitives runs on 64 queries spread over the parts."""

    def __init__(self, name):
        self.name = name
        self.pc = point_case(name)
        self.frusta, self.parts = frustum_sets(self.pc.hs, self.pc.geo, self.pc.lo, self.pc.hi)
        n = len(self.frusta)
        self.n_prims = self.pc.geo.ns + self.pc.geo.nq + self.pc.geo.nt
        self.rows = np.unique(np.linspace(0, n - 1, 64).astype(int)) if name == COFFEE else np.arange(n)
        self._brute = None
        self._walk = ()

    def brute(self):
        """(counts, prims, offsets) of the definition on rows."""
        if self._brute is None:
            b = self.frusta[self.rows]
            counts = frustumbrute(self.pc.sim, b, "count")
            prims, c2 = frustumbrute_list(self.pc.sim, b, csr(counts))
            assert same_bits(c2, counts) and same_bits((counts > 0).astype(np.int32), frustumbrute(self.pc.sim, b, "any"))
            self._brute = (counts, prims, csr(counts))
        return self._brute

    def walk(self):
        """(any, counts, prims) of the leaf-4 walk of the 64-byte nodes on the full set."""
        if not self._walk:
            counts = frustumsim(self.pc.sim, self.frusta, "count")
            self._walk = (frustumsim(self.pc.sim, self.frusta, "any"), counts, frustumsim_list(self.pc.sim, self.frusta, csr(counts))[0])
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
    """frustumsim_query's and frustumsim_list's bytes are frustumsim_brute's, whole buffers: any, count and the list at exact capacities,
    no query excluded.  On coffee the definition covers Case.rows, and the walk of this tree is compared with the leaf-4 walk of the
    64-byte nodes on the full set besides."""
    c = case_of(name)
    want_c, want_p, want_off = c.brute()
    sim = HostsimHandle(c.pc.hs, leaf)
    try:
        anyone, counts = frustumsim(sim, c.frusta, "any", fmt), frustumsim(sim, c.frusta, "count", fmt)
        assert anyone.dtype == np.int32 and counts.dtype == np.int32
        assert same_bits(counts[c.rows], want_c), np.where(counts[c.rows] != want_c)[0][:8]
        assert same_bits(anyone, (counts > 0).astype(np.int32))
        prims, lc = frustumsim_list(sim, c.frusta[c.rows], want_off, fmt)
        assert same_bits(lc, want_c) and same_bits(prims, want_p)
        if name == COFFEE:
            ref_any, ref_c, ref_p = c.walk()
            full_p, full_c = frustumsim_list(sim, c.frusta, csr(ref_c), fmt)
            assert same_bits(anyone, ref_any) and same_bits(counts, ref_c) and same_bits(full_c, ref_c) and same_bits(full_p, ref_p)
    finally:
        sim.close()


@pytest.mark.parametrize("name", [COFFEE, "case:mixed"], ids=["coffee", "mixed"])
def test_walk_equals_the_loop_after_update_faces_and_refit(name):
    c = case_of(name)
    fp, _ = moved_faces(c.pc.hs, 0.02)
    rs = RefitSim(c.pc.hs, 4)
    try:
        rs.update(0, fp); rs.refit()
        b = c.frusta[c.rows]
        want = frustumbrute(rs._sim, b, "count")
        for fmt in (64, 128):
            got = frustumsim(rs._sim, c.frusta, "count", fmt)
            assert same_bits(got[c.rows], want), (fmt, np.where(got[c.rows] != want)[0][:8])
            prims, lc = frustumsim_list(rs._sim, b, csr(want), fmt)
            assert same_bits(lc, want) and same_bits(prims, frustumbrute_list(rs._sim, b, csr(want))[0])
        assert not same_bits(want, c.brute()[0])                        # the move changed the answer
    finally:
        rs.close()


def test_frustum_sets_have_every_kind_of_query():
    """What the sets are for: queries that meet nothing, one, a few and many primitives, in every part; the invalid ones are invalid."""
    c = case_of("case:counts_2049")
    counts = c.brute()[0]
    assert 800 <= len(c.frusta) <= 1100
    assert (counts == 0).sum() > 100 and ((counts > 0) & (counts < 64)).sum() > 50 and (counts >= 64).sum() > 10
    for part in ("tiles", "persp", "beams", "wedges", "slabs", "halves", "thin", "scaled"):
        assert (counts[c.parts[part]] > 0).sum() >= 5, part
    valid = valid_frusta(c.frusta)
    assert valid[:c.parts["invalid"].start].all() and not valid[c.parts["invalid"]].any()
    assert not counts[c.parts["invalid"]].any() and not counts[c.parts["empty"]].any() and not counts[c.parts["void"]].any()
    assert (counts[c.parts["zero"]] == c.n_prims).all()
    f = c.frusta.reshape(-1, 6, 4)
    assert ((f[c.parts["wedges"], :, :3] == 0).all(axis=2).sum(axis=1) == 4).all()
    assert ((f[c.parts["halves"], :, :3] == 0).all(axis=2).sum(axis=1) == 5).all()


# ---- 2: exact rationals ----
def test_predicate_against_exact_rationals():
    """predicate_pairs' 5,400 pairs through the mirror's triangle predicate and through tri_region_exact, which shares no code with the
    header.  Both implications at TAU: a pair the predicate rejects is not exact on the region shrunk by TAU x scale; a pair it accepts is
    exact on the region grown by TAU x scale.  The smallest tau that would do is measured and printed first."""
    tris, fr = predicate_pairs()
    assert len(tris) >= 5000
    got, stage = predicate("tri", tris.reshape(-1, 9), fr)
    mix = {STAGES[k]: int((stage == k).sum()) for k in np.unique(stage)}
    exact = np.array([tri_region_exact(tris[i], fr[i]) for i in range(len(tris))])
    differ = np.where(exact != got)[0]
    taus = np.array([smallest_tau(tris[i], fr[i], got[i]) for i in differ]) if len(differ) else np.zeros(0)
    print("frustum exact: %d pairs, decided by %s, %d accepted; %d differ from the exact verdict at tau = 0 (by stage %s), smallest tau / scale "
          "that reconciles all %.3g" % (len(tris), mix, int(got.sum()), len(differ),
                                        {STAGES[k]: int((stage[differ] == k).sum()) for k in np.unique(stage[differ])}, taus.max() if len(taus) else 0.0))
    degenerate = np.linalg.norm(np.cross(tris[:, 1].astype(np.float64) - tris[:, 0], tris[:, 2].astype(np.float64) - tris[:, 0]), axis=1) < 1e-6 * \
        np.abs(tris).max(axis=(1, 2)) ** 2
    reduced = (fr.reshape(-1, 6, 4)[:, :, :3] == 0).all(axis=2).any(axis=1)
    assert (degenerate | reduced).mean() >= 0.3
    assert mix["E"] >= 0.05 * len(tris) and mix["V"] >= 0.05 * len(tris), mix
    assert 0.2 < got.mean() < 0.8
    for i in differ:
        s = Fraction(TAU) * Fraction(pair_scale(tris[i], fr[i]))
        if got[i]:
            assert tri_region_exact(tris[i], fr[i], s), (i, STAGES[int(stage[i])])
        else:
            assert not tri_region_exact(tris[i], fr[i], -s), (i, STAGES[int(stage[i])])
    assert TAU_MEASURED <= 1e-6


# ---- 3: exact where the arithmetic is exact ----
def test_plane_stages_are_exact_on_an_integer_grid():
    """Integer normals |n| <= 4, integer d, vertices on a half-integer grid within +-16: every s_ji is an exact binary32 value, so every
    pair that R or A decides must equal the rational evaluation at tau = 0 -- touching ones, which A accepts, among them."""
    rng = np.random.default_rng(33)
    n = 4000
    planes = np.zeros((n, 6, 4))
    planes[:, :, :3] = rng.integers(-4, 5, (n, 6, 3))
    planes[:, :, 3] = rng.integers(-4, 25, (n, 6))
    planes[::5, 3:] = 0                                                  # three planes only
    planes[1::5, 1:, :3] = 0; planes[1::5, 1:, 3] = rng.integers(0, 3, (len(planes[1::5]), 5))       # a half-space
    ext = rng.choice([1, 2, 4, 8, 16], n)
    c = rng.integers(-8, 9, (n, 1, 3)) * 0.5
    tris = np.clip(c + rng.integers(-ext[:, None, None], ext[:, None, None] + 1, (n, 3, 3)) * 0.5, -16.0, 16.0).astype(np.float32)
    tris[::11, 1] = tris[::11, 0]
    fr = pack(planes)
    got, stage = predicate("tri", tris.reshape(-1, 9), fr)
    plane_decided = np.where((stage == R) | (stage == A))[0]
    assert len(plane_decided) >= 2000
    touching = 0
    for i in plane_decided:
        want = tri_region_exact(tris[i], fr[i])
        assert want == bool(got[i]), (i, STAGES[int(stage[i])])
        if want and not tri_region_exact(tris[i], fr[i], Fraction(-1, 1024)):
            touching += 1
    print("frustum exact grid: %d pairs, %d decided by R or A (%d R, %d A), %d of them touch" % (n, len(plane_decided), (stage == R).sum(), (stage == A).sum(), touching))
    assert touching >= 50 and (stage == A).sum() >= 200 and (stage == R).sum() >= 200
    # the rest is not claimed exact, but holds at TAU
    for i in np.where((stage != R) & (stage != A))[0][:400]:
        s = Fraction(TAU) * Fraction(pair_scale(tris[i], fr[i]))
        assert tri_region_exact(tris[i], fr[i], s) if got[i] else not tri_region_exact(tris[i], fr[i], -s), (i, STAGES[int(stage[i])])


# ---- 4: the box queries ----
@pytest.mark.parametrize("name", NAMES[:4], ids=IDS[:4])
def test_six_planes_of_a_box_against_the_box_queries(name):
    """The box tests' boxes as six planes (unit normals, the box's own floats) against the box queries' mirror on the same boxes: the
    triangles and quads in the two sets may differ only on pairs within 4 TAU of touching -- not exact on the box shrunk by that, exact on
    the box grown by it.  Every differing pair is checked.  Spheres are left out: the box queries test the surface, the frusta the ball."""
    pc = point_case(name)
    boxes, _ = box_helpers.box_sets(pc.geo, pc.lo, pc.hi)
    boxes = boxes[box_helpers.valid_boxes(boxes)]
    if name == COFFEE:
        boxes = boxes[::6]
    fr = aabb_planes(boxes)
    fc, bc = frustumsim(pc.sim, fr, "count"), box_helpers.boxsim(pc.sim, boxes, "count")
    fp, bp = frustumsim_list(pc.sim, fr, csr(fc))[0], box_helpers.boxsim_list(pc.sim, boxes, csr(bc))[0]
    fo, bo = csr(fc), csr(bc)
    ns, nq = pc.geo.ns, pc.geo.nq
    differing = both = 0
    for i in range(len(boxes)):
        a, b = fp[fo[i]:fo[i + 1]], bp[bo[i]:bo[i + 1]]
        a, b = a[a >= ns], b[b >= ns]
        both += len(np.intersect1d(a, b))
        for prim in np.setxor1d(a, b):
            differing += 1
            if prim >= ns + nq:
                halves = [pc.geo.tri[prim - ns - nq].astype(np.float32)]
            else:
                k = [pc.geo.anchor[prim - ns] + u * pc.geo.E1[prim - ns] + v * pc.geo.E2[prim - ns] for u, v in ((0, 0), (1, 0), (1, 1), (0, 1))]
                halves = [np.array([k[0], k[1], k[2]], np.float32), np.array([k[0], k[2], k[3]], np.float32)]
            s = Fraction(4 * TAU) * Fraction(max(pair_scale(t, fr[i]) for t in halves))
            assert not any(tri_region_exact(t, fr[i], -s) for t in halves), (i, prim)
            assert any(tri_region_exact(t, fr[i], s) for t in halves), (i, prim)
    print("frustum vs box %-14s %d boxes: %d pairs in both sets, %d differ, all within 4 tau of touching" % (name, len(boxes), both, differing))
    assert both > 300


# ---- 5: semantics ----
@pytest.mark.parametrize("name", NAMES[:4] + ["case:degenerate", "case:mixed"], ids=IDS[:4] + ["degenerate", "mixed"])
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
    sel = np.arange(0, len(c.frusta), 7) if name == COFFEE else np.arange(len(c.frusta))
    sel = sel[counts[sel] < 5000]
    b, n = c.frusta[sel], counts[sel].astype(np.int64)
    for fmt in (64, 128):
        for label, cap in (("larger", n + 3), ("smaller", np.maximum(n - 1, 0)), ("zero", np.zeros_like(n)), ("fixed 4", np.full_like(n, 4))):
            o = csr(cap)
            p, got = frustumsim_list(c.pc.sim, b, o, fmt)
            assert same_bits(got, counts[sel]), label
            assert not (p == -7).any(), label                                         # every byte of every slice is defined
            for i in np.where(cap > 0)[0][::max(1, len(sel) // 200)]:
                s = p[o[i]:o[i + 1]]
                if n[i] <= cap[i]:
                    assert np.array_equal(s[:n[i]], prims[off[sel[i]]:off[sel[i] + 1]]) and (s[n[i]:] == -1).all(), (label, i)
                else:
                    assert (s == -1).all(), (label, i)


@pytest.mark.parametrize("name", NAMES[:4] + ["case:mixed"], ids=IDS[:4] + ["mixed"])
def test_invalid_empty_and_unconstrained_queries(name):
    """A non-finite float in any of the 24 slots: nothing.  A plane 0 0 0 d with d < 0: nothing.  Contradictory planes: no triangle and no
    quad.  Six zero planes: every id, in order."""
    c = case_of(name)
    for fmt in (64, 128):
        # contradictory planes: no triangle and no quad; the plane rule still reports a ball whose radius bridges the gap between them
        b = c.frusta[c.parts["empty"]]
        counts = frustumsim(c.pc.sim, b, "count", fmt)
        prims = frustumsim_list(c.pc.sim, b, csr(counts), fmt)[0]
        assert (prims < c.pc.geo.ns).all() and (c.pc.geo.ns > 0 or not counts.any())
        for part in ("invalid", "void"):
            b = c.frusta[c.parts[part]]
            assert not frustumsim(c.pc.sim, b, "any", fmt).any() and not frustumsim(c.pc.sim, b, "count", fmt).any()
            prims, counts = frustumsim_list(c.pc.sim, b, np.arange(len(b) + 1) * 3, fmt)
            assert not counts.any() and (prims == -1).all()
        z = c.frusta[c.parts["zero"]]
        assert (frustumsim(c.pc.sim, z, "count", fmt) == c.n_prims).all() and frustumsim(c.pc.sim, z, "any", fmt).all()
        prims, counts = frustumsim_list(c.pc.sim, z[:1], [0, c.n_prims], fmt)
        assert counts[0] == c.n_prims and np.array_equal(prims, np.arange(c.n_prims))
    assert not frustumbrute(c.pc.sim, c.frusta[c.parts["invalid"]], "count").any()


@pytest.mark.parametrize("name", NAMES[:4] + ["case:mixed", "case:offset"], ids=IDS[:4] + ["mixed", "offset"])
def test_plane_order_and_power_of_two_scaling_leave_the_set_alone(name):
    """S bit for bit under every rotation of the six planes and two random permutations, and under a power of two 2^-20 .. 2^20 on each
    plane's four floats: the lists are the same bytes."""
    c = case_of(name)
    sel = np.arange(0, c.parts["invalid"].start, 5 if name == COFFEE else 1)
    base = c.frusta[sel]
    _, counts, _ = c.walk()
    keep = counts[sel] < 20000
    base, want_c = base[keep], counts[sel][keep]
    want_p = frustumsim_list(c.pc.sim, base, csr(want_c))[0]
    rng = np.random.default_rng(34)
    orders = [np.roll(np.arange(6), k) for k in range(1, 6)] + [rng.permutation(6), rng.permutation(6)]
    for order in orders[::3] if name == COFFEE else orders:
        b = np.ascontiguousarray(base.reshape(-1, 6, 4)[:, order].reshape(-1, 24))
        p, lc = frustumsim_list(c.pc.sim, b, csr(want_c))
        assert same_bits(lc, want_c) and same_bits(p, want_p), order
    b = scale_planes(base, rng)
    assert not same_bits(b, base)
    p, lc = frustumsim_list(c.pc.sim, b, csr(want_c))
    assert same_bits(lc, want_c) and same_bits(p, want_p)
    assert same_bits(frustumbrute(c.pc.sim, b[::16], "count"), want_c[::16])


def test_sphere_rule_against_binary64_and_the_pinned_corner():
    """The sphere predicate is the plane rule on the ball: against the same rule in binary64 on random pairs (pairs within 1e-6 of a
    plane's threshold left out), and the corner case the header names: a ball within `radius` of two faces of a box but further than
    `radius` from their common edge is reported."""
    rng = np.random.default_rng(35)
    n = 4000
    rot = random_rotations(rng, n)
    planes = box_planes(rng.uniform(-1, 1, (n, 3)), rng.uniform(0.05, 0.5, (n, 3)), rot)
    planes[::3] = perspective(rng.uniform(-1, 1, (len(planes[::3]), 3)), rot[::3], rng.uniform(0.1, 1, len(planes[::3])), rng.uniform(0.1, 1, len(planes[::3])),
                              np.full(len(planes[::3]), 0.1), np.full(len(planes[::3]), 2.0))
    planes *= 2.0 ** rng.integers(-3, 4, (n, 6, 1))                      # not unit length
    planes[1::7, 3:] = 0.0
    fr = pack(planes)
    sph = np.concatenate([rng.uniform(-1.5, 1.5, (n, 3)), rng.uniform(0.01, 0.5, (n, 1))], axis=1).astype(np.float32)
    got = predicate("sphere", sph, fr)
    f, s = fr.astype(np.float64).reshape(-1, 6, 4), sph.astype(np.float64)
    ln = np.linalg.norm(f[:, :, :3], axis=2)
    margin = (f[:, :, :3] * s[:, None, :3]).sum(axis=2) + f[:, :, 3] + s[:, 3:4] * ln
    want = (margin >= 0).all(axis=1)
    near = ((np.abs(margin) <= 1e-6 * (np.abs(f[:, :, :3]).sum(axis=2) * 2.0 + np.abs(f[:, :, 3]))) & (ln > 0)).any(axis=1)      # a zero plane's margin is d itself
    assert np.array_equal(got[~near], want[~near]) and near.mean() < 0.01 and 0.05 < want.mean() < 0.95
    # the pinned corner: the box [-1, 1]^3; a ball of radius 1 centred at (1.9, 1.9, 0) is within 1 of the faces x = 1 and y = 1 (0.9 each)
    # but 1.27 from their common edge, so it does not touch the box: the plane rule reports it all the same
    cube = pack(box_planes([[0, 0, 0]], [[1, 1, 1]], np.eye(3)[None]))
    corner = np.array([[1.9, 1.9, 0.0, 1.0]], np.float32)
    assert np.hypot(0.9, 0.9) > 1.0 and predicate("sphere", corner, cube)[0]
    assert not predicate("sphere", np.array([[2.1, 1.9, 0.0, 1.0]], np.float32), cube)[0]       # outside one plane by more than the radius
    # the ball, not the surface: a region wholly inside a sphere meets it
    assert predicate("sphere", np.array([[0.0, 0.0, 0.0, 10.0]], np.float32), cube)[0]
    # and exact on a half-space: touching counts, 2^-23 further (s = -1 - 2^-23, a binary32 value) does not
    half = np.zeros((1, 24), np.float32); half[0, 0] = 1.0; half[0, 3] = -2.0           # x >= 2
    assert predicate("sphere", np.array([[1.0, 5.0, 5.0, 1.0]], np.float32), half)[0]
    assert not predicate("sphere", np.array([[1.0 - 2.0 ** -23, 5.0, 5.0, 1.0]], np.float32), half)[0]


def test_quads_are_their_two_triangles():
    hs = M.HostScene("cornell_quads", 64, 36)
    geo = Geometry(hs)
    assert geo.nq >= 5
    c = case_of("cornell_quads")
    b = c.frusta[valid_frusta(c.frusta)]
    counts = frustumbrute(hs, b, "count")
    got = membership(frustumbrute_list(hs, b, csr(counts))[0], csr(counts), geo.ns + geo.nq + geo.nt)
    f = hs.flat()["quads"]
    v3 = lambda v: [v.x, v.y, v.z]
    hit = np.zeros(geo.nq, int)
    for q in range(geo.nq):
        rec = np.array([v3(f[q].v1) + v3(f[q].v2) + v3(f[q].anchor)], np.float32)
        by_quad = predicate("quad", np.repeat(rec, len(b), axis=0), b)
        assert np.array_equal(by_quad, got[:, geo.ns + q])
        k = [(geo.anchor[q] + u * geo.E1[q] + v * geo.E2[q]).astype(np.float32) for u, v in ((0, 0), (1, 0), (1, 1), (0, 1))]
        t1 = predicate("tri", np.repeat(np.concatenate([k[0], k[1], k[2]])[None], len(b), axis=0), b)[0]
        t2 = predicate("tri", np.repeat(np.concatenate([k[0], k[2], k[3]])[None], len(b), axis=0), b)[0]
        # the corners here come from binary64 edges rounded once, the predicate's from binary32 arithmetic: equal but for a graze
        assert (by_quad != (t1 | t2)).mean() < 0.01
        hit[q] = by_quad.sum()
    assert (hit > 10).all()


# ---- 6: the renderer's camera ----
@pytest.mark.parametrize("name", NAMES[:4], ids=IDS[:4])
def test_tiles_of_the_renderers_camera_hold_what_their_rays_hit(name):
    """The scene's camera with lensRadius taken as 0 and a 4 x 4 split of the frame: the closest-hit primitive of every primary ray whose
    screen position lies at least 1/1000 of the frame inside its tile is in that tile's list; a primitive wholly behind the camera is in
    no tile's list."""
    pc = point_case(name)
    params = copy.copy(pc.hs.params)
    params.cam.lensRadius = 0.0
    pinhole = MovedScene(pc.hs, params=params)
    cam = scene_camera(pc.hs)
    rays = camera_rays(pinhole, 7)
    hits = querysim(pc.sim, rays, "closest")
    o, h, v, ll = (np.array(cam[k], np.float64) for k in ("origin", "horizontal", "vertical", "scrLowerLeftCorner"))
    assert np.allclose(rays[:, :3], o)
    # the screen position of a ray: ll - o + x h + y v = lambda d
    d = rays[:, 3:6].astype(np.float64)
    m = np.stack([np.broadcast_to(h, d.shape), np.broadcast_to(v, d.shape), -d], axis=2)
    xy = np.linalg.solve(m, np.broadcast_to(o - ll, d.shape)[:, :, None])[:, :2, 0]
    assert (xy > -0.05).all() and (xy < 1.05).all()                      # the pixel filter reaches a little over the frame's edge
    rects = tiles(4)
    fr = M.camera_frusta(cam, rects)
    assert fr.shape == (16, 24) and fr.dtype == np.float32
    counts = frustumsim(pc.sim, fr, "count")
    prims = frustumsim_list(pc.sim, fr, csr(counts))[0]
    off = csr(counts)
    n_prims = pc.geo.ns + pc.geo.nq + pc.geo.nt
    member = np.zeros((16, n_prims), bool)
    for t in range(16):
        member[t, prims[off[t]:off[t + 1]]] = True
    checked = 0
    for t, (x0, y0, x1, y1) in enumerate(rects):
        inside = (xy[:, 0] >= x0 + 1e-3) & (xy[:, 0] <= x1 - 1e-3) & (xy[:, 1] >= y0 + 1e-3) & (xy[:, 1] <= y1 - 1e-3) & (hits["prim"] >= 0)
        assert member[t, hits["prim"][inside]].all(), (t, np.unique(hits["prim"][inside][~member[t, hits["prim"][inside]]])[:8])
        checked += int(inside.sum())
    assert checked > 500
    # behind the camera: a triangle (for the scenes that have triangles) or a sphere moved to the mirror image of what the camera sees
    axis = np.cross(h, v); axis /= np.linalg.norm(axis)
    if axis @ (ll + 0.5 * h + 0.5 * v - o) < 0:
        axis = -axis
    if pc.geo.nt:
        depth = (pc.geo.tri - o) @ axis
        behind = np.where((depth < 0).all(axis=1))[0] + pc.geo.ns + pc.geo.nq
    else:
        depth = (pc.geo.centre - o) @ axis
        behind = np.where(depth + pc.geo.radius < 0)[0]
    print("frustum camera %-14s %d rays checked, %d primitives wholly behind the camera" % (name, checked, len(behind)))
    assert not member[:, behind].any()
    whole = M.camera_frusta(cam, [[0, 0, 1, 1]])
    everything = frustumsim_list(pc.sim, whole, [0, n_prims])[0]
    assert set(np.unique(hits["prim"][hits["prim"] >= 0]).tolist()) - set(everything.tolist()) == set() or xy.min() < 1e-3


def test_camera_frusta_planes():
    cam = dict(origin=[1.0, 2.0, 3.0], horizontal=[4.0, 0.0, 0.0], vertical=[0.0, 2.0, 0.0], scrLowerLeftCorner=[-1.0, 1.0, 2.0], lensRadius=0.3)
    f = M.camera_frusta(cam, [[0, 0, 1, 1], [0.25, 0.5, 0.5, 1.0]], near=0.5, far=10.0).astype(np.float64).reshape(2, 6, 4)
    inside = lambda q, p: ((q[:, :3] @ p + q[:, 3]) >= -1e-6).all()
    # the view axis is -z here: a point on the ray through screen (x, y) at depth t
    pt = lambda x, y, t: np.array([1.0, 2.0, 3.0]) + t * (np.array([-1.0 + 4 * x, 1.0 + 2 * y, 2.0]) - np.array([1.0, 2.0, 3.0]))
    assert inside(f[0], pt(0.5, 0.5, 1.0)) and inside(f[0], pt(0.01, 0.99, 5.0)) and not inside(f[0], pt(-0.01, 0.5, 1.0))
    assert not inside(f[0], pt(0.5, 0.5, 0.4)) and not inside(f[0], pt(0.5, 0.5, 10.5)) and not inside(f[0], pt(0.5, 0.5, -1.0))
    assert inside(f[1], pt(0.3, 0.7, 2.0)) and not inside(f[1], pt(0.6, 0.7, 2.0)) and not inside(f[1], pt(0.3, 0.4, 2.0))
    assert np.allclose(np.linalg.norm(f[:, :, :3], axis=2), 1.0, atol=1e-6)
    g = M.camera_frusta(cam, [[0, 0, 1, 1]]).reshape(6, 4)
    assert not g[5].any() and abs(g[4, :3] @ np.array([1.0, 2.0, 3.0]) + g[4, 3]) < 1e-6      # far = inf: a zero plane; near = 0: through the origin
    assert same_bits(M.camera_frusta(cam, [[0, 0, 1, 1]], near=0.5, far=10.0), M.camera_frusta({k: v for k, v in cam.items() if k != "lensRadius"},
                                                                                                [[0, 0, 1, 1]], near=0.5, far=10.0))
    hs = M.HostScene("spheres", 64, 36)
    assert same_bits(M.camera_frusta(hs.params.cam, tiles(2)), M.camera_frusta(scene_camera(hs), tiles(2)))
    for bad in (dict(rects=[[0, 0, 1]]), dict(rects=[[0.5, 0, 0.25, 1]]), dict(rects=[[0, 0, 1, 1]], near=2.0, far=1.0), dict(rects=[[0, 0, 1, 1]], near=-1.0)):
        with pytest.raises(ValueError):
            M.camera_frusta(cam, **bad)


# ---- 7: frustum_planes ----
@pytest.mark.parametrize("depth", ["gl", "zero"])
def test_frustum_planes_is_the_clip_space_test(depth):
    """A point's membership by the six planes equals its clip-space test, for both depth conventions, on points at least 1e-4 from the
    boundary; on a perspective and an orthographic matrix times a rigid motion."""
    rng = np.random.default_rng(36)
    n, f, asp, t = 0.5, 20.0, 1.6, np.tan(np.radians(30.0))
    if depth == "gl":
        proj = np.array([[1 / (asp * t), 0, 0, 0], [0, 1 / t, 0, 0], [0, 0, -(f + n) / (f - n), -2 * f * n / (f - n)], [0, 0, -1, 0]])
    else:
        proj = np.array([[1 / (asp * t), 0, 0, 0], [0, 1 / t, 0, 0], [0, 0, -f / (f - n), -f * n / (f - n)], [0, 0, -1, 0]])
    ortho = np.diag([0.5, 0.25, -0.1, 1.0]); ortho[2, 3] = -0.2
    view = np.eye(4); view[:3, :3] = random_rotations(rng, 1)[0]; view[:3, 3] = [0.3, -0.2, 1.0]
    mats = np.stack([proj @ view, ortho @ view])
    planes = M.frustum_planes(mats, depth)
    assert planes.shape == (2, 24) and planes.dtype == np.float32 and same_bits(M.frustum_planes(mats[0], depth), planes[:1])
    pts = rng.uniform(-25, 25, (20000, 3)); pts[:10000] *= 0.1
    hom = np.concatenate([pts, np.ones((len(pts), 1))], axis=1)
    for k in range(2):
        clip = hom @ mats[k].T
        x, y, z, w = clip.T
        margins = np.stack([w + x, w - x, w + y, w - y, w + z if depth == "gl" else z, w - z], axis=1)
        want = (margins >= 0).all(axis=1)
        clear = (np.abs(margins) >= 1e-4).all(axis=1)
        p = planes[k].astype(np.float64).reshape(6, 4)
        got = ((pts @ p[:, :3].T + p[:, 3]) >= 0).all(axis=1)
        assert np.array_equal(got[clear], want[clear]) and want.sum() > 100 and (~want).sum() > 100 and clear.mean() > 0.99
    # the planes answer a query as they are: the torus in a clip volume that holds it, and in one that does not
    ts = mesh_scene("torus")
    look = np.eye(4); look[2, 3] = -5.0                                  # the camera 5 units up the z axis, looking down -z
    assert frustumsim(ts, M.frustum_planes(proj @ look, depth), "count")[0] == Geometry(ts).nt
    away = np.eye(4); away[2, 3] = 5.0
    assert frustumsim(ts, M.frustum_planes(proj @ away, depth), "count")[0] == 0
    with pytest.raises(ValueError):
        M.frustum_planes(np.eye(3))
    with pytest.raises(ValueError):
        M.frustum_planes(np.eye(4), "dx")


# ---- the stack, pruning, the surface ----
@pytest.mark.parametrize("name", [COFFEE, "case:mixed", "case:geometric", "case:counts_2050"], ids=["coffee", "mixed", "geometric", "counts_2050"])
def test_stack_depth_is_within_the_trees_bound(name):
    c = case_of(name)
    depth = hostsim_bvh(c.pc.sim)[4]
    for fmt in (64, 128):
        for mode in ("any", "count"):
            d = frustum_stack_depth(c.pc.sim, c.frusta, mode, fmt)
            assert d <= 3 * depth + 1, (fmt, mode, d, depth)
            if name == COFFEE and mode == "count":
                assert d > 16, d              # more than the kernel keeps in LDS: its overflow columns are in use on this set


def test_beams_test_few_triangles():
    """Over the beam part of coffee's set the walk puts far fewer triangles through the predicate than the scene holds."""
    c = case_of(COFFEE)
    beams = c.frusta[c.parts["beams"]]
    steps, tested = frustum_work(c.pc.sim, beams)
    found = frustumsim(c.pc.sim, beams, "count")
    print("frustum prune coffee %d beams: %d triangles tested (%d node steps, %d ids found)" % (len(beams), tested.sum(), steps.sum(), found.sum()))
    assert found.sum() > 0 and tested.sum() >= found.sum() and tested.sum() < 0.05 * len(beams) * c.pc.geo.nt


def test_empty_batch():
    hs = M.HostScene("spheres", 64, 36)
    assert len(frustumsim(hs, np.zeros((0, 24), np.float32), "count")) == 0
    prims, counts = frustumsim_list(hs, np.zeros((0, 24), np.float32), [0])
    assert len(prims) == 0 and len(counts) == 0


def test_symbols_and_host_side_argument_checks():
    names = {"moptix_query_frusta", "moptix_query_frusta_device", "moptix_query_frusta_list", "moptix_query_frusta_list_device"}
    header = open(os.path.join(REPO, "include", "moptix.h")).read()
    assert names <= set(re.findall(r"\bint (moptix_[a-z0-9_]+)\s*\(", header))
    assert "Not offered: frusta" not in header and "frusta and general plane sets" not in header
    assert names <= set(K.DEVICE_SYMBOLS) and K.BOX_ANY == BOX_ANY == 0 and K.BOX_COUNT == BOX_COUNT == 1
    lib = K.device_lib()
    assert all(hasattr(lib, n) for n in names)
    assert "query_frusta" in dir(M.Context) and "frustum_planes" in dir(M) and "camera_frusta" in dir(M)
    assert lib.moptix_query_frusta(None, None, 0, 0, None) == K.ERR_INVALID
    assert lib.moptix_query_frusta_device(None, None, 0, 0, None) == K.ERR_INVALID
    assert lib.moptix_query_frusta_list(None, None, 0, None, None, None) == K.ERR_INVALID
    assert lib.moptix_query_frusta_list_device(None, None, 0, None, None, None) == K.ERR_INVALID
    blank = object.__new__(M.Context)                                  # mode, max_prims and the shape are refused before the context is looked at
    b = np.zeros((4, 24), np.float32)
    for kw in (dict(mode="closest"), dict(mode="count", max_prims=4), dict(mode="list", max_prims=-1)):
        with pytest.raises(ValueError):
            M.Context.query_frusta(blank, b, **kw)
    for bad in (b.reshape(-1), b[:, :23], np.zeros((4, 16), np.float32), np.zeros((4, 4, 6), np.float32)):
        with pytest.raises(ValueError):
            M.Context.query_frusta(blank, bad)
