"""Oriented box queries without a GPU: the CPU mirror of the oriented box kernel (tests/obbsim/obbsim.cpp: pt_obb.h compiled for the host, on
the host mirror of the builder's tree) against the definition -- a loop over every primitive record through its predicate --, against
the axis-aligned predicate and an exact rational evaluation where the frame is a signed permutation, against a binary64 separating-axis
gap in the box's frame from the scenes' original vertices, and against answers known from the geometry."""
import os
import re

import numpy as np
import pytest

import box_helpers
import lbvh_cases
from common import M, HostsimHandle, REPO, hostsim_bvh
from obb_helpers import (BOX_ANY, BOX_COUNT, Geometry, all_pairs_gap64, beam_set, csr, membership, obb_sets, obb_stack_depth, obb_work,
                         obbbrute, obbbrute_list, obbsim, obbsim_list, pack, padded_boxes_meeting, predicate, random_rotations, same_bits,
                         scene_extent, signed_permutations, valid_obbs, world_aabb)
from point_helpers import point_case
from query_helpers import SCENES
from sign_helpers import mesh_scene

K = M._capi
NAMES = [k for k, _ in SCENES] + ["case:" + n for n in lbvh_cases.CASE_NAMES]
IDS = [n.replace("file:", "").replace("case:", "") for n in NAMES]
COFFEE = "file:coffee"
# The largest |gap| / scale of a pair on which the binary32 predicate and the binary64 gap disagree, measured by
# test_predicates_against_the_binary64_gap on its four scenes, is 2.22e-8 (the torus; 1.6e-8 on spheres, below 1e-16 on cornell_quads and
# offset; profiles/r30_obb.txt section 4): TOL is 4 x that, the box and sweep tests' margin.  The reference maps the scene's original
# vertices by the query's sixteen floats in binary64; the predicate takes the record's v1 = p0 + e0 and v2 = p0 - e1, each up to an ulp away
# from them, and rounds v - c and the three dot products once more.  The scale of a pair includes the box's enclosing world box.
TOL = 4 * 2.22e-8
EYE = np.eye(3)


class Case:
    """A scene of the point tests (point_helpers.point_case: the scene, its geometry, its box, its leaf-4 mirror handle) with its oriented
    box set and the definition's answer -- counts and the CSR list of exact capacities -- computed once and only read afterwards.  On coffee
    the loop over 168,196 primitives runs on a subsample: every 24th box, and the special ones."""

    def __init__(self, name):
        self.name = name
        self.pc = point_case(name)
        self.obbs, self.parts = obb_sets(self.pc.geo, self.pc.lo, self.pc.hi)
        n = len(self.obbs)
        self.n_prims = self.pc.geo.ns + self.pc.geo.nq + self.pc.geo.nt
        sp = self.parts["special"]
        self.rows = np.unique(np.concatenate([np.arange(0, n, 24), np.arange(sp.start, sp.stop)])) if name == COFFEE else np.arange(n)
        self._brute = None
        self._walk = ()

    def brute(self):
        """(counts, prims, offsets) of the definition on rows."""
        if self._brute is None:
            b = self.obbs[self.rows]
            counts = obbbrute(self.pc.sim, b, "count")
            prims, c2 = obbbrute_list(self.pc.sim, b, csr(counts))
            assert same_bits(c2, counts) and same_bits((counts > 0).astype(np.int32), obbbrute(self.pc.sim, b, "any"))
            self._brute = (counts, prims, csr(counts))
        return self._brute

    def walk(self):
        """(any, counts, prims) of the leaf-4 walk of the 64-byte nodes on the full set."""
        if not self._walk:
            counts = obbsim(self.pc.sim, self.obbs, "count")
            self._walk = (obbsim(self.pc.sim, self.obbs, "any"), counts, obbsim_list(self.pc.sim, self.obbs, csr(counts))[0])
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
    """obbsim_query's and obbsim_list's bytes are obbsim_brute's, whole buffers: any, count and the list at exact capacities, no box
    excluded.  On coffee the definition covers Case.rows, and the walk of this tree is compared with the leaf-4 walk of the 64-byte
    nodes on the full set besides."""
    c = case_of(name)
    want_c, want_p, want_off = c.brute()
    sim = HostsimHandle(c.pc.hs, leaf)
    try:
        anyone, counts = obbsim(sim, c.obbs, "any", fmt), obbsim(sim, c.obbs, "count", fmt)
        assert anyone.dtype == np.int32 and counts.dtype == np.int32
        assert same_bits(counts[c.rows], want_c), np.where(counts[c.rows] != want_c)[0][:8]
        assert same_bits(anyone, (counts > 0).astype(np.int32))
        prims, lc = obbsim_list(sim, c.obbs[c.rows], want_off, fmt)
        assert same_bits(lc, want_c) and same_bits(prims, want_p)
        if name == COFFEE:
            ref_any, ref_c, ref_p = c.walk()
            full_p, full_c = obbsim_list(sim, c.obbs, csr(ref_c), fmt)
            assert same_bits(anyone, ref_any) and same_bits(counts, ref_c) and same_bits(full_c, ref_c) and same_bits(full_p, ref_p)
    finally:
        sim.close()


def test_obb_sets_have_every_kind_of_box():
    """What the sets are for: boxes that meet nothing, one, a few and many primitives, in every part; the invalid ones are invalid."""
    c = case_of("case:counts_2049")
    counts = c.brute()[0]
    assert 1400 <= len(c.obbs) <= 1600
    assert (counts == 0).sum() > 100 and (counts == 1).sum() > 10 and ((counts > 1) & (counts < 64)).sum() > 100 and (counts >= 64).sum() > 10
    for part in ("random", "beams", "tilted", "permuted", "flat", "touching"):
        assert (counts[c.parts[part]] > 0).sum() >= 10, part
    assert (counts[c.parts["far"]] > 0).any() and (counts[c.parts["far"]] == 0).any()
    valid = valid_obbs(c.obbs)
    assert valid[:c.parts["invalid"].start].all() and not valid[c.parts["invalid"]].any()
    assert counts[c.parts["whole"]] == c.n_prims and not counts[c.parts["invalid"]].any()
    h = c.obbs[c.parts["flat"], 3:6]
    assert {1, 2, 3} == set((h == 0).sum(axis=1).tolist())
    # a thin beam's enclosing world box is far larger than the beam
    b = c.obbs[c.parts["beams"]].astype(np.float64)
    w = world_aabb(b)
    assert (np.prod(w[:, 3:] - w[:, :3], axis=1) > 50 * np.prod(2 * b[:, 3:6], axis=1)).all()      # a 100:1 beam on a face diagonal: 71 times


# ---- 2: signed-permutation frames on an exact grid ----
def _half_grid(rng, shape):
    return (rng.integers(-6, 7, shape) * 0.5).astype(np.float32)       # -3 .. 3: a narrow range, so that many pairs touch


def test_signed_permutation_frames_are_exact_on_a_half_integer_grid():
    """The grid of test_box_cpu.test_predicates_are_exact_on_a_half_integer_grid: every coordinate, half-extent and radius a multiple of 1/2.
    With a signed permutation as axes the local coordinates are the world ones permuted and negated, exactly, and every intermediate of the
    local test is exact as it is there; the grown world box only ever grows.  So on every pair the predicate must equal the axis-aligned
    predicate (boxsim) of the permuted box c -+ P^T h, and the exact rational evaluation of that box -- touching pairs (gap exactly 0)
    included, all of which are overlaps."""
    rng = np.random.default_rng(43)
    nb, nt, ns = 144, 48, 24
    c = _half_grid(rng, (nb, 3))
    h = (rng.integers(0, 7, (nb, 3)) * 0.5).astype(np.float32)
    h[::10] = 0                                                          # points
    frames = signed_permutations()[np.arange(nb) % 48]
    obbs = pack(c, h, frames)
    hw = np.einsum("njk,nj->nk", np.abs(frames), h.astype(np.float64)).astype(np.float32)      # the half-extent along each world axis
    boxes = np.concatenate([c - hw, c + hw], axis=1)
    tris = _half_grid(rng, (nt, 3, 3))
    tris[:6] = np.round(tris[:6] * 0.25 * 2) / 2                         # small ones, inside boxes
    tris[6] = tris[6][[0, 0, 0]]                                         # a point
    step = np.array([0.5, -1.0, 0.5], np.float32)
    tris[7][1], tris[7][2] = tris[7][0] + step, tris[7][0] + 2 * step    # collinear
    spheres = np.concatenate([_half_grid(rng, (ns, 3)), (rng.integers(0, 13, (ns, 1)) * 0.5).astype(np.float32)], axis=1)
    bi, ti = np.meshgrid(np.arange(nb), np.arange(nt), indexing="ij")
    got = predicate("tri", tris[ti.ravel()].reshape(-1, 9), obbs[bi.ravel()])
    aligned = box_helpers.predicate("tri", tris[ti.ravel()].reshape(-1, 9), boxes[bi.ravel()])
    want = np.array([box_helpers.tri_box_exact(tris[t], boxes[b]) for b, t in zip(bi.ravel(), ti.ravel())])
    assert np.array_equal(got, aligned), np.where(got != aligned)[0][:8]
    assert np.array_equal(got, want[:, 0]), np.where(got != want[:, 0])[0][:8]
    bi, si = np.meshgrid(np.arange(nb), np.arange(ns), indexing="ij")
    got_s = predicate("sphere", spheres[si.ravel()], obbs[bi.ravel()])
    aligned_s = box_helpers.predicate("sphere", spheres[si.ravel()], boxes[bi.ravel()])
    want_s = np.array([box_helpers.sphere_box_exact(spheres[s], boxes[b]) for b, s in zip(bi.ravel(), si.ravel())])
    assert np.array_equal(got_s, aligned_s) and np.array_equal(got_s, want_s[:, 0]), np.where(got_s != want_s[:, 0])[0][:8]
    print("obb exact grid: %d triangle pairs (%d overlap, %d touch exactly), %d sphere pairs (%d overlap, %d touch exactly)" % (
        len(want), want[:, 0].sum(), want[:, 1].sum(), len(want_s), want_s[:, 0].sum(), want_s[:, 1].sum()))
    assert want[:, 1].sum() >= 100 and want_s[:, 1].sum() >= 20
    assert got[want[:, 1]].all() and got_s[want_s[:, 1]].all()
    assert 0.05 < want[:, 0].mean() < 0.95 and 0.05 < want_s[:, 0].mean() < 0.95


# ---- 3: binary64 on real geometry ----
def _small_scene(which):
    if which == "torus":
        return mesh_scene("torus")
    if which == "offset":
        return lbvh_cases.case_scene("offset")
    return M.HostScene(which, 64, 36)


@pytest.mark.parametrize("which", ["torus", "cornell_quads", "spheres", "offset"])
def test_predicates_against_the_binary64_gap(which):
    """Every box of the scene's set (the valid ones) against every primitive: the mirror's S from the definition's loop over the records,
    the binary64 gap in the box's frame from the scene's original vertices mapped by the query's own sixteen floats.  The predicate must
    agree with gap <= 0 wherever |gap| > TOL x scale, scale the largest |coordinate| of the pair; at most 1 % of the pairs may lie within
    that band.  Zero-area triangles are left out."""
    hs = _small_scene(which)
    geo = Geometry(hs)
    lo, hi = scene_extent(geo) if which in ("cornell_quads", "spheres") else geo.box()
    obbs, _ = obb_sets(geo, lo, hi)
    obbs = obbs[valid_obbs(obbs)]
    n_prims = geo.ns + geo.nq + geo.nt
    counts = obbbrute(hs, obbs, "count")
    prims, _ = obbbrute_list(hs, obbs, csr(counts))
    got = membership(prims, csr(counts), n_prims)
    gap, scale, usable = all_pairs_gap64(geo, obbs)
    want = gap <= 0
    differ = (got != want) & usable[None, :]
    rel = np.abs(gap) / scale
    worst = float(rel[differ].max()) if differ.any() else 0.0
    band = (rel <= TOL) & usable[None, :]
    print("obb64 %-14s %d boxes x %d primitives: %d overlaps, %d pairs differ, worst |gap| / scale of one %.3g, %.4f %% of pairs within %.3g" % (
        which, len(obbs), n_prims, int(want.sum()), int(differ.sum()), worst, 100.0 * band.mean(), TOL))
    assert want.sum() > 500 and (~want).sum() > 1000
    assert not (differ & (rel > TOL)).any(), worst
    assert band.mean() <= 0.01


# ---- 4: semantics ----
def test_invalid_boxes_meet_nothing():
    c = case_of(COFFEE)
    whole = c.obbs[c.parts["whole"]]
    bad = []
    for k in range(15):
        for v in (np.nan, np.inf, -np.inf):
            r = whole.copy(); r[k] = v; bad.append(r)
    for k in range(3, 6):
        r = whole.copy(); r[k] = -r[k]; bad.append(r)
        r = whole.copy(); r[k] = np.float32(-1e-30); bad.append(r)
    for j in range(3):
        r = whole.copy(); r[6 + 3 * j:9 + 3 * j] *= np.float32(1.01); bad.append(r)
        r = whole.copy(); r[6 + 3 * j:9 + 3 * j] *= np.float32(0.99); bad.append(r)
        r = whole.copy(); r[6 + 3 * j:9 + 3 * j] += np.float32(0.01) * r[6 + 3 * ((j + 1) % 3):9 + 3 * ((j + 1) % 3)]; bad.append(r)
    r = whole.copy(); r[6:15] = 0; bad.append(r)
    bad = np.concatenate([np.array(bad, np.float32), c.obbs[c.parts["invalid"]]])
    assert not valid_obbs(bad).any()
    for fmt in (64, 128):
        assert not obbsim(c.pc.sim, bad, "any", fmt).any() and not obbsim(c.pc.sim, bad, "count", fmt).any()
        prims, counts = obbsim_list(c.pc.sim, bad, np.arange(len(bad) + 1) * 3, fmt)
        assert not counts.any() and (prims == -1).all()
    assert not obbbrute(c.pc.sim, bad, "count").any()
    ok = np.stack([whole, whole, whole])
    ok[0, 15] = np.nan                                                  # the sixteenth float is not read
    ok[1, 6:9] *= np.float32(1.0 + 2.0 ** -12)                          # within 2^-10 of unit length
    ok[2, 9:12] += np.float32(2.0 ** -12) * ok[2, 6:9]                  # within 2^-10 of orthogonal
    assert valid_obbs(ok).all()
    assert (obbsim(c.pc.sim, ok, "count") == c.n_prims).all()          # the valid box they were made from meets everything


@pytest.mark.parametrize("name", NAMES[:4] + ["case:mixed"], ids=IDS[:4] + ["mixed"])
def test_whole_scene_box_counts_every_primitive(name):
    c = case_of(name)
    whole = c.obbs[c.parts["whole"]][None]
    assert obbsim(c.pc.sim, whole, "count")[0] == c.n_prims and obbsim(c.pc.sim, whole, "any")[0] == 1
    prims, counts = obbsim_list(c.pc.sim, whole, [0, c.n_prims])
    assert counts[0] == c.n_prims and np.array_equal(prims, np.arange(c.n_prims))


def test_box_inside_a_sphere_or_inside_the_torus_meets_nothing():
    rot = random_rotations(np.random.default_rng(5), 3)
    hs = M.HostScene("spheres", 64, 36)
    geo = Geometry(hs)
    i = int(np.argmin(geo.radius))
    ctr, r = geo.centre[i], geo.radius[i]
    others = [j for j in range(geo.ns) if j != i and np.linalg.norm(geo.centre[j] - ctr) < geo.radius[j]]      # a ground sphere may hold it too
    assert not others
    inside = pack([ctr], [np.full(3, 0.3 * r)], rot[:1])               # its far corner is 0.52 r from the centre
    assert obbsim(hs, inside, "count")[0] == 0 and obbbrute(hs, inside, "count")[0] == 0
    through = pack([ctr + 0.6 * r * rot[0, 0]], [[0.9 * r, 0.3 * r, 0.3 * r]], rot[:1])      # reaches 1.5 r along its own axis 0
    prims, counts = obbsim_list(hs, through, [0, 4])
    assert counts[0] >= 1 and i in prims[:counts[0]]
    # the torus (R = 1, r = 0.4 about the z axis): a box in the tube's interior meets no face, one through the tube's wall does
    ts = mesh_scene("torus")
    tube = pack([[1.0, 0.0, 0.0]], [[0.1, 0.1, 0.1]], rot[1:2])
    hole = pack([[0.0, 0.0, 0.0]], [[0.2, 0.2, 0.2]], rot[2:3])
    along = np.array([[[1.0, 0.0, 0.0], [0.0, np.sqrt(0.5), np.sqrt(0.5)], [0.0, -np.sqrt(0.5), np.sqrt(0.5)]]])
    wall = pack([[1.25, 0.0, 0.0]], [[0.35, 0.1, 0.1]], along)
    assert obbsim(ts, tube, "count")[0] == 0 and obbsim(ts, hole, "any")[0] == 0 and obbsim(ts, wall, "count")[0] > 0


def test_point_box_on_a_vertex_finds_every_face_sharing_it():
    """h = 0 and c on a vertex, the frame a signed permutation: the local coordinates are exact differences, the vertex is the origin."""
    ts = mesh_scene("torus")
    tri = Geometry(ts).tri.astype(np.float32)
    frames = signed_permutations()
    for v in (tri[0, 0], tri[100, 1], tri[333, 2]):
        sharing = np.where((tri == v[None, None, :]).all(axis=2).any(axis=1))[0]
        assert len(sharing) >= 4
        obbs = pack(np.repeat(v[None], 48, axis=0), np.zeros((48, 3)), frames)
        counts = obbsim(ts, obbs, "count")
        prims, lc = obbsim_list(ts, obbs, csr(counts))
        assert same_bits(lc, counts)
        for k in range(48):
            found = set(prims[csr(counts)[k]:csr(counts)[k + 1]].tolist())
            assert set(sharing) <= found, (k, found, sharing)


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
    sel = np.arange(0, len(c.obbs), 7) if name == COFFEE else np.arange(len(c.obbs))
    sel = sel[counts[sel] < 5000]
    b, n = c.obbs[sel], counts[sel].astype(np.int64)
    for fmt in (64, 128):
        for label, cap in (("larger", n + 3), ("smaller", np.maximum(n - 1, 0)), ("zero", np.zeros_like(n)), ("fixed 4", np.full_like(n, 4))):
            o = csr(cap)
            p, got = obbsim_list(c.pc.sim, b, o, fmt)
            assert same_bits(got, counts[sel]), label
            assert not (p == -7).any(), label                                         # every byte of every slice is defined
            for i in np.where(cap > 0)[0][::max(1, len(sel) // 200)]:
                s = p[o[i]:o[i + 1]]
                if n[i] <= cap[i]:
                    assert np.array_equal(s[:n[i]], prims[off[sel[i]]:off[sel[i] + 1]]) and (s[n[i]:] == -1).all(), (label, i)
                else:
                    assert (s == -1).all(), (label, i)


def test_coincident_triangles_list_in_face_order():
    from pointmulti_helpers import duplicates_scene
    hs = duplicates_scene()
    tri = Geometry(hs).tri
    assert hs.sizes.nSpheres == 0 and hs.sizes.nQuads == 0
    rot = random_rotations(np.random.default_rng(9), 2)
    size = float(np.abs(tri[0] - tri[0].mean(axis=0)).max())
    obbs = pack([tri[0].mean(axis=0)] * 2, [np.full(3, 2.0 * size), np.full(3, 1e-3 * size)], rot)
    for leaf in (1, 4, 8):
        sim = HostsimHandle(hs, leaf)
        try:
            for fmt in (64, 128):
                prims, counts = obbsim_list(sim, obbs, [0, 100, 200], fmt)
                assert (counts >= 100).all() and np.array_equal(prims[:100], np.arange(100)) and np.array_equal(prims[100:], np.arange(100))
        finally:
            sim.close()


# ---- 5: the stack ----
@pytest.mark.parametrize("name", [COFFEE, "case:mixed", "case:geometric", "case:counts_2050"], ids=["coffee", "mixed", "geometric", "counts_2050"])
def test_stack_depth_is_within_the_trees_bound(name):
    c = case_of(name)
    depth = hostsim_bvh(c.pc.sim)[4]
    for fmt in (64, 128):
        for mode in ("any", "count"):
            d = obb_stack_depth(c.pc.sim, c.obbs, mode, fmt)
            assert d <= 3 * depth + 1, (fmt, mode, d, depth)
            if name == COFFEE and mode == "count":
                assert d > 16, d              # more than the kernel keeps in LDS: its overflow columns are in use on this set


# ---- 6: pruning ----
@pytest.mark.parametrize("name", ["torus", COFFEE], ids=["torus", "coffee"])
def test_beams_test_fewer_triangles_than_their_world_boxes_hold(name):
    """Over the beam set (100:1 and 1000:1 on diagonals) the walk puts strictly fewer triangles through the predicate in total than have
    a padded box meeting the beam's enclosing world box -- what a walk of that box would have to test at the least."""
    if name == "torus":
        hs = mesh_scene("torus")
        geo = Geometry(hs)
        lo, hi = geo.box()
        sim = hs
    else:
        pc = point_case(name)
        geo, lo, hi, sim = pc.geo, pc.lo, pc.hi, pc.sim
    beams = beam_set(geo, lo, hi, np.random.default_rng(31))
    assert valid_obbs(beams).all()
    tlo, thi = geo.tri.reshape(-1, 3).min(axis=0), geo.tri.reshape(-1, 3).max(axis=0)
    steps, tested = obb_work(sim, beams)
    inside = padded_boxes_meeting(geo.tri, float((thi - tlo).max()), world_aabb(beams))
    found = obbsim(sim, beams, "count")
    print("obb prune %-7s %d beams: %d triangles tested by the walk (%d node steps, %d ids found), %d in the enclosing world boxes, ratio %.4f" % (
        name.replace("file:", ""), len(beams), tested.sum(), steps.sum(), found.sum(), inside.sum(), tested.sum() / max(inside.sum(), 1)))
    assert found.sum() > 0 and tested.sum() >= found.sum()
    assert tested.sum() < inside.sum()


# ---- 7: packing, the empty batch, the surface ----
def test_oriented_boxes_packs_the_transpose():
    rng = np.random.default_rng(3)
    rot = random_rotations(rng, 5)                                      # rows = axes
    c, h = rng.normal(size=(5, 3)), rng.uniform(0.1, 1.0, (5, 3))
    want = pack(c, h, rot)
    got = M.oriented_boxes(c, h, np.swapaxes(rot, 1, 2))                # local-to-world: columns = axes
    assert got.dtype == np.float32 and got.shape == (5, 16) and same_bits(got, want)
    one = M.oriented_boxes(c, h[0], np.swapaxes(rot, 1, 2)[0])
    assert same_bits(one, pack(c, np.repeat(h[:1], 5, axis=0), np.repeat(rot[:1], 5, axis=0)))
    # a rotation by +90 degrees about z takes the box's x axis to world y
    rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert np.array_equal(M.oriented_boxes(np.zeros((1, 3)), np.ones(3), rz)[0, 6:9], [0.0, 1.0, 0.0])
    for bad in (dict(centre=np.zeros(3), half=np.ones(3), rotation=EYE), dict(centre=np.zeros((2, 3)), half=np.ones((3, 3)), rotation=EYE),
                dict(centre=np.zeros((2, 3)), half=np.ones(3), rotation=np.zeros((3, 3, 3)))):
        with pytest.raises(ValueError):
            M.oriented_boxes(**bad)
    # an identity frame answers as the axis-aligned query does
    ts = mesh_scene("torus")
    cells = M.occupancy_boxes((-1.5, -1.5, -0.5), (1.5, 1.5, 0.5), (8, 8, 4)).astype(np.float64)
    obbs = M.oriented_boxes(0.5 * (cells[:, :3] + cells[:, 3:]), 0.5 * (cells[:, 3:] - cells[:, :3]), EYE)
    occ = obbsim(ts, obbs, "any").reshape(8, 8, 4)
    assert occ.any() and not occ[3:5, 3:5].any() and not occ[0, 0].any()      # the hole and the corners are empty


def test_empty_batch():
    hs = M.HostScene("spheres", 64, 36)
    assert len(obbsim(hs, np.zeros((0, 16), np.float32), "count")) == 0
    prims, counts = obbsim_list(hs, np.zeros((0, 16), np.float32), [0])
    assert len(prims) == 0 and len(counts) == 0


def test_symbols_and_host_side_argument_checks():
    names = {"moptix_query_obbs", "moptix_query_obbs_device", "moptix_query_obbs_list", "moptix_query_obbs_list_device"}
    header = open(os.path.join(REPO, "include", "moptix.h")).read()
    assert names <= set(re.findall(r"\bint (moptix_[a-z0-9_]+)\s*\(", header))
    assert "Not offered: oriented boxes" not in header
    assert names <= set(K.DEVICE_SYMBOLS) and K.BOX_ANY == BOX_ANY == 0 and K.BOX_COUNT == BOX_COUNT == 1
    lib = K.device_lib()
    assert all(hasattr(lib, n) for n in names)
    assert "query_obbs" in dir(M.Context) and "oriented_boxes" in dir(M)
    assert lib.moptix_query_obbs(None, None, 0, 0, None) == K.ERR_INVALID
    assert lib.moptix_query_obbs_device(None, None, 0, 0, None) == K.ERR_INVALID
    assert lib.moptix_query_obbs_list(None, None, 0, None, None, None) == K.ERR_INVALID
    assert lib.moptix_query_obbs_list_device(None, None, 0, None, None, None) == K.ERR_INVALID
    blank = object.__new__(M.Context)                                  # mode, max_prims and the shape are refused before the context is looked at
    b = np.zeros((4, 16), np.float32)
    for kw in (dict(mode="closest"), dict(mode="count", max_prims=4), dict(mode="list", max_prims=-1)):
        with pytest.raises(ValueError):
            M.Context.query_obbs(blank, b, **kw)
    for bad in (b.reshape(-1), b[:, :15], np.zeros((4, 6), np.float32), np.zeros((4, 4, 4), np.float32)):
        with pytest.raises(ValueError):
            M.Context.query_obbs(blank, bad)
