"""Box overlap queries without a GPU: the CPU mirror of the box kernel (tests/boxsim/boxsim.cpp: pt_box.h compiled for the host, on the host
mirror of the builder's tree) against the definition -- a loop over every primitive record through its predicate -- against an exact
rational evaluation of the predicates, against a binary64 separating-axis gap from the scenes' original vertices, and against answers
known from the geometry."""
import os
import re

import numpy as np
import pytest

import lbvh_cases
from box_helpers import (BOX_ANY, BOX_COUNT, Geometry, all_pairs_gap64, box_sets, box_stack_depth, boxbrute, boxbrute_list, boxsim,
                         boxsim_list, csr, membership, predicate, same_bits, scene_extent, sphere_box_exact, tri_box_exact, valid_boxes)
from common import M, HostsimHandle, REPO, hostsim_bvh
from point_helpers import point_case
from query_helpers import SCENES
from sign_helpers import mesh_scene

K = M._capi
NAMES = [k for k, _ in SCENES] + ["case:" + n for n in lbvh_cases.CASE_NAMES]
IDS = [n.replace("file:", "").replace("case:", "") for n in NAMES]
COFFEE = "file:coffee"
# The largest |gap| / scale of a pair on which the binary32 predicate and the binary64 gap disagree, measured by
# test_predicates_against_the_binary64_gap on its four scenes, is 8.61e-8 (the torus; profiles/r26_box.txt section 4): TOL is 4 x that,
# a third of the point queries' 1e-6.  The reference takes the scene's original vertices, the predicate the record's v1 = p0 + e0 and
# v2 = p0 - e1, each up to an ulp (6e-8 |v|) away from them: that, not the 13 axes' own arithmetic, is the measured figure.
TOL = 4 * 8.61e-8


class Case:
    """A scene of the point tests (point_helpers.point_case: the scene, its geometry, its box, its leaf-4 mirror handle) with its box set
    and the definition's answer -- counts and the CSR list of exact capacities -- computed once and only read afterwards.  On coffee the
    loop over 168,196 primitives runs on 64 boxes: 20 of each random part, 20 of the triangle specials and the last four."""

    def __init__(self, name):
        self.name = name
        self.pc = point_case(name)
        self.boxes, self.parts = box_sets(self.pc.geo, self.pc.lo, self.pc.hi)
        n = len(self.boxes)
        self.n_prims = self.pc.geo.ns + self.pc.geo.nq + self.pc.geo.nt
        if name == COFFEE:
            sp = self.parts["special"]
            self.rows = np.unique(np.concatenate([np.arange(0, 1024, 52), np.arange(1024, 1536, 26),
                                                  np.linspace(sp.start, n - 5, 20).astype(np.int64), np.arange(n - 4, n)]))
            assert len(self.rows) <= 64
        else:
            self.rows = np.arange(n)
        self._brute = None
        self._walk = {}

    def brute(self):
        """(counts, prims, offsets) of the definition on rows."""
        if self._brute is None:
            b = self.boxes[self.rows]
            counts = boxbrute(self.pc.sim, b, "count")
            prims, c2 = boxbrute_list(self.pc.sim, b, csr(counts))
            assert same_bits(c2, counts) and same_bits((counts > 0).astype(np.int32), boxbrute(self.pc.sim, b, "any"))
            self._brute = (counts, prims, csr(counts))
        return self._brute

    def walk(self):
        """(any, counts, prims) of the leaf-4 walk of the 64-byte nodes on the full set."""
        if not self._walk:
            counts = boxsim(self.pc.sim, self.boxes, "count")
            self._walk = (boxsim(self.pc.sim, self.boxes, "any"), counts, boxsim_list(self.pc.sim, self.boxes, csr(counts))[0])
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
    """boxsim_query's and boxsim_list's bytes are boxsim_brute's, whole buffers: any, count and the list at exact capacities, no box
    excluded.  On coffee the definition covers Case.rows, and the walk of this tree is compared with the leaf-4 walk of the 64-byte
    nodes on the full set besides."""
    c = case_of(name)
    want_c, want_p, want_off = c.brute()
    sim = HostsimHandle(c.pc.hs, leaf)
    try:
        anyone, counts = boxsim(sim, c.boxes, "any", fmt), boxsim(sim, c.boxes, "count", fmt)
        assert anyone.dtype == np.int32 and counts.dtype == np.int32
        assert same_bits(counts[c.rows], want_c), np.where(counts[c.rows] != want_c)[0][:8]
        assert same_bits(anyone, (counts > 0).astype(np.int32))
        prims, lc = boxsim_list(sim, c.boxes[c.rows], want_off, fmt)
        assert same_bits(lc, want_c) and same_bits(prims, want_p)
        if name == COFFEE:
            ref_any, ref_c, ref_p = c.walk()
            full_p, full_c = boxsim_list(sim, c.boxes, csr(ref_c), fmt)
            assert same_bits(anyone, ref_any) and same_bits(counts, ref_c) and same_bits(full_c, ref_c) and same_bits(full_p, ref_p)
    finally:
        sim.close()


def test_box_sets_have_every_kind_of_box():
    """What the sets are for: boxes that meet nothing, one, a few and many primitives; degenerate boxes; the touching pair of specials."""
    c = case_of("case:counts_2049")
    counts = c.brute()[0]
    b, parts = c.boxes, c.parts
    assert (counts == 0).sum() > 100 and (counts == 1).sum() > 10 and ((counts > 1) & (counts < 64)).sum() > 100 and (counts >= 64).sum() > 10
    sp = parts["special"]
    n_t = (sp.stop - sp.start - 4) // 4
    vertex = b[sp.start + n_t:sp.start + 2 * n_t]
    assert n_t > 10 and (vertex[:, :3] == vertex[:, 3:]).all()
    touch, below = counts[sp.start + 2 * n_t:sp.start + 3 * n_t], counts[sp.start + 3 * n_t:sp.start + 4 * n_t]
    # The box one ulp lower is inside the touching one, so it never finds more (step A alone says so for the face itself), and it loses
    # faces the touching one found.  Not every touching box finds its face: S is a function of the records (v1 and v2 are a rounding or two
    # away from the face's vertices), and the contact is a single point, where the rounded edge-cross terms of step B may land on either side.
    assert (below <= touch).all() and (below < touch).sum() >= 10 and (touch >= 1).sum() >= n_t // 2
    assert counts[parts["whole"]] == c.n_prims and not counts[[parts["inverted"], parts["nan"], parts["inf"]]].any()


# ---- 2: the predicates on an exact grid ----
def _half_grid(rng, shape):
    return (rng.integers(-6, 7, shape) * 0.5).astype(np.float32)       # -3 .. 3: a narrow range, so that many pairs touch


def test_predicates_are_exact_on_a_half_integer_grid():
    """Every coordinate and radius a multiple of 1/2 in [-8, 8]: every intermediate of the predicates is then exact in binary32 (products of
    multiples of 1/4 below 2^6, the plane term a multiple of 1/64 below 2^17), so the predicate must equal the exact rational evaluation on
    every pair -- touching pairs (gap exactly 0) included, all of which are overlaps."""
    rng = np.random.default_rng(41)
    nb, nt, ns = 150, 48, 24
    lo = _half_grid(rng, (nb, 3))
    hi = lo + (rng.integers(0, 7, (nb, 3)) * 0.5).astype(np.float32)
    hi[::10] = lo[::10]                                                  # points
    boxes = np.concatenate([lo, hi], axis=1)
    tris = _half_grid(rng, (nt, 3, 3))
    tris[:6] = np.round(tris[:6] * 0.25 * 2) / 2                         # small ones, inside boxes
    tris[6] = tris[6][[0, 0, 0]]                                         # a point
    step = np.array([0.5, -1.0, 0.5], np.float32)
    tris[7][1], tris[7][2] = tris[7][0] + step, tris[7][0] + 2 * step    # collinear
    spheres = np.concatenate([_half_grid(rng, (ns, 3)), (rng.integers(0, 13, (ns, 1)) * 0.5).astype(np.float32)], axis=1)
    bi, ti = np.meshgrid(np.arange(nb), np.arange(nt), indexing="ij")
    got = predicate("tri", tris[ti.ravel()].reshape(-1, 9), boxes[bi.ravel()])
    want = np.array([tri_box_exact(tris[t], boxes[b]) for b, t in zip(bi.ravel(), ti.ravel())])
    assert np.array_equal(got, want[:, 0]), np.where(got != want[:, 0])[0][:8]
    bi, si = np.meshgrid(np.arange(nb), np.arange(ns), indexing="ij")
    got_s = predicate("sphere", spheres[si.ravel()], boxes[bi.ravel()])
    want_s = np.array([sphere_box_exact(spheres[s], boxes[b]) for b, s in zip(bi.ravel(), si.ravel())])
    assert np.array_equal(got_s, want_s[:, 0]), np.where(got_s != want_s[:, 0])[0][:8]
    touching = int(want[:, 1].sum()) + int(want_s[:, 1].sum())
    print("box exact grid: %d triangle pairs (%d overlap, %d touch exactly), %d sphere pairs (%d overlap, %d touch exactly)" % (
        len(want), want[:, 0].sum(), want[:, 1].sum(), len(want_s), want_s[:, 0].sum(), want_s[:, 1].sum()))
    assert touching >= 200 and want[:, 1].sum() >= 100 and want_s[:, 1].sum() >= 20
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
    the binary64 gap from the scene's original vertices.  The predicate must agree with gap <= 0 wherever |gap| > TOL x scale, scale the
    largest |coordinate| of the pair; at most 1 % of the pairs may lie within that band.  Zero-area triangles are left out."""
    hs = _small_scene(which)
    geo = Geometry(hs)
    lo, hi = scene_extent(geo) if which in ("cornell_quads", "spheres") else geo.box()
    boxes, _ = box_sets(geo, lo, hi)
    boxes = boxes[valid_boxes(boxes)]
    n_prims = geo.ns + geo.nq + geo.nt
    counts = boxbrute(hs, boxes, "count")
    prims, _ = boxbrute_list(hs, boxes, csr(counts))
    got = membership(prims, csr(counts), n_prims)
    gap, scale, usable = all_pairs_gap64(geo, boxes)
    want = gap <= 0
    differ = (got != want) & usable[None, :]
    rel = np.abs(gap) / scale
    worst = float(rel[differ].max()) if differ.any() else 0.0
    band = (rel <= TOL) & usable[None, :]
    print("box64 %-14s %d boxes x %d primitives: %d overlaps, %d pairs differ, worst |gap| / scale of one %.3g, %.4f %% of pairs within %.3g" % (
        which, len(boxes), n_prims, int(want.sum()), int(differ.sum()), worst, 100.0 * band.mean(), TOL))
    assert want.sum() > 500 and (~want).sum() > 1000
    assert not (differ & (rel > TOL)).any(), worst
    assert band.mean() <= 0.01


# ---- 4: semantics ----
def test_invalid_boxes_overlap_nothing():
    c = case_of(COFFEE)
    whole = c.boxes[c.parts["whole"]]
    bad = []
    for k in range(6):
        for v in (np.nan, np.inf, -np.inf):
            r = whole.copy(); r[k] = v; bad.append(r)
    for k in range(3):
        r = whole.copy(); r[k], r[3 + k] = whole[3 + k], whole[k]; bad.append(r)
    bad = np.array(bad, np.float32)
    assert not valid_boxes(bad).any()
    for fmt in (64, 128):
        assert not boxsim(c.pc.sim, bad, "any", fmt).any() and not boxsim(c.pc.sim, bad, "count", fmt).any()
        prims, counts = boxsim_list(c.pc.sim, bad, np.arange(len(bad) + 1) * 3, fmt)
        assert not counts.any() and (prims == -1).all()
    assert not boxbrute(c.pc.sim, bad, "count").any()
    assert boxsim(c.pc.sim, whole[None], "count")[0] == c.n_prims      # the valid box they were made from meets everything


@pytest.mark.parametrize("name", NAMES[:4] + ["case:mixed"], ids=IDS[:4] + ["mixed"])
def test_whole_scene_box_counts_every_primitive(name):
    c = case_of(name)
    whole = c.boxes[c.parts["whole"]][None]
    assert boxsim(c.pc.sim, whole, "count")[0] == c.n_prims and boxsim(c.pc.sim, whole, "any")[0] == 1
    prims, counts = boxsim_list(c.pc.sim, whole, [0, c.n_prims])
    assert counts[0] == c.n_prims and np.array_equal(prims, np.arange(c.n_prims))


def test_box_inside_a_sphere_or_inside_the_torus_meets_nothing():
    hs = M.HostScene("spheres", 64, 36)
    geo = Geometry(hs)
    i = int(np.argmin(geo.radius))
    ctr, r = geo.centre[i], geo.radius[i]
    inside = np.concatenate([ctr - 0.3 * r, ctr + 0.3 * r]).astype(np.float32)[None]
    others = [j for j in range(geo.ns) if j != i and np.linalg.norm(geo.centre[j] - ctr) < geo.radius[j]]      # a ground sphere may hold it too
    assert not others
    assert boxsim(hs, inside, "count")[0] == 0 and boxbrute(hs, inside, "count")[0] == 0
    through = np.concatenate([ctr - 0.3 * r, ctr + np.array([1.2 * r, 0.3 * r, 0.3 * r])]).astype(np.float32)[None]
    prims, counts = boxsim_list(hs, through, [0, 4])
    assert counts[0] >= 1 and i in prims[:counts[0]]
    # the torus (R = 1, r = 0.4 about the z axis): a box in the tube's interior meets no face, one through the tube's wall does
    ts = mesh_scene("torus")
    tube = np.array([[0.9, -0.1, -0.1, 1.1, 0.1, 0.1]], np.float32)
    hole = np.array([[-0.2, -0.2, -0.2, 0.2, 0.2, 0.2]], np.float32)
    wall = np.array([[0.9, -0.1, -0.1, 1.6, 0.1, 0.1]], np.float32)
    assert boxsim(ts, tube, "count")[0] == 0 and boxsim(ts, hole, "any")[0] == 0 and boxsim(ts, wall, "count")[0] > 0


def test_point_box_on_a_vertex_finds_every_face_sharing_it():
    ts = mesh_scene("torus")
    tri = Geometry(ts).tri.astype(np.float32)
    for v in (tri[0, 0], tri[100, 1], tri[333, 2]):
        sharing = np.where((tri == v[None, None, :]).all(axis=2).any(axis=1))[0]
        assert len(sharing) >= 4
        box = np.concatenate([v, v])[None]
        n = boxsim(ts, box, "count")[0]
        prims, counts = boxsim_list(ts, box, [0, n])
        assert counts[0] == n and set(sharing) <= set(prims.tolist())
        # nothing else: every face found has the vertex within an ulp or two of its own plane and edges -- on this mesh, only the sharers
        assert set(prims.tolist()) == set(sharing), (prims, sharing)


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
    sel = np.concatenate([np.arange(0, 1536, 7), np.arange(len(c.boxes) - 8, len(c.boxes))]) if name == COFFEE else np.arange(len(c.boxes))
    sel = sel[counts[sel] < 5000]
    b, n = c.boxes[sel], counts[sel].astype(np.int64)
    for fmt in (64, 128):
        for label, cap in (("larger", n + 3), ("smaller", np.maximum(n - 1, 0)), ("zero", np.zeros_like(n)), ("fixed 4", np.full_like(n, 4))):
            o = csr(cap)
            p, got = boxsim_list(c.pc.sim, b, o, fmt)
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
    boxes = np.array([np.concatenate([tri[0].min(axis=0), tri[0].max(axis=0)]), np.concatenate([tri[0].mean(axis=0) - 1e-3, tri[0].mean(axis=0) + 1e-3])], np.float32)
    for leaf in (1, 4, 8):
        sim = HostsimHandle(hs, leaf)
        try:
            for fmt in (64, 128):
                prims, counts = boxsim_list(sim, boxes, [0, 100, 200], fmt)
                assert (counts >= 100).all() and np.array_equal(prims[:100], np.arange(100)) and np.array_equal(prims[100:], np.arange(100))
        finally:
            sim.close()


# ---- 5: the stack ----
@pytest.mark.parametrize("name", [COFFEE, "case:mixed", "case:geometric", "case:counts_2050"], ids=["coffee", "mixed", "geometric", "counts_2050"])
def test_stack_depth_is_within_the_trees_bound(name):
    c = case_of(name)
    depth = hostsim_bvh(c.pc.sim)[4]
    b = c.boxes if name != COFFEE else np.concatenate([c.boxes[:1536], c.boxes[-4:]])
    for fmt in (64, 128):
        for mode in ("any", "count"):
            d = box_stack_depth(c.pc.sim, b, mode, fmt)
            assert d <= 3 * depth + 1, (fmt, mode, d, depth)
            if name == COFFEE and mode == "count":
                assert d > 16, d              # more than the kernel keeps in LDS: its overflow columns are in use on this set


# ---- 6: the grid helper, the empty batch, the surface ----
def test_occupancy_boxes_share_their_planes():
    b = M.occupancy_boxes((-1.0, 0.0, 0.1), (2.0, 0.7, 0.3), (3, 4, 5)).reshape(3, 4, 5, 6)
    assert b.dtype == np.float32
    assert same_bits(b[1:, :, :, 0], b[:-1, :, :, 3]) and same_bits(b[:, 1:, :, 1], b[:, :-1, :, 4]) and same_bits(b[:, :, 1:, 2], b[:, :, :-1, 5])
    assert (b[0, :, :, 0] == np.float32(-1.0)).all() and (b[-1, :, :, 3] == np.float32(2.0)).all() and (b[..., 5][:, :, -1] == np.float32(0.3)).all()
    assert valid_boxes(b.reshape(-1, 6)).all()
    with pytest.raises(ValueError):
        M.occupancy_boxes((0, 0, 0), (1, 1, 1), (2, 0, 2))
    ts = mesh_scene("torus")
    cells = M.occupancy_boxes((-1.5, -1.5, -0.5), (1.5, 1.5, 0.5), (8, 8, 4))
    occ = boxsim(ts, cells, "any").reshape(8, 8, 4)
    assert occ.any() and not occ[3:5, 3:5].any() and not occ[0, 0].any()      # the hole and the corners are empty


def test_empty_batch():
    hs = M.HostScene("spheres", 64, 36)
    assert len(boxsim(hs, np.zeros((0, 6), np.float32), "count")) == 0
    prims, counts = boxsim_list(hs, np.zeros((0, 6), np.float32), [0])
    assert len(prims) == 0 and len(counts) == 0


def test_symbols_and_host_side_argument_checks():
    names = {"moptix_query_boxes", "moptix_query_boxes_device", "moptix_query_boxes_list", "moptix_query_boxes_list_device"}
    header = open(os.path.join(REPO, "include", "moptix.h")).read()
    assert names <= set(re.findall(r"\bint (moptix_[a-z0-9_]+)\s*\(", header)) and "MOPTIX_BOX_ANY = 0, MOPTIX_BOX_COUNT = 1" in header
    assert names <= set(K.DEVICE_SYMBOLS) and K.BOX_ANY == BOX_ANY == 0 and K.BOX_COUNT == BOX_COUNT == 1
    lib = K.device_lib()
    assert all(hasattr(lib, n) for n in names)
    assert "query_boxes" in dir(M.Context) and "occupancy" in dir(M.Context)
    assert lib.moptix_query_boxes(None, None, 0, 0, None) == K.ERR_INVALID
    assert lib.moptix_query_boxes_device(None, None, 0, 0, None) == K.ERR_INVALID
    assert lib.moptix_query_boxes_list(None, None, 0, None, None, None) == K.ERR_INVALID
    assert lib.moptix_query_boxes_list_device(None, None, 0, None, None, None) == K.ERR_INVALID
    blank = object.__new__(M.Context)                                  # mode, max_prims and the shape are refused before the context is looked at
    b = np.zeros((4, 6), np.float32)
    for kw in (dict(mode="closest"), dict(mode="count", max_prims=4), dict(mode="list", max_prims=-1)):
        with pytest.raises(ValueError):
            M.Context.query_boxes(blank, b, **kw)
    for bad in (b.reshape(-1), b[:, :5], np.zeros((4, 3, 2), np.float32)):
        with pytest.raises(ValueError):
            M.Context.query_boxes(blank, bad)
