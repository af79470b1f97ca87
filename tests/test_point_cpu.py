"""Point queries on the CPU (csrc/pt_point.h through tests/hostsim/pointsim.cpp): the traversal gives the bytes of a loop over every primitive, the
distances agree with an independent binary64 computation, degenerate triangles are well defined, and the details of the contract hold."""
import numpy as np
import pytest

import lbvh_cases
from common import M, HostsimHandle, MovedScene
from point_helpers import (INF, POINT_DTYPE, Geometry, invalid_queries, point_case, pointbrute, pointsim, prim_dist64, same_bits,
                           scene_dist64, tri_dist64, with_max)
from query_helpers import SCENES
from refit_helpers import RefitSim, moved_faces

ALL = [k for k, _ in SCENES] + ["case:" + n for n in lbvh_cases.CASE_NAMES]
IDS = [n.replace("file:", "").replace("case:", "") for n in ALL]

# The tolerances of the binary64 comparisons, relative to max(|q|_inf, the largest |coordinate| of a box).  Measured over every point set
# of every scene and case here (profiles/r16_point.txt), then 4 x the worst, rounded up to one significant digit:
#   TOL_BOX   the box the points were drawn from (query_helpers.scene_box; the cases' own box).  Worst 1.80e-5, on "spheres": that scene
#             stands on a quad 2,000 units wide which its box leaves out, and the quad's nearest point is rounded to a float near 1,000.
#   TOL_ALL   the box of every primitive, such a quad's corners included.  Worst 2.35e-7 (big_first_299_1), four ulps of the scale.
# Both are asserted: the first is the stated scale, the second keeps that one scene from loosening the check for all the others.
TOL_BOX, TOL_ALL = 8e-5, 1e-6


def _tol(pc, idx=slice(None)):
    return np.minimum(TOL_BOX * pc.scale_box[idx], TOL_ALL * pc.scale_all[idx])


def _records_differ(a, b):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1); b = np.ascontiguousarray(b).view(np.uint8).reshape(len(b), -1)
    return np.nonzero((a != b).any(axis=1))[0]


@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("leaf", [1, 4, 8])
@pytest.mark.parametrize("name", ALL, ids=IDS)
def test_traversal_equals_brute_force(name, leaf, fmt):
    """Every point of every set, both modes: pointsim_query's bytes are pointsim_brute's.  The loop runs once per scene, on the leaf-4
    handle: the (d2, prim) rule is a strict total order, so its answer cannot depend on the order of the records, which is all a leaf size
    changes -- shown here on every scene but coffee (whose loop takes a minute) by running it on this handle's own records as well."""
    pc = point_case(name)
    sim = HostsimHandle(pc.hs, leaf)
    try:
        for set_name, q in pc.sets():
            for mode in ("closest", "any"):
                want = pc.brute(set_name, mode)
                got = pointsim(sim, q, mode, node_format=fmt)
                assert same_bits(got, want), (set_name, mode, _records_differ(got, want)[:5])
                if pc.geo.nt <= 10000 and fmt == 64:
                    assert same_bits(pointbrute(sim, q, mode), want), (set_name, mode)
    finally:
        sim.close()


@pytest.mark.parametrize("name", ALL, ids=IDS)
def test_distances_against_binary64(name):
    """dist against the binary64 distance to the whole scene and to the reported primitive, p against the reported primitive; every point
    hits (maxDist = inf).  The primitive id is not compared: points on shared edges and vertices have several exact minimisers."""
    pc = point_case(name)
    b = pc.brute("inf", "closest")
    assert (b["prim"] >= 0).all() and np.isfinite(b["dist"]).all() and np.isfinite(b["p"]).all()
    q = pc.pts.astype(np.float64)
    dist = b["dist"].astype(np.float64)
    e_scene = np.abs(dist - scene_dist64(pc.geo, q, dist))
    e_prim = np.abs(dist - prim_dist64(pc.geo, q, b["prim"]))
    e_on = prim_dist64(pc.geo, b["p"].astype(np.float64), b["prim"], on=True)
    worst = {k: (float((e / pc.scale_box).max()), float((e / pc.scale_all).max())) for k, e in (("scene", e_scene), ("prim", e_prim), ("on", e_on))}
    print("point64 %-22s %6d points  worst error / scale_box, / scale_all:  scene %.3g %.3g  prim %.3g %.3g  p-on-prim %.3g %.3g" % (
        (name, len(q)) + worst["scene"] + worst["prim"] + worst["on"]))
    tol = _tol(pc)
    for k, e in (("scene", e_scene), ("prim", e_prim), ("on", e_on)):
        assert (e <= tol).all(), (k, int(np.argmax(e / tol)), worst[k])


def _collinear_scene():
    """Six triangles of three distinct collinear vertices (the middle vertex first, second or third; along an axis and along a diagonal;
    all coordinates small integers, so collinear exactly in binary32), far enough apart that each is nearest to its own points."""
    rows = []
    for k, (a, d) in enumerate((((0, 0, 0), (1, 0, 0)), ((0, 8, 0), (1, 1, 2)))):
        a, d = np.array(a, np.float64), np.array(d, np.float64)
        ends = [a, a + d, a + 3 * d]                       # the longest segment: ends[0] .. ends[2]
        for order in ((0, 1, 2), (1, 0, 2), (0, 2, 1)):
            off = np.array([0.0, 0.0, 16.0 * (len(rows) + 1)])
            rows.append(np.concatenate([ends[i] + off for i in order]))
    return MovedScene(M.HostScene("file:coffee", 64, 36), np.array(rows, np.float32), new_faces=True)


def test_degenerate_triangles():
    """Zero-area triangles in real leaves: every output finite; a triangle with two equal vertices is its segment, one with three its
    point, one with three distinct collinear vertices its longest segment -- each against binary64."""
    for name in ("case:degenerate", "case:line"):
        pc = point_case(name)
        for set_name, _ in pc.sets():
            r = pc.brute(set_name, "closest")
            hit = r["prim"] >= 0
            for f in ("dist", "u", "v", "p"):
                assert np.isfinite(r[f][hit]).all(), (name, set_name, f)
    pc = point_case("case:degenerate")
    r = pc.brute("inf", "closest")
    k = r["prim"] - pc.geo.ns - pc.geo.nq                  # (the cases stand in coffee's frame, which brings its three quads along)
    tri = k >= 0
    k = np.where(tri, k, 1)                                # face 1 is an ordinary triangle
    t = pc.geo.tri[k]
    two, three = tri & ((k % 5 == 0) | (k % 7 == 0)), tri & (k % 35 == 0)
    assert two.sum() > 100 and three.sum() > 10
    q = pc.pts.astype(np.float64)
    seg = tri_dist64(q, np.stack([t[:, 0], t[:, 2], t[:, 2]], axis=1))[0]          # p1 == p0: the segment p0 .. p2
    assert (np.abs(r["dist"] - seg)[two & ~three] <= _tol(pc)[two & ~three]).all()
    assert (np.abs(r["dist"] - np.linalg.norm(q - t[:, 0], axis=1))[three] <= _tol(pc)[three]).all()
    # three distinct collinear vertices
    hs = _collinear_scene()
    geo = Geometry(hs)
    rng = np.random.default_rng(3)
    f = rng.integers(0, geo.nt, 2048)
    lam = rng.uniform(-0.5, 1.5, (2048, 1))
    lo, hi = geo.tri.min(axis=1), geo.tri.max(axis=1)      # the ends of the longest segment (the vertices are ordered along a direction with positive components)
    pts = (lo[f] + lam * (hi[f] - lo[f]) + rng.normal(size=(2048, 3)) * 10.0 ** rng.uniform(-6, 0, (2048, 1))).astype(np.float32)
    r = pointbrute(hs, with_max(pts))
    assert same_bits(pointsim(hs, with_max(pts)), r) and np.isfinite(r["dist"]).all()
    q = pts.astype(np.float64)
    k = r["prim"] - geo.ns - geo.nq                        # (coffee's frame brings its quads along)
    assert (k == f).mean() > 0.9
    tri = k >= 0
    k, q = k[tri], q[tri]
    want = tri_dist64(q, np.stack([lo[k], hi[k], hi[k]], axis=1))[0]
    scale = np.maximum(np.abs(q).max(axis=1), np.abs(geo.tri).max())
    assert (np.abs(r["dist"][tri] - want) <= TOL_ALL * scale).all(), float((np.abs(r["dist"][tri] - want) / scale).max())


def test_equal_distance_gives_the_lower_id():
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float32)
    hs = MovedScene(M.HostScene("file:coffee", 64, 36), np.concatenate([tri + 5.0, tri, tri, tri + 5.0]), new_faces=True)      # faces 1 and 2 coincide
    rng = np.random.default_rng(5)
    pts = rng.uniform(-1.0, 2.0, (512, 3)).astype(np.float32)
    base = hs.sizes.nSpheres + hs.sizes.nQuads             # (coffee's frame brings its quads along)
    for leaf in (1, 4):
        r = pointsim(hs, with_max(pts), leaf_size=leaf)
        assert (r["prim"] == base + 1).sum() > 100 and not (r["prim"] == base + 2).any()
    pc = point_case("case:duplicates")                     # one triangle 100 times: every point, the shared vertices among them, reports face 0
    base = pc.geo.ns + pc.geo.nq
    for set_name in ("inf", "shortened"):
        r = pc.brute(set_name, "closest")
        assert (r["prim"] == base).sum() > 1000 and not (r["prim"] > base).any()
    r = pc.brute("inf", "closest")
    vertex = pc.parts["special"].start                    # the first special point is a vertex, exactly
    assert r["dist"][vertex] == 0.0 and r["prim"][vertex] == base


@pytest.mark.parametrize("name", ["file:coffee", "spheres", "cornell_quads", "random_spheres", "case:degenerate", "case:offset"])
def test_uv_reconstruct_p(name):
    pc = point_case(name)
    r = pc.brute("inf", "closest")
    g = pc.geo
    u, v = r["u"].astype(np.float64)[:, None], r["v"].astype(np.float64)[:, None]
    k = r["prim"]
    want = r["p"].astype(np.float64).copy()
    t = k >= g.ns + g.nq
    tri = g.tri[k[t] - g.ns - g.nq]
    want[t] = tri[:, 0] + u[t] * (tri[:, 1] - tri[:, 0]) + v[t] * (tri[:, 2] - tri[:, 0])
    s = k < g.ns
    assert not r["u"][s].any() and not r["v"][s].any()
    qd = (k >= g.ns) & ~t
    i = k[qd] - g.ns
    want[qd] = g.anchor[i] + u[qd] * g.E1[i] + v[qd] * g.E2[i]
    assert (np.abs(want - r["p"]).max(axis=1) <= _tol(pc)).all()
    assert ((r["u"] >= 0) & (r["v"] >= 0)).all() and (r["u"][t] + r["v"][t] <= 1 + 1e-6).all() and (r["u"][qd] <= 1).all() and (r["v"][qd] <= 1).all()


@pytest.mark.parametrize("name", ALL, ids=IDS)
def test_any_is_closest_finding_a_primitive(name):
    pc = point_case(name)
    for set_name, q in pc.sets():
        c, a = pc.brute(set_name, "closest"), pc.brute(set_name, "any")
        assert a.dtype == np.int32 and np.array_equal(a, (c["prim"] >= 0).astype(np.int32)), set_name
    # a smaller radius that still holds the nearest point changes nothing but the misses
    full, short = pc.brute("inf", "closest"), pc.brute("shortened", "closest")
    hit = short["prim"] >= 0
    assert hit.sum() > 1000 and (~hit).sum() > 1000      # (a point ON the surface has distance 0: either factor makes its maxDist 0, a miss)
    assert same_bits(short[hit], full[hit])
    q = dict(pc.sets())["shortened"]
    miss = short[~hit]
    assert same_bits(miss["dist"], q[~hit, 3]) and (miss["prim"] == -1).all() and (miss["mat"] == -1).all()
    assert not miss["u"].any() and not miss["v"].any() and not miss["p"].any()


def test_a_point_at_a_spheres_centre():
    pc = point_case("random_spheres")
    g = pc.geo
    c32, r32 = g.centre.astype(np.float32), g.radius.astype(np.float32)
    r = pointsim(pc.sim, with_max(c32))
    own = r["prim"] == np.arange(g.ns)
    assert own.sum() > g.ns // 2
    scale = np.maximum(np.abs(c32).max(axis=1), pc.scale_all.min())
    assert (np.abs(r["dist"].astype(np.float64) - r32)[own] <= TOL_ALL * scale[own]).all()      # the radius, up to the rounding of centre + radius
    assert np.array_equal(r["p"][own], (c32 + np.float32([1, 0, 0]) * r32[:, None])[own])
    assert np.array_equal(pointsim(pc.sim, with_max(c32, r32 * np.float32(0.5)), "any")[own], np.zeros(own.sum(), np.int32))


@pytest.mark.parametrize("name", ["file:coffee", "spheres"])
def test_invalid_queries_are_misses(name):
    pc = point_case(name)
    near = np.append(pc.pts[pc.parts["near"].start], np.float32(1e3))
    bad = invalid_queries(near)
    assert pointsim(pc.sim, near[None])["prim"][0] >= 0
    for fmt in (64, 128):
        r = pointsim(pc.sim, bad, node_format=fmt)
        assert same_bits(r["dist"], bad[:, 3])                                          # the given maxDist, NaN payload and -0 included
        assert (r["prim"] == -1).all() and (r["mat"] == -1).all() and not r["u"].any() and not r["v"].any() and not r["p"].any()
        assert not pointsim(pc.sim, bad, "any", node_format=fmt).any()
    assert same_bits(pointbrute(pc.sim, bad), pointsim(pc.sim, bad))
    ok = near.copy(); ok[3] = INF
    assert pointsim(pc.sim, ok[None])["prim"][0] >= 0                                   # +inf is "no limit", not a defect
    assert len(pointsim(pc.sim, np.zeros((0, 4), np.float32))) == 0


@pytest.mark.parametrize("leaf", [1, 4])
def test_after_a_refit(leaf):
    """A deformed mesh on the mirror's handle, refitted as a context refits: the traversal of the refitted tree equals the loop over the
    new records, in both node formats (where the refit kept the 64-byte form) and both modes."""
    pc = point_case("file:coffee")
    rs = RefitSim(pc.hs, leaf)
    try:
        fp, _ = moved_faces(pc.hs, 0.02)
        pts = pc.pts[::24]
        q = with_max(pts)
        before = pointsim(rs._sim, q)
        rs.update(0, fp)
        rs.refit()
        want = pointbrute(rs._sim, q)
        assert len(_records_differ(want, before)) > len(q) // 2                        # the mesh did move
        short = q.copy(); short[:, 3] = np.where(np.arange(len(q)) % 2 == 0, np.float32(0.5), np.float32(2.0)) * want["dist"]
        moved = Geometry(MovedScene(pc.hs, fp))
        e = np.abs(want["dist"] - prim_dist64(moved, pts.astype(np.float64), want["prim"]))
        scale = np.maximum(np.abs(pts.astype(np.float64)).max(axis=1), np.abs(moved.tri).max())      # the moved mesh's own coordinates
        assert (e <= TOL_ALL * scale).all(), float((e / scale).max())
        for fmt in (64, 128):
            assert same_bits(pointsim(rs._sim, q, node_format=fmt), want)
            for mode in ("closest", "any"):
                assert same_bits(pointsim(rs._sim, short, mode, node_format=fmt), pointbrute(rs._sim, short, mode)), (fmt, mode)
    finally:
        rs.close()
