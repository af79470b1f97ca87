"""Signed point queries on the CPU mirror (tests/hostsim/signsim.cpp): atan2_ac, the topology and its report, the table of pseudonormals
against a binary64 computation of its own, traversal == loop over every primitive byte for byte, signed == closest but for the sign bit,
and the sign against a binary64 generalized winding number."""
import numpy as np
import pytest

from common import M, HostsimHandle
from point_helpers import invalid_queries, point_case, pointsim, shortened
from refit_helpers import RefitSim, displace
from sign_helpers import (CLOSED_OUTWARD, INF, MESHES, atan2_ac, index_edges, mesh_points, pseudonormals64, same_bits, sign_case, sign_info,
                          sign_table, signbrute, signsim, spheres_and_cube, winding_number, with_max)

ALL = tuple(MESHES)


def test_atan2_ac_against_binary64():
    """Max absolute error <= 1e-6 over a log-uniform grid of magnitudes 1e-6 .. 1e3 in both arguments, both signs of x, and the exact cases
    y = 0, x = 0, y = x.  Measured: 2.5e-7 (written beside the function in pt_sign.h)."""
    m = np.float32(10.0) ** np.linspace(-6.0, 3.0, 361, dtype=np.float32)
    y, x = [a.reshape(-1) for a in np.meshgrid(m, m)]
    y = np.concatenate([y, y, np.zeros_like(m), np.zeros_like(m), m, m, m]).astype(np.float32)
    x = np.concatenate([x, -x, m, -m, np.zeros_like(m), m, -m]).astype(np.float32)
    got = atan2_ac(y, x).astype(np.float64)
    err = np.abs(got - np.arctan2(y.astype(np.float64), x.astype(np.float64)))
    print("atan2_ac: max absolute error %.3g over %d pairs" % (err.max(), len(y)))
    assert err.max() <= 1e-6
    n = len(m)
    assert (got[-2 * n:-n] == np.float32(np.pi / 4)).all()                      # y = x
    assert (got[2 * len(m) ** 2:2 * len(m) ** 2 + n] == 0).all()                # y = 0, x > 0
    assert atan2_ac([0.0], [0.0])[0] == 0


# open_torus: four quads of one ring are gone, and with them their four diagonals and the three edges between them
EXPECT = {   # weldedVerts, edges, boundaryEdges, nonManifoldEdges, flippedEdges, degenerateFaces, closed
    "cube": (8, 18, 0, 0, 0, 0, 1), "spike": (4, 6, 0, 0, 0, 0, 1), "l_prism": (12, 30, 0, 0, 0, 0, 1), "torus": (288, 864, 0, 0, 0, 0, 1),
    "open_torus": (288, 857, 10, 0, 0, 0, 0), "cube_one_reversed": (8, 18, 0, 0, 3, 0, 0), "fan": (5, 7, 6, 1, 0, 0, 0),
    "cube_degenerate": (8, 18, 0, 0, 0, 1, 0), "seam_pair": (8, 18, 0, 0, 0, 0, 1), "cube_inward": (8, 18, 0, 0, 0, 0, 1),
}
VOLUME = {"cube": 1.0, "l_prism": 3.0, "seam_pair": 1.0, "cube_inward": -1.0, "cube_degenerate": 1.0}


@pytest.mark.parametrize("name", ALL)
def test_topology_and_info(name):
    sc = sign_case(name)
    info = sign_info(sc.sim)
    got = tuple(info[k] for k in ("weldedVerts", "edges", "boundaryEdges", "nonManifoldEdges", "flippedEdges", "degenerateFaces", "closed"))
    assert got == EXPECT[name], info
    # the same counts from the index array instead of the positions
    count = index_edges(sc.f)
    assert info["edges"] == len(count) and info["boundaryEdges"] == sum(1 for c in count.values() if c == 1)
    assert info["nonManifoldEdges"] == sum(1 for c in count.values() if c > 2)
    assert info["weldedVerts"] == len(set(np.asarray(sc.f).reshape(-1).tolist()))
    if name in VOLUME:
        assert abs(info["signedVolume"] - VOLUME[name]) <= 1e-6, info
    t = sc.tri
    vol64 = (t[:, 0] * np.cross(t[:, 1], t[:, 2])).sum() / 6.0
    assert abs(info["signedVolume"] - vol64) <= 1e-9 * max(1.0, abs(vol64))
    if name in CLOSED_OUTWARD:
        assert info["signedVolume"] > 0
    assert info["tableBuilds"] == 0


def _angles(a, b):
    """Angle between corresponding rows, in radians, by atan2 of cross and dot (accurate for small angles)."""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(axis=-1))


@pytest.mark.parametrize("name", ALL)
def test_table_against_binary64_pseudonormals(name):
    sc = sign_case(name)
    tab = sign_table(sc.sim)
    assert not tab[:, 21:].any()                                                # the padding
    got = tab[:, :21].astype(np.float64).reshape(-1, 7, 3)
    want = pseudonormals64(sc.face_pos)
    dead = ~want.any(axis=(1, 2))
    assert dead.sum() == EXPECT[name][5]
    assert not got[dead].any()                                                  # a degenerate face's record is zero
    live = ~dead
    size = np.linalg.norm(want[live], axis=2)
    defined = size > 1e-3                                                       # a sum that cancels (the reversed face's edges) has no direction
    assert defined.all() or name == "cube_one_reversed"
    assert np.linalg.norm(got[live], axis=2)[~defined].max(initial=0.0) <= 1e-6
    ang = _angles(got[live], want[live])[defined]
    print("%s: largest angle between a table row and its binary64 direction %.3g rad" % (name, ang.max()))
    assert ang.max() <= 1e-5
    assert np.abs(np.linalg.norm(got[live][:, 6], axis=1) - 1.0).max() <= 1e-6  # the face normal is a unit vector


def _query_sets(sc):
    ref = signbrute(sc.sim, sc.q)
    return [("inf", sc.q), ("shortened", shortened(sc.q, np.abs(ref["dist"]), ref["prim"])), ("invalid", invalid_queries(np.append(sc.pts[0], INF)))]


def _only_sign_differs(signed, closest):
    a, b = signed.copy(), closest.copy()
    a["dist"] = np.abs(a["dist"]); b["dist"] = np.abs(b["dist"])
    return same_bits(a, b)


@pytest.mark.parametrize("name", ALL)
def test_traversal_is_the_loop_and_signed_is_closest(name):
    """Leaf sizes 1, 4, 8 x node formats 64, 128: the signed traversal's bytes are the signed loop's; and only the sign bit of dist tells
    the signed record from the closest mode's, misses and invalid queries included."""
    sc = sign_case(name)
    for set_name, q in _query_sets(sc):
        want = signbrute(sc.sim, q)
        closest = pointsim(sc.sim, q)
        assert _only_sign_differs(want, closest), set_name
        miss = closest["prim"] < 0
        assert same_bits(want[miss], closest[miss]), set_name
        if set_name == "invalid":
            assert miss.all()
        for leaf in (1, 4, 8):
            sim = sc.sim if leaf == 4 else HostsimHandle(sc.hs, leaf)
            for fmt in (64, 128):
                assert same_bits(signsim(sim, q, fmt), want), (set_name, leaf, fmt)
    if name in CLOSED_OUTWARD:
        assert (signbrute(sc.sim, sc.q)["dist"] < 0).sum() > 50                 # the sets do have points inside


def _agrees_with_winding(sc, signed, inside, label):
    """Every query at least 1e-5 x scale from the surface has the winding number's side; at most 1 % of the set is nearer than that."""
    far = np.abs(signed["dist"]) >= 1e-5 * sc.scale
    excluded = int((~far).sum())
    wrong = np.nonzero(far & ((signed["dist"] < 0) != inside))[0]
    print("%s: %d of %d queries excluded, %d mismatches, nearest counted query at %.3g x scale" % (
        label, excluded, len(far), len(wrong), np.abs(signed["dist"][far]).min() / sc.scale))
    assert len(wrong) == 0, (label, wrong[:8], sc.pts[wrong[:8]], signed[wrong[:8]])
    return excluded


@pytest.mark.parametrize("name", CLOSED_OUTWARD)
def test_sign_against_the_winding_number(name):
    sc = sign_case(name)
    inside, w = sc.inside64()
    off = slice(0, 2048)                                                        # the uniform and the near-surface points
    assert np.abs(w - np.round(w))[off].max() < 0.01                            # closed: the winding number is 0 or 1 off the surface
    signed = signbrute(sc.sim, sc.q)
    excluded = _agrees_with_winding(sc, signed[off], inside[off], name)
    assert excluded <= 0.01 * 2048


@pytest.mark.parametrize("name", ALL)
def test_points_on_the_features_are_not_negative(name):
    """The vertices, edge midpoints and face centroids themselves: dist is not negative (s == 0, and q == c, give +).

    This holds for the points that ARE on their feature as binary32 numbers (sign_helpers.on_feature_exact: every vertex, the midpoints
    binary32 holds exactly -- all of the cube's, the L-prism's and the torus', whose vertices lie on a grid of 2^-10 for this -- and the
    centroids of axis-parallel faces), and it is asserted for every one of them.  The remaining midpoints and centroids are moved off
    the surface by their own rounding to binary32, to either side, by up to 4e-8 of the scale; for those the contract's answer is the side
    they are on, so "not negative" cannot hold for them: measured with every on-feature point taken as it comes, 2 of 20 on the spike and
    618 of 2,592 on a torus with unrounded vertices were negative, each at |dist| <= 3.3e-8 x scale, no vertex among them.  For those
    points the assertion is that they are found within 1e-6 x scale of the surface."""
    sc = sign_case(name)
    on = signbrute(sc.sim, sc.q[sc.parts["on"]])
    nv = len(sc.v)
    neg = np.signbit(on["dist"])
    exact = sc.on_exact
    print("%s: %d of %d on-feature points negative (vertices: %d of %d; exactly on their feature in binary32: %d of %d), largest |dist| %.3g x scale" % (
        name, neg.sum(), len(on), neg[:nv].sum(), nv, neg[exact].sum(), exact.sum(), np.abs(on["dist"]).max() / sc.scale))
    assert len(exact) == len(on) and exact[:nv].all() and exact.sum() >= nv + (3 * len(sc.f) if name != "spike" else 0)
    assert (on["dist"][:nv] == 0).all()                                         # a vertex is found at distance 0 exactly
    assert np.abs(on["dist"]).max() <= 1e-6 * sc.scale
    assert not neg[exact].any()


def _moved(sc, amplitude=0.05):
    """The case's faces displaced by a smooth function of the position: shared vertices stay shared, the surface stays closed."""
    return displace(sc.face_pos.reshape(-1, 3), amplitude, k=np.float32(2.0)).reshape(-1, 9)


def test_refitted_torus():
    sc = sign_case("torus")
    rs = RefitSim(sc.hs, 4)
    try:
        before = sign_table(rs._sim)
        assert same_bits(before, sign_table(sc.sim))
        fp = _moved(sc)
        rs.update(0, fp); rs.refit()
        after = sign_table(rs._sim)
        assert not same_bits(after, before) and (after != before).mean() > 0.5
        info = sign_info(rs._sim)
        assert info["closed"] == 1 and info["weldedVerts"] == 288               # the topology is the one taken before the move
        got = signsim(rs._sim, sc.q)
        assert same_bits(got, signbrute(rs._sim, sc.q))
        assert same_bits(signsim(rs._sim, sc.q, 128), got)
        w = winding_number(sc.pts[:2048], fp.astype(np.float64).reshape(-1, 3, 3))
        assert _agrees_with_winding(sc, got[:2048], w > 0.5, "moved torus") <= 0.01 * 2048
        assert ((got["dist"] < 0) != (signbrute(sc.sim, sc.q)["dist"] < 0)).sum() > 10       # the surface did move across some points
        rs.update(0, fp); rs.refit()                                            # a refit over unchanged positions
        assert same_bits(sign_table(rs._sim), after)
        ang = _angles(after[:, :21].astype(np.float64).reshape(-1, 7, 3), pseudonormals64(fp))
        assert ang.max() <= 1e-5
    finally:
        rs.close()


def test_inward_cube_flips_every_sign():
    """The convention: a mesh wound inwards reports a negative volume, and every sign is the opposite of the winding number's of the
    outward mesh."""
    sc, out = sign_case("cube_inward"), sign_case("cube")
    assert sign_info(sc.sim)["signedVolume"] < 0
    inside, _ = out.inside64()
    signed = signbrute(sc.sim, out.q)[:2048]                                    # the outward cube's points
    far = np.abs(signed["dist"]) >= 1e-5 * sc.scale
    assert (~far).sum() <= 0.01 * 2048
    assert ((signed["dist"] < 0)[far] == ~inside[:2048][far]).all()
    assert (np.abs(signed["dist"]) == np.abs(signbrute(out.sim, out.q)[:2048]["dist"])).all()


def test_spheres_quads_and_a_mesh_in_one_scene():
    hs, c, r, v, f = spheres_and_cube()
    sim = HostsimHandle(hs, 4)
    rng = np.random.default_rng(5)
    small = np.nonzero(r < 100)[0]
    d = rng.normal(size=(len(small), 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = np.concatenate([c[small], c[small] + 0.5 * r[small, None] * d, c[small] + 1.5 * r[small, None] * d, mesh_points(v, f)[0]]).astype(np.float32)
    q = with_max(pts)
    got = signbrute(sim, q)
    assert (got["prim"] >= 0).all()
    for fmt in (64, 128):
        assert same_bits(signsim(sim, q, fmt), got)
    closest = pointsim(sim, q)
    assert _only_sign_differs(got, closest)
    ns, nq = hs.sizes.nSpheres, hs.sizes.nQuads
    k = len(small)
    # A point halfway out is inside its sphere.  The spheres of this scene touch, so a centre is as far from its neighbour's surface as
    # from its own: at equal d2 the lower id wins, and the centre of the higher one is OUTSIDE the winner -- solids are not united
    assert (got["dist"][k:2 * k] < 0).all() and (got["prim"][k:2 * k] == small).all()
    own = got["prim"][:k] == small
    assert own.any() and (got["dist"][:k][own] < 0).all() and (got["dist"][:k][~own] > 0).all()
    sph = got["prim"] < ns
    dc = np.linalg.norm(pts[sph].astype(np.float64) - c[got["prim"][sph]], axis=1)
    clear = np.abs(dc - r[got["prim"][sph]]) > 1e-5 * r[got["prim"][sph]]
    assert ((got["dist"][sph] < 0) == (dc < r[got["prim"][sph]]))[clear].all()
    quad = (got["prim"] >= ns) & (got["prim"] < ns + nq)
    assert (got["dist"][quad] > 0).all()
    tri = got["prim"] >= ns + nq
    assert tri.sum() > 500
    w = winding_number(pts[tri], v.astype(np.float32).astype(np.float64)[f])
    far = np.abs(got["dist"][tri]) >= 1e-5 * np.sqrt(3.0) * 0.5
    assert ((got["dist"][tri] < 0) == (w > 0.5))[far].all() and (got["dist"][tri] < 0).sum() > 20


def test_cornell_quads_is_all_positive():
    pc = point_case("cornell_quads")
    q = with_max(pc.pts)
    got = signbrute(pc.sim, q)
    assert same_bits(got, pointsim(pc.sim, q)) and same_bits(signsim(pc.sim, q), got)
    assert (got["prim"] >= 0).all() and not np.signbit(got["dist"]).any()
    assert sign_info(pc.sim) == dict(weldedVerts=0, edges=0, boundaryEdges=0, nonManifoldEdges=0, flippedEdges=0, degenerateFaces=0, closed=0,
                                     tableBuilds=0, signedVolume=0.0)
