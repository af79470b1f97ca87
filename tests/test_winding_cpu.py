"""Winding-number queries without a GPU: the CPU mirror of the winding kernel and its moments pass (tests/windingsim/windingsim.cpp:
pt_winding.h compiled for the host, on the host mirror of the builder's tree) against the definition -- every primitive in id order,
no tree --, against a binary64 numpy solid-angle sum that shares no code with either, and against values known from the geometry.

The mirror takes no node format: the walk reads references and moments, never a box, so there is nothing a format could change; both
option settings are run on the device (tests/test_gpu_winding.py)."""
import numpy as np
import pytest

import lbvh_cases
from common import HostsimHandle, hostsim_bvh
from point_helpers import point_case
from refit_helpers import RefitSim, moved_faces, same_words
from winding_helpers import (INF, QNAN, Geometry, box_points, cube, mesh_scene, off_surface, same_bits, solid_angle64, spheres_only, tri_term,
                             uv_sphere, winding64, winding_table, winding_work, windingbrute, windingsim)

K_EMPTY = lbvh_cases.K_EMPTY_REF

# ---- the measured figures (profiles/r32_winding.txt); every test holds four times its figure, the project's convention ----
# 1. The triangle term against binary64 on TERM_TRI and the 384 points of _term_points: the largest |omega - omega64|, in steradians.
TERM_MEASURED = 6.47e-7
# 3. The walk at beta = +inf against the binary64 sum, |w - w64| / max(1, s64) with s64 the sum of the terms' absolute values over 4 pi (a
# mesh of many overlapping faces has |terms| that add up to tens; the sum's error grows with them, not with w): the largest over the
# UV sphere and every lbvh_cases mesh, leaf sizes 1 and 4, 400 points each (2,000 on the sphere) uniform in 1.5 x the box and further
# than 1e-3 of the extent from the surface.  The largest is "duplicates" (100 copies of one triangle: the errors of its term add up
# coherently); the sphere has 1.19e-7.  What is measured is the conditioning of a solid angle near an edge more than the arithmetic:
# the binary32 rounding of v - q moves a vertex by 6e-8 of its coordinates, 1e-3 of the extent away from the edge.
WALK_MEASURED = 2.04e-6
# 2. The same figure for the scenes of spheres and quads: the largest of cornell_quads (9.77e-7) and random_spheres.  A quad's corners
# are anchor + E1 + E2 with E = v / dot(v, v) in binary32; the reference takes them in binary64.
QUADS_MEASURED = 2.77e-6
# 4. The far field on the UV sphere: the largest |w(beta) - w(inf)| over leaf sizes 1 and 4 and the 3,000 points of _far_points (beta 2:
# 0.03268 at leaf 1, 0.03088 at leaf 4; beta 4: 0.006374 and 0.006454).  A numpy prototype of the scheme gave 0.029 and 0.0053.
FAR_MEASURED = {2.0: 0.0327, 4.0: 0.00646}

TERM_TRI = np.array([[0.1, 0.2, 0.3], [1.3, 0.1, -0.2], [0.4, 1.1, 0.5]], np.float32)


def _term_points():
    """384 points around TERM_TRI's centroid at distances 1e-3 .. 1e2 of its size (64 per decade), none in its plane."""
    rng = np.random.default_rng(1)
    p = np.concatenate([rng.uniform(-1, 1, (64, 3)) * 10.0 ** k + TERM_TRI.mean(axis=0) for k in range(-3, 3)]).astype(np.float32)
    return p


def test_triangle_term_against_binary64():
    p = _term_points()
    got = tri_term(np.broadcast_to(TERM_TRI, (len(p), 3, 3)), p)
    ref = solid_angle64(TERM_TRI[None], p)[:, 0]
    err = float(np.abs(got - ref).max())
    print("triangle term: max |omega - omega64| = %.3g sr over %d points, omega in %.3f .. %.3f" % (err, len(p), ref.min(), ref.max()))
    assert (ref != 0).all() and ref.min() < -6.0 and ref.max() > 6.0          # both sides, up to nearly the half space
    assert err <= 4 * TERM_MEASURED


def test_triangle_term_is_exactly_zero_in_the_plane():
    """q at a vertex, on an edge, in the interior, coplanar outside: det is exactly 0 where the binary32 points lie in the plane exactly
    (z = 0.25 throughout; a rounded midpoint of a general edge is NOT on the edge, and rightly sees about pi)."""
    cases = {"vertex of a general triangle": TERM_TRI[1]}
    tri2 = np.array([[0, 0, 0.25], [1, 0, 0.25], [0, 1, 0.25]], np.float32)      # a plane the binary32 points lie in exactly
    pts2 = {"interior": [0.25, 0.25, 0.25], "coplanar outside": [2.0, 3.0, 0.25], "on an edge": [0.5, 0.0, 0.25], "at a vertex": [1.0, 0.0, 0.25]}
    for name, q in cases.items():
        w = tri_term(TERM_TRI[None], np.asarray(q, np.float32)[None])
        assert w.view(np.uint32)[0] in (0, 0x80000000) and w[0] == 0, (name, w)
    for name, q in pts2.items():
        w = tri_term(tri2[None], np.asarray(q, np.float32)[None])
        assert w.view(np.uint32)[0] == 0, (name, w)
    zero = np.zeros((1, 3, 3), np.float32)
    assert tri_term(zero, np.zeros((1, 3), np.float32)).view(np.uint32)[0] == 0       # a = b = c = 0
    assert tri_term(zero + 0.75, np.full((1, 3), 0.75, np.float32)).view(np.uint32)[0] == 0


# ---- known values ----
CUBE_IN = np.array([[0, 0, 0], [0.2, -0.3, 0.1], [0.49, 0.49, 0.49], [-0.45, 0.1, 0.3]], np.float32)
CUBE_OUT = np.array([[2, 0, 0], [0, 3, 0.3], [0.7, 0.1, 0.1], [-0.51, -0.51, -0.51]], np.float32)


@pytest.mark.parametrize("leaf", [1, 4])
def test_cube_inside_and_outside(leaf):
    tol = 4 * WALK_MEASURED * 2          # s64 of a cube seen from anywhere is at most 2 (front and back)
    for inward, inside in ((False, 1.0), (True, -1.0)):
        sim = HostsimHandle(mesh_scene(cube(inward=inward)), leaf)
        w_in, w_out = windingsim(sim, CUBE_IN), windingsim(sim, CUBE_OUT)
        print("cube inward=%s leaf %d: inside %s outside %s" % (inward, leaf, w_in, w_out))
        assert np.abs(w_in - inside).max() <= tol and np.abs(w_out).max() <= tol
        assert same_bits(windingbrute(sim, np.concatenate([CUBE_IN, CUBE_OUT])), np.concatenate([w_in, w_out]))


def test_open_cube_at_its_centre_is_five_sixths():
    sim = HostsimHandle(mesh_scene(cube(top=False)), 4)
    w = windingsim(sim, np.zeros((1, 3), np.float32))
    print("open cube, centre: %r" % w[0])
    assert abs(float(w[0]) - 5.0 / 6.0) <= 4 * WALK_MEASURED


def test_sphere_primitives_are_exactly_one_and_zero():
    """The scene "spheres" without its quads: three spheres and nothing else.  A sphere adds the binary64 4 pi, so w is the exact integer
    count of the spheres that hold the point."""
    hs = spheres_only()
    geo = Geometry(hs)
    assert geo.ns >= 2 and geo.nq == 0 and geo.nt == 0
    c, r = geo.centre.astype(np.float32), geo.radius.astype(np.float32)
    inside = c.copy(); inside[:, 0] += np.float32(0.25) * r
    outside = c.copy(); outside[:, 1] += np.float32(1.5) * r
    pts = np.concatenate([inside, outside, [[1e4, 2e4, -3e4]]]).astype(np.float32)
    holds = (((pts.astype(np.float64)[:, None, :] - geo.centre[None]) ** 2).sum(axis=-1) < geo.radius[None] ** 2).sum(axis=1)
    sim = HostsimHandle(hs, 4)
    for w in (windingsim(sim, pts, 2.0), windingbrute(sim, pts)):
        print("spheres alone: w %s" % w)
        assert same_bits(w, holds.astype(np.float32))
    assert (holds[:len(c)] >= 1).all() and (holds == 0).any()


@pytest.mark.parametrize("name", ["cornell_quads", "random_spheres"])
def test_spheres_and_quads_against_numpy(name):
    pc = point_case(name)
    pts = box_points(pc.lo, pc.hi, 600, 3)
    keep = off_surface(pc.sim, pts, float((pc.hi - pc.lo).max()))
    w, b = windingsim(pc.sim, pts, 2.0), windingbrute(pc.sim, pts)
    ref, s = winding64(pc.geo, pts, want_abs=True)
    err = float((np.abs(w - ref) / np.maximum(1.0, s))[keep].max())
    print("%s: %d spheres %d quads, excluded %.4f, max err %.3g, w in %.3f .. %.3f" % (name, pc.geo.ns, pc.geo.nq, 1 - keep.mean(), err, ref.min(), ref.max()))
    assert same_bits(w, b)                       # no tree: beta plays no part
    assert (~keep).sum() <= 0.02 * len(keep) and err <= 4 * QUADS_MEASURED


# ---- the walk against the definition ----
class Mesh:
    """A mesh scene with its geometry, its points (uniform in 1.5 x the box, winding_helpers.box_points), the binary64 sum on them and the
    leaf-1 and leaf-4 mirrors, made once and only read afterwards."""

    def __init__(self, name):
        self.hs = mesh_scene(uv_sphere()) if name == "uv_sphere" else lbvh_cases.case_scene(name)
        self.geo = Geometry(self.hs)
        self.lo, self.hi = self.geo.box()
        self.extent = float((self.hi - self.lo).max())
        self.pts = box_points(self.lo, self.hi, 2000 if name == "uv_sphere" else 400, 7)
        self.ref, self.s = winding64(self.geo, self.pts, want_abs=True)
        self._sims = {}

    def sim(self, leaf):
        if leaf not in self._sims:
            self._sims[leaf] = HostsimHandle(self.hs, leaf)
        return self._sims[leaf]


_meshes = {}


def mesh(name):
    if name not in _meshes:
        _meshes[name] = Mesh(name)
    return _meshes[name]


MESHES = ("uv_sphere",) + lbvh_cases.CASE_NAMES


@pytest.mark.parametrize("leaf", [1, 4])
@pytest.mark.parametrize("name", MESHES)
def test_walk_is_the_definition_and_the_binary64_sum(name, leaf):
    m = mesh(name)
    sim = m.sim(leaf)
    w, b = windingsim(sim, m.pts), windingbrute(sim, m.pts)
    keep = off_surface(sim, m.pts, m.extent)
    excluded = 1 - keep.mean()
    rel = np.abs(w - m.ref) / np.maximum(1.0, m.s)
    relb = np.abs(b - m.ref) / np.maximum(1.0, m.s)
    print("%s leaf %d: %d tris, excluded %.4f, walk %.3g brute %.3g (of max(1, s64)), s64 up to %.1f, words equal %.4f"
          % (name, leaf, m.geo.nt, excluded, rel[keep].max(), relb[keep].max(), m.s.max(), (w.view(np.uint32) == b.view(np.uint32)).mean()))
    assert np.isfinite(w).all() and np.isfinite(b).all()
    assert (~keep).sum() <= 0.02 * len(keep)
    assert rel[keep].max() <= 4 * WALK_MEASURED and relb[keep].max() <= 4 * WALK_MEASURED
    # the same binary32 terms in another order into a binary64 sum: the words differ by at most the final rounding
    assert np.abs(w - b).max() <= np.spacing(np.abs(b).max().astype(np.float32)) + 1e-12


def test_uv_sphere_is_closed_and_has_2208_faces():
    m = mesh("uv_sphere")
    assert m.geo.nt == 2208 and m.geo.nq == 0 and m.geo.ns == 0
    r = np.linalg.norm(m.pts.astype(np.float64), axis=1)
    w = windingsim(m.sim(4), m.pts)
    assert np.abs(w[r < 0.99] - 1).max() <= 4 * WALK_MEASURED * 2 and np.abs(w[r > 1.0]).max() <= 4 * WALK_MEASURED * 2


# ---- the far field ----
def _far_points():
    """The UV sphere's box points and 1,000 points at -1 % and +1 % of the radius from its surface."""
    m = mesh("uv_sphere")
    d = np.random.default_rng(6).normal(size=(500, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([m.pts, (d * 1.01).astype(np.float32), (d * 0.99).astype(np.float32)]), len(m.pts)


@pytest.mark.parametrize("leaf", [1, 4])
@pytest.mark.parametrize("beta", [2.0, 4.0])
def test_far_field_against_the_exact_walk(beta, leaf):
    m = mesh("uv_sphere")
    sim = m.sim(leaf)
    pts, n_box = _far_points()
    exact, approx = windingsim(sim, pts), windingsim(sim, pts, beta)
    clusters, tris, depth = winding_work(sim, pts, beta)
    both = (clusters > 0) & (tris > 0)
    err = float(np.abs(approx - exact).max())
    print("beta %g leaf %d: max |w - w(inf)| = %.4g (near the surface %.4g); both kinds of term in %.3f of the queries (%.3f near the surface); "
          "clusters %.1f tris %.1f a query; depth %d" % (beta, leaf, err, np.abs(approx - exact)[n_box:].max(), both.mean(), both[n_box:].mean(),
                                                            clusters.mean(), tris.mean(), depth.max()))
    assert both.any() and both[n_box:].mean() > 0.5 and clusters.sum() > 0 and tris.sum() > 0
    assert tris.mean() < 0.25 * m.geo.nt                       # the expansion saves work
    bound = 4 * FAR_MEASURED[beta]
    assert err <= bound
    decided = np.abs(exact - 0.5) > bound
    assert decided.mean() > 0.5 and ((approx > 0.5) == (exact > 0.5))[decided].all()
    ce, te, _ = winding_work(sim, pts[:64], INF)
    assert (ce == 0).all() and (te == m.geo.nt).all()           # +inf approximates nothing


# ---- the table ----
def _check_table(nodes, tris, root, table, face_pos):
    """Every child record of the table against numpy on the faces below it (face_pos [nFaces, 3, 3] binary64, by original id): the ball
    holds every vertex, in binary64 with no margin; A and N are the sums, to the binary32 rounding of a face's cross product.  Returns
    the number of records checked."""
    refs = nodes[:, 24:28].view(np.int32)
    prim = tris[:, 7].view(np.int32)
    checked = 0

    def below(ref):
        if ref < 0:
            first, count = (~ref) >> 3, ((~ref) & 7) + 1
            return list(prim[first:first + count])
        out = []
        for k in range(4):
            if refs[ref, k] != K_EMPTY:
                out += below(int(refs[ref, k]))
        return out
    if root == K_EMPTY or root < 0:
        return 0
    for n in range(len(nodes)):
        for k in range(4):
            rec = table[n, k].astype(np.float64)
            if refs[n, k] == K_EMPTY:
                assert (table[n, k].view(np.uint32) == 0).all()
                continue
            f = face_pos[below(int(refs[n, k]))]
            A, p, N, r = rec[0], rec[1:4], rec[4:7], rec[7]
            far = np.sqrt(((f.reshape(-1, 3) - p) ** 2).sum(axis=1)).max()
            assert far <= r, (n, k, far, r)
            e0, e1 = f[:, 1] - f[:, 0], f[:, 2] - f[:, 0]
            a = 0.5 * np.cross(e0, e1)
            scale = (np.linalg.norm(e0, axis=1) * np.linalg.norm(e1, axis=1)).sum() + 1e-300
            assert np.abs(N - a.sum(axis=0)).max() <= 2.0 ** -20 * scale, (n, k)
            assert abs(A - np.linalg.norm(a, axis=1).sum()) <= 2.0 ** -20 * scale, (n, k)
            checked += 1
    return checked


@pytest.mark.parametrize("leaf", [1, 4])
@pytest.mark.parametrize("name", ["uv_sphere", "degenerate", "offset", "mixed", "counts_9", "geometric"])
def test_table_balls_hold_their_faces_and_sums_are_the_numpy_sums(name, leaf):
    m = mesh(name)
    sim = m.sim(leaf)
    nodes, tris, prim, root, depth = hostsim_bvh(sim, leaf)
    table = winding_table(sim)
    assert len(table) == len(nodes)
    checked = _check_table(nodes, tris, root, table, m.geo.tri)
    print("%s leaf %d: %d nodes, %d child records checked" % (name, leaf, len(nodes), checked))
    assert checked >= len(nodes) * 2 or len(nodes) == 0


def test_table_after_a_refit():
    m = mesh("uv_sphere")
    rs = RefitSim(m.hs, 4)
    try:
        before = winding_table(rs._sim).copy()
        rs.refit()
        assert same_words(winding_table(rs._sim), before)      # a refit over unchanged positions: word for word
        fp, moved = moved_faces(m.hs, 0.05)
        rs.update(0, fp); rs.refit()
        t = rs.read()
        after = winding_table(rs._sim)
        assert not same_words(after, before)
        assert _check_table(t["nodes"], t["tris"], t["rootRef"], after, fp.astype(np.float64).reshape(-1, 3, 3)) > len(after)
        # and the walk on the refitted tree is the definition on the moved faces
        pts = m.pts[:300]
        geo = Geometry.__new__(Geometry)
        geo.__dict__.update(m.geo.__dict__); geo.tri = fp.astype(np.float64).reshape(-1, 3, 3)
        ref, s = winding64(geo, pts, want_abs=True)
        keep = off_surface(rs._sim, pts, m.extent)
        w = windingsim(rs._sim, pts)
        assert (np.abs(w - ref) / np.maximum(1.0, s))[keep].max() <= 4 * WALK_MEASURED
    finally:
        rs.close()


# ---- invalid rows ----
def test_invalid_rows_give_the_quiet_nan():
    sim = HostsimHandle(mesh_scene(cube()), 4)
    good = np.array([0.1, 0.2, 0.3, 2.0], np.float32)
    bad = []
    for k in range(3):
        for v in (np.nan, np.inf, -np.inf):
            r = good.copy(); r[k] = v; bad.append(r)
    for beta in (0.5, np.nan, -1.0, 0.0, -np.inf, np.float32(1.0) - np.float32(2.0 ** -24)):
        r = good.copy(); r[3] = beta; bad.append(r)
    bad = np.array(bad, np.float32)
    for entry in (windingsim, lambda s, q: windingbrute(s, q)):
        assert (entry(sim, bad).view(np.uint32) == QNAN).all()
    ok = np.array([good, [0.1, 0.2, 0.3, 1.0], [0.1, 0.2, 0.3, np.inf], [0.1, 0.2, 0.3, 3e38]], np.float32)
    w = windingsim(sim, ok)
    assert np.isfinite(w).all() and np.abs(w - 1).max() < 0.1          # beta = 1 is valid (and coarse), +inf exact
    assert abs(float(w[2]) - 1) <= 4 * WALK_MEASURED * 2
    mixed = np.concatenate([ok, bad[:3]])
    assert same_bits(windingsim(sim, mixed)[:4], w)


def test_empty_scene_is_zero():
    sim = HostsimHandle(mesh_scene(np.zeros((0, 3, 3), np.float32)), 4)
    pts = np.array([[0, 0, 0], [1, 2, 3]], np.float32)
    assert (windingsim(sim, pts, 2.0).view(np.uint32) == 0).all() and (windingbrute(sim, pts).view(np.uint32) == 0).all()
    assert len(winding_table(sim)) == 0
    one = HostsimHandle(mesh_scene(cube()[:1]), 4)               # a root that is a leaf: exact whatever beta says
    assert same_bits(windingsim(one, pts, 1.0), windingbrute(one, pts))
