"""The point queries of the CPU mirror (tests/hostsim/pointsim.cpp, in libhostsim.so), with the point sets of the point-query tests and a
binary64 distance that shares no code with the mirror."""
import numpy as np

from common import M, _f32, _ptr, hostsim_handle, hostsim_lib
from query_helpers import same_bits, scene_box      # noqa: F401  (same_bits: for the tests)

POINT_DTYPE = M.POINT_DTYPE
INF = np.float32(np.inf)


def _mode(mode):
    return {"closest": 0, "any": 1}[mode]


def _points(points):
    return _f32(np.asarray(points, np.float32).reshape(-1, 4))


def pointsim(hs, points, mode="closest", node_format=64, leaf_size=4):
    """moptix_query_points on the CPU, by the traversal: a POINT_DTYPE record array ("closest") or an int32 array ("any").  hs: a scene,
    or a built one."""
    sim = hostsim_handle(hs, leaf_size)
    pts = _points(points)
    out = np.zeros(len(pts), POINT_DTYPE if mode == "closest" else np.int32)
    assert hostsim_lib().pointsim_query(sim._h, int(node_format), _ptr(pts), len(pts), _mode(mode), out.ctypes.data) == 0
    return out


def pointbrute(hs, points, mode="closest", leaf_size=4):
    """The same from a loop over every primitive record of the built scene: no tree."""
    sim = hostsim_handle(hs, leaf_size)
    pts = _points(points)
    out = np.zeros(len(pts), POINT_DTYPE if mode == "closest" else np.int32)
    assert hostsim_lib().pointsim_brute(sim._h, _ptr(pts), len(pts), _mode(mode), out.ctypes.data) == 0
    return out


def stack_depth(hs, points, node_format=64, leaf_size=4):
    """Most stack entries the closest walk of any of the points holds."""
    sim = hostsim_handle(hs, leaf_size)
    pts = _points(points)
    d = hostsim_lib().pointsim_stack_depth(sim._h, int(node_format), _ptr(pts), len(pts))
    assert d >= 0
    return d


# ---- the scene's primitives as plain arrays (binary64), for the point sets and the binary64 distances ----
class Geometry:
    """tri [m, 3, 3], sphere centres [s, 3] and radii [s], quad anchors [k, 3] and edges E1, E2 [k, 3] (anchor + a1 E1 + a2 E2,
    a in [0, 1]); ids as the queries number them: spheres, quads, triangles."""

    def __init__(self, hs):
        f = hs.flat()
        ns, nq = hs.sizes.nSpheres, hs.sizes.nQuads
        self.centre = np.array([[f["spheres"][i].center.x, f["spheres"][i].center.y, f["spheres"][i].center.z] for i in range(ns)], np.float64).reshape(-1, 3)
        self.radius = np.array([f["spheres"][i].radius for i in range(ns)], np.float64)
        v3 = lambda v: [v.x, v.y, v.z]
        self.anchor = np.array([v3(f["quads"][i].anchor) for i in range(nq)], np.float64).reshape(-1, 3)
        v1 = np.array([v3(f["quads"][i].v1) for i in range(nq)], np.float64).reshape(-1, 3)
        v2 = np.array([v3(f["quads"][i].v2) for i in range(nq)], np.float64).reshape(-1, 3)
        self.E1 = v1 / np.maximum((v1 * v1).sum(axis=1, keepdims=True), 1e-300)
        self.E2 = v2 / np.maximum((v2 * v2).sum(axis=1, keepdims=True), 1e-300)
        self.tri = np.asarray(hs.face_arrays()[0], np.float32).astype(np.float64).reshape(-1, 3, 3)
        self.ns, self.nq, self.nt = ns, nq, len(self.tri)

    def box(self):
        """The box of everything but quads thousands of units wide (query_helpers.scene_box's rule is the caller's; this is the fallback
        for the cases, which are meshes)."""
        p = self.tri.reshape(-1, 3)
        return p.min(axis=0), p.max(axis=0)

    def surface_points(self, rng, n):
        """n random points on the surface, each primitive kind in proportion to its count (at least one of each kind present)."""
        kinds = [k for k, c in (("tri", self.nt), ("sphere", self.ns), ("quad", self.nq)) if c]
        out = []
        share = {k: max(1, n // len(kinds)) for k in kinds}
        share[kinds[0]] += n - sum(share.values())
        for k in kinds:
            m = share[k]
            if k == "tri":
                t = self.tri[rng.integers(0, self.nt, m)]
                a, b = rng.uniform(size=m), rng.uniform(size=m)
                flip = a + b > 1
                a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
                out.append(t[:, 0] + a[:, None] * (t[:, 1] - t[:, 0]) + b[:, None] * (t[:, 2] - t[:, 0]))
            elif k == "sphere":
                i = rng.integers(0, self.ns, m)
                d = rng.normal(size=(m, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
                out.append(self.centre[i] + self.radius[i, None] * d)
            else:
                i = rng.integers(0, self.nq, m)
                out.append(self.anchor[i] + rng.uniform(size=(m, 1)) * self.E1[i] + rng.uniform(size=(m, 1)) * self.E2[i])
        return np.concatenate(out)[:n]


def point_sets(geo, lo, hi, seed=13):
    """The three point sets of a scene as one float32 [n, 3] array and the slices of its parts: 2,048 points uniform in the box lo .. hi
    enlarged by half its size on each side; 1,024 random surface points each offset along a random direction by the box diagonal x 10^k,
    k uniform in [-7, -1]; every 37th triangle's vertices, centroid and edge midpoints (the vertices exactly)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    size = np.maximum(hi - lo, 1e-3 * max(float(np.linalg.norm(hi - lo)), 1e-30))
    diag = float(np.linalg.norm(hi - lo))
    uni = rng.uniform(lo - 0.5 * size, hi + 0.5 * size, (2048, 3))
    d = rng.normal(size=(1024, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    near = geo.surface_points(rng, 1024) + d * (diag * 10.0 ** rng.uniform(-7.0, -1.0, (1024, 1)))
    t = geo.tri[::37]
    special = np.concatenate([t[:, 0], t[:, 1], t[:, 2], t.mean(axis=1), 0.5 * (t[:, 0] + t[:, 1]), 0.5 * (t[:, 1] + t[:, 2]),
                              0.5 * (t[:, 2] + t[:, 0])]) if len(t) else np.zeros((0, 3))
    pts = np.concatenate([uni, near, special]).astype(np.float32)
    return pts, dict(uniform=slice(0, 2048), near=slice(2048, 3072), special=slice(3072, len(pts)))


def with_max(pts, max_dist=INF):
    """[n, 3] positions -> [n, 4] queries."""
    pts = np.asarray(pts, np.float32)
    md = np.broadcast_to(np.asarray(max_dist, np.float32).reshape(-1, 1) if np.ndim(max_dist) else np.float32(max_dist), (len(pts), 1))
    return np.ascontiguousarray(np.concatenate([pts, md], axis=1), np.float32)


def shortened(queries, dist, prim):
    """Half the queries (even indices) end at 0.5 x the brute-force distance, the other half at 2 x; misses keep their maxDist
    (query_helpers.shortened's alternation)."""
    out = queries.copy()
    hit = prim >= 0
    f = np.where(np.arange(len(queries)) % 2 == 0, np.float32(0.5), np.float32(2.0)).astype(np.float32)
    out[hit, 3] = (f[hit] * dist[hit]).astype(np.float32)
    return out


def invalid_queries(base):
    """Queries that are misses by definition, one defect each, on top of the valid query `base` (x y z maxDist); the last two rows are
    maxDist = 0 and -1."""
    base = np.asarray(base, np.float32)
    rows = []
    for k in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            r = base.copy(); r[k] = bad; rows.append(r)
    for bad in (np.nan, -np.inf, -0.0, 0.0, -1.0):
        r = base.copy(); r[3] = bad; rows.append(r)
    return np.ascontiguousarray(np.array(rows, np.float32))


def query_sets(hs_built, pts, reference=None):
    """The three uses of a point set on a built scene: maxDist = inf; 0.5 x / 2 x the reference distance (the loop over every primitive,
    unless another function is given); the invalid rows."""
    q = with_max(pts)
    ref = (reference or pointbrute)(hs_built, q)
    return [("inf", q), ("shortened", shortened(q, ref["dist"], ref["prim"])), ("invalid", invalid_queries(np.append(pts[0], INF)))]


# ---- binary64, vectorised, independent of the mirror: Ericson's region classification for the triangle ----
def tri_dist64(q, t):
    """Distances from points q [n, 3] to triangles t [n, 3, 3], pairwise, and the nearest points [n, 3]; degenerate triangles included
    (they fall through to the segments)."""
    q = np.asarray(q, np.float64); t = np.asarray(t, np.float64)

    def seg(a, b):
        ab = b - a
        den = (ab * ab).sum(axis=1)
        s = np.clip(((q - a) * ab).sum(axis=1) / np.where(den > 0, den, 1.0), 0.0, 1.0)
        s = np.where(den > 0, s, 0.0)
        c = a + s[:, None] * ab
        return np.linalg.norm(q - c, axis=1), c
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    best, bc = seg(a, b)
    for u, v in ((b, c), (c, a)):
        d, cc = seg(u, v)
        m = d < best
        best = np.where(m, d, best); bc = np.where(m[:, None], cc, bc)
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(axis=1)
    ok = nn > 0
    nn1 = np.where(ok, nn, 1.0)
    h = ((q - a) * n).sum(axis=1) / nn1
    proj = q - h[:, None] * n
    # inside: the projected point is on the inner side of all three edges
    def side(u, v):
        return (np.cross(v - u, proj - u) * n).sum(axis=1)
    inside = ok & (side(a, b) >= 0) & (side(b, c) >= 0) & (side(c, a) >= 0)
    d = np.abs(h) * np.sqrt(nn1)
    m = inside & (d < best)
    return np.where(m, d, best), np.where(m[:, None], proj, bc)


def sphere_dist64(q, centre, radius):
    return np.abs(np.linalg.norm(np.asarray(q, np.float64) - centre, axis=1) - radius)


def quad_dist64(q, anchor, E1, E2):
    """The quad as the ray test defines it: the coordinates a_i = dot(v_i, q - anchor), v_i = E_i / |E_i|^2, clamped to [0, 1] each.  For a
    rectangle this is the nearest point; cornell_quads' blocks are parallelograms half a percent off a rectangle, for which it is the
    contract's point all the same."""
    w = np.asarray(q, np.float64) - anchor
    a1 = np.clip((w * E1).sum(axis=1) / (E1 * E1).sum(axis=1), 0.0, 1.0)
    a2 = np.clip((w * E2).sum(axis=1) / (E2 * E2).sum(axis=1), 0.0, 1.0)
    return np.linalg.norm(w - a1[:, None] * E1 - a2[:, None] * E2, axis=1)


def quad_off64(p, anchor, E1, E2):
    """How far p is from the parallelogram anchor + a E1 + b E2, a, b in [0, 1]: (a, b) by the Gram matrix, clamped, then the residual."""
    w = np.asarray(p, np.float64) - anchor
    g11, g12, g22 = (E1 * E1).sum(axis=1), (E1 * E2).sum(axis=1), (E2 * E2).sum(axis=1)
    r1, r2 = (w * E1).sum(axis=1), (w * E2).sum(axis=1)
    det = g11 * g22 - g12 * g12
    a = np.clip((r1 * g22 - r2 * g12) / det, 0.0, 1.0); b = np.clip((r2 * g11 - r1 * g12) / det, 0.0, 1.0)
    return np.linalg.norm(w - a[:, None] * E1 - b[:, None] * E2, axis=1)


def prim_dist64(geo, q, prim, on=False):
    """Binary64 distance from q[i] to primitive prim[i] (>= 0).  on: q is meant to lie ON the primitive -- quads then by quad_off64."""
    q = np.asarray(q, np.float64); prim = np.asarray(prim)
    out = np.zeros(len(q))
    s = prim < geo.ns
    if s.any():
        out[s] = sphere_dist64(q[s], geo.centre[prim[s]], geo.radius[prim[s]])
    k = (prim >= geo.ns) & (prim < geo.ns + geo.nq)
    if k.any():
        i = prim[k] - geo.ns
        out[k] = (quad_off64 if on else quad_dist64)(q[k], geo.anchor[i], geo.E1[i], geo.E2[i])
    t = prim >= geo.ns + geo.nq
    if t.any():
        out[t] = tri_dist64(q[t], geo.tri[prim[t] - geo.ns - geo.nq])[0]
    return out


def scene_dist64(geo, q, upper):
    """Binary64 distance from every q[i] to the whole scene.  upper[i]: any valid upper bound of it (the mirror's distance; slack is
    added here).  Triangles are grouped 64 at a time by a coarse grid over their centres; groups, then triangles, whose bounding sphere
    lies beyond the bound are left out, which changes no minimum."""
    q = np.asarray(q, np.float64)
    best = np.full(len(q), np.inf)
    for i in range(geo.ns):
        best = np.minimum(best, sphere_dist64(q, geo.centre[i], geo.radius[i]))
    for i in range(geo.nq):
        best = np.minimum(best, quad_dist64(q, geo.anchor[i][None], geo.E1[i][None], geo.E2[i][None]))
    if not geo.nt:
        return best
    lo, hi = geo.tri.min(axis=1), geo.tri.max(axis=1)
    cen = 0.5 * (lo + hi); rad = 0.5 * np.linalg.norm(hi - lo, axis=1)
    slo, shi = lo.min(axis=0), hi.max(axis=0)
    cell = np.minimum(((cen - slo) / np.maximum(shi - slo, 1e-300) * 32).astype(np.int64), 31)
    order = np.argsort((cell[:, 0] * 32 + cell[:, 1]) * 32 + cell[:, 2], kind="stable")
    G = 64
    ng = (geo.nt + G - 1) // G
    member = np.full(ng * G, order[-1]); member[:geo.nt] = order; member = member.reshape(ng, G)      # the last group repeats a triangle
    glo, ghi = lo[member].min(axis=1), hi[member].max(axis=1)
    gcen = 0.5 * (glo + ghi); grad = 0.5 * np.linalg.norm(ghi - glo, axis=1)
    scale = max(float(np.abs(geo.tri).max()), float(np.abs(q).max()))
    reach = np.asarray(upper, np.float64) * 1.001 + 1e-6 * scale
    step = max(1, (1 << 22) // ng)
    for a in range(0, len(q), step):
        qa, ra = q[a:a + step], reach[a:a + step]
        d = np.linalg.norm(qa[:, None, :] - gcen[None, :, :], axis=2)
        pi, gi = np.nonzero(d <= ra[:, None] + grad[None, :])
        for b in range(0, len(pi), 1 << 16):
            pj = np.repeat(pi[b:b + (1 << 16)], G); tj = member[gi[b:b + (1 << 16)]].reshape(-1)
            keep = np.linalg.norm(qa[pj] - cen[tj], axis=1) <= ra[pj] + rad[tj]
            pj, tj = pj[keep], tj[keep]
            np.minimum.at(best, a + pj, tri_dist64(qa[pj], geo.tri[tj])[0])
    return best


# ---- the scenes of the point tests, made once: geometry, box, point set, the leaf-4 mirror handle and its brute-force answers ----
class PointCase:
    def __init__(self, name):
        """name: a kind of query_helpers.SCENES ("file:coffee", ..., with its iarg) or "case:<lbvh_cases name>"."""
        import lbvh_cases
        from common import HostsimHandle
        from query_helpers import SCENES
        self.name = name
        if name.startswith("case:"):
            self.hs = lbvh_cases.case_scene(name[5:])
            self.geo = Geometry(self.hs)
            self.lo, self.hi = self.geo.box()
        else:
            self.hs = M.HostScene(name, 64, 36, iarg=dict(SCENES)[name])
            self.geo = Geometry(self.hs)
            self.lo, self.hi = scene_box(self.hs)
        self.pts, self.parts = point_sets(self.geo, self.lo, self.hi)
        # what a tolerance is relative to: max(|q|_inf, the largest |coordinate| of a box).  scale_box: the box the points were drawn from
        # (for the scenes of spheres on a ground quad thousands of units wide that is query_helpers.scene_box's box round the spheres);
        # scale_all: the box of every primitive, that quad's corners included -- the magnitudes the arithmetic really passes through
        g = self.geo
        far = [np.abs(self.lo).max(), np.abs(self.hi).max()]
        if g.nt:
            far.append(np.abs(g.tri).max())
        if g.ns:
            far.append((np.abs(g.centre) + g.radius[:, None]).max())
        for k in range(g.nq):
            far.append(max(np.abs(g.anchor[k] + a * g.E1[k] + b * g.E2[k]).max() for a in (0, 1) for b in (0, 1)))
        qmax = np.abs(self.pts.astype(np.float64)).max(axis=1)
        self.scale_box = np.maximum(qmax, max(np.abs(self.lo).max(), np.abs(self.hi).max()))
        self.scale_all = np.maximum(qmax, max(far))
        self.sim = HostsimHandle(self.hs, 4)
        self._sets, self._brute = None, {}

    def sets(self, walked=False):
        """walked: the shortened set from the traversal's distances instead of the loop's -- the same bytes (test_point_cpu.py), without
        the minute the loop takes on coffee; for the GPU tests, which compare with the traversal alone."""
        if self._sets is None:
            if walked and not self._brute:
                return query_sets(self.sim, self.pts, pointsim)
            self._sets = query_sets(self.sim, self.pts)
        return self._sets

    def brute(self, set_name, mode):
        """The loop over every primitive on the leaf-4 handle's records.  The (d2, prim) rule is a strict total order, so the answer does
        not depend on the order of the records: the one array serves the trees of every leaf size."""
        key = (set_name, mode)
        if key not in self._brute:
            self._brute[key] = pointbrute(self.sim, dict(self.sets())[set_name], mode)
        return self._brute[key]


_cases = {}


def point_case(name):
    if name not in _cases:
        _cases[name] = PointCase(name)
    return _cases[name]
