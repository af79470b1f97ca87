"""The signed point queries of the CPU mirror (tests/hostsim/signsim.cpp, in libhostsim.so), the meshes and point sets of the sign tests,
and two binary64 references that share no code with the mirror: the generalized winding number and the angle-weighted pseudonormals."""
import ctypes as C

import numpy as np

from common import M, HostsimHandle, MovedScene, SignsimInfo, _f32, _ptr, hostsim_lib
from point_helpers import INF, POINT_DTYPE, with_max      # noqa: F401  (for the tests)
from query_helpers import same_bits                        # noqa: F401

INFO_FIELDS = tuple(n for n, _ in SignsimInfo._fields_[:-1])      # the counters; signedVolume is the last field


class _SignState:
    """signsim_create on a built scene: the topology of its faces as they are at this moment."""

    def __init__(self, sim):
        self._s = C.c_void_p(hostsim_lib().signsim_create(sim._h))
        assert self._s

    def __del__(self):
        if getattr(self, "_s", None):
            hostsim_lib().signsim_free(self._s)
            self._s = None


def _state(sim):
    """The sign state of a HostsimHandle, made at the first sign call on it (a context's first signed query) and kept on the handle."""
    assert isinstance(sim, HostsimHandle) and sim._h
    if not hasattr(sim, "_sign_state"):
        sim._sign_state = _SignState(sim)
    return sim._sign_state._s


def atan2_ac(y, x):
    y, x = _f32(y), _f32(x)
    out = np.zeros(len(y), np.float32)
    hostsim_lib().signsim_atan2(_ptr(y), _ptr(x), _ptr(out), len(y))
    return out


def sign_info(sim):
    """moptix_get_sign_info of the mirror: a dict."""
    r = SignsimInfo()
    assert hostsim_lib().signsim_info_read(_state(sim), C.byref(r)) == 0
    d = {n: int(getattr(r, n)) for n in INFO_FIELDS}
    d["signedVolume"] = float(r.signedVolume)
    return d


def sign_table(sim):
    """The mirror's table for the handle's faces as they are now: (nFaces, 24) float32."""
    out = np.zeros((max(1, sim.n_faces), 24), np.float32)
    assert hostsim_lib().signsim_table(_state(sim), out.ctypes.data, None) == 0
    return out[:sim.n_faces]


def _points(points):
    return _f32(np.asarray(points, np.float32).reshape(-1, 4))


def signsim(sim, points, node_format=64):
    pts = _points(points)
    out = np.zeros(len(pts), POINT_DTYPE)
    assert hostsim_lib().signsim_query(_state(sim), int(node_format), _ptr(pts), len(pts), out.ctypes.data) == 0
    return out


def signbrute(sim, points):
    pts = _points(points)
    out = np.zeros(len(pts), POINT_DTYPE)
    assert hostsim_lib().signsim_brute(_state(sim), _ptr(pts), len(pts), out.ctypes.data) == 0
    return out


# ---- the meshes: (vertices [v, 3] float64, faces [f, 3] int), all wound outwards unless the name says otherwise ----
def _outward(v, f):
    """Flips every face whose normal points at the centroid of the vertices (for the convex meshes)."""
    v = np.asarray(v, np.float64); f = np.array(f, np.int64)
    c = v.mean(axis=0)
    t = v[f]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    flip = ((t.mean(axis=1) - c) * n).sum(axis=1) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return v, f


def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return _outward(v, f)


def spike():
    v = np.array([(0, 0, 0), (1, 0, 0), (.5, .05, 0), (.5, .02, 3)], np.float64)
    return _outward(v, [(0, 1, 2), (0, 1, 3), (1, 2, 3), (2, 0, 3)])


def l_prism():
    poly = [(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)]                    # counter-clockwise
    v = np.array([(x, y, z) for z in (0, 1) for x, y in poly], np.float64)     # bottom 0..5, top 6..11
    cap = [(0, 1, 3), (1, 2, 3), (0, 3, 5), (3, 4, 5)]
    f = [(a, c, b) for a, b, c in cap] + [(a + 6, b + 6, c + 6) for a, b, c in cap]
    for i in range(6):
        j = (i + 1) % 6
        f += [(i, j, j + 6), (i, j + 6, i + 6)]
    return v, np.array(f, np.int64)


def torus(nu=24, nv=12, R=1.0, r=0.4):
    u = 2 * np.pi * np.arange(nu) / nu; w = 2 * np.pi * np.arange(nv) / nv
    v = np.array([((R + r * np.cos(b)) * np.cos(a), (R + r * np.cos(b)) * np.sin(a), r * np.sin(b)) for a in u for b in w], np.float64)
    v = np.round(v * 1024.0) / 1024.0              # on a grid of 2^-10: the edge midpoints are binary32 numbers too, exactly on their edges
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            f += [(a, b, c), (a, c, d)]
    return v, np.array(f, np.int64)


def fan():
    v = np.array([(0, 0, 0), (0, 0, 1), (1, 0, .5), (-.5, .8, .5), (-.5, -.8, .5)], np.float64)
    return v, np.array([(0, 1, 2), (0, 1, 3), (0, 1, 4)], np.int64)


def _reversed(mesh, faces):
    v, f = mesh
    f = f.copy(); f[faces] = f[faces][:, [0, 2, 1]]
    return v, f


MESHES = {
    "cube": cube, "spike": spike, "l_prism": l_prism, "torus": torus,
    "open_torus": lambda: (torus()[0], torus()[1][8:]),                         # four quads of one ring are missing
    "cube_one_reversed": lambda: _reversed(cube(), [5]),
    "fan": fan,
    "cube_degenerate": lambda: (cube()[0], np.concatenate([cube()[1], [[0, 1, 1]]])),      # a zero-area face on an edge of the cube
    "seam_pair": cube,                                                           # the cube as two meshes: the first and the last six faces
    "cube_inward": lambda: _reversed(cube(), slice(None)),
}
CLOSED_OUTWARD = ("cube", "spike", "l_prism", "torus")


def index_edges(f):
    """{unordered vertex pair: number of faces} from the index array: the counts the topology must report, from the indices instead of
    the positions."""
    count = {}
    for a, b, c in np.asarray(f):
        if len({a, b, c}) < 3:
            continue
        for x, y in ((a, b), (b, c), (c, a)):
            k = (min(x, y), max(x, y))
            count[k] = count.get(k, 0) + 1
    return count


def _mesh_only(hs):
    """hs without its quads (coffee's three are its lights' geometry, and lie where the meshes are): the sizes are a copy."""
    sizes = type(hs.sizes)()
    C.memmove(C.byref(sizes), C.byref(hs.sizes), C.sizeof(sizes))
    sizes.nQuads = 0
    hs.sizes = sizes
    return hs


def mesh_scene(name):
    """The mesh alone as a scene in coffee's frame, materials and lights (lbvh_cases.case_scene's way, without coffee's quads); "seam_pair"
    has two materials, so its upload is two moptix_add_mesh calls whose faces share vertices by position only."""
    v, f = MESHES[name]()
    fp = v.astype(np.float32)[f.reshape(-1)].reshape(len(f), 9)
    hs = _mesh_only(MovedScene(M.HostScene("file:coffee", 64, 36), fp, new_faces=True))
    if name == "seam_pair":
        hs.flat()["faceMat"][len(f) // 2:] = 1
    return hs


def spheres_and_cube():
    """The scene "spheres" with the unit cube beside its spheres: spheres, a quad and a mesh in one scene."""
    base = M.HostScene("spheres", 64, 36)
    sph = base.flat()["spheres"]
    c = np.array([[sph[i].center.x, sph[i].center.y, sph[i].center.z] for i in range(base.sizes.nSpheres)], np.float64)
    r = np.array([sph[i].radius for i in range(base.sizes.nSpheres)], np.float64)
    v, f = cube()
    small = r < 100                                                              # not a ground sphere, if the scene has one
    v = v * 0.5 + (c[small].max(axis=0) + r[small].max() + 0.25)
    fp = v.astype(np.float32)[f.reshape(-1)].reshape(len(f), 9)
    hs = MovedScene(base, fp, new_faces=True)
    hs.accel = "Trbvh"                                                           # "spheres" itself asks for no tree: it has no mesh
    return hs, c, r, v, f


# ---- point sets ----
def mesh_points(v, f, seed=3):
    """float32 [n, 3] and the slices of its parts: 1,024 points uniform in the box grown by half its size; 1,024 at a random surface point
    plus an offset along the face normal within 2 % of the scale (the box diagonal) either way; and the vertices, edge midpoints and face
    centroids themselves ("on")."""
    rng = np.random.default_rng(seed)
    v = np.asarray(v, np.float32).astype(np.float64)
    t = v[np.asarray(f)]
    lo, hi = v.min(axis=0), v.max(axis=0)
    scale = float(np.linalg.norm(hi - lo))
    uni = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (1024, 3))
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    ok = np.linalg.norm(n, axis=1) > 0
    tt, nn = t[ok], n[ok] / np.linalg.norm(n[ok], axis=1, keepdims=True)
    i = rng.integers(0, len(tt), 1024)
    a, b = rng.uniform(size=1024), rng.uniform(size=1024)
    flip = a + b > 1
    a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
    near = tt[i, 0] + a[:, None] * (tt[i, 1] - tt[i, 0]) + b[:, None] * (tt[i, 2] - tt[i, 0]) + nn[i] * rng.uniform(-0.02, 0.02, (1024, 1)) * scale
    on = np.concatenate([v, 0.5 * (t[:, 0] + t[:, 1]), 0.5 * (t[:, 1] + t[:, 2]), 0.5 * (t[:, 2] + t[:, 0]), t.mean(axis=1)])
    pts = np.concatenate([uni, near, on]).astype(np.float32)
    return pts, dict(uniform=slice(0, 1024), near=slice(1024, 2048), on=slice(2048, len(pts))), scale


def on_feature_exact(v, f):
    """For the "on" part of mesh_points: True where the point AS A BINARY32 NUMBER lies exactly on its feature, decided in binary64 --
    every vertex; an edge midpoint that binary32 holds exactly (the midpoint of two binary32 points is exact in binary64); a centroid whose
    binary32 rounding has height exactly 0 over its face's plane (the rounding of a centroid of an axis-parallel face stays in the plane).
    The other midpoints and centroids were moved off the surface, to either side, when they were rounded to binary32."""
    v = np.asarray(v, np.float32).astype(np.float64)
    t = v[np.asarray(f)]
    mids = np.concatenate([0.5 * (t[:, 0] + t[:, 1]), 0.5 * (t[:, 1] + t[:, 2]), 0.5 * (t[:, 2] + t[:, 0])])
    mid_ok = (mids.astype(np.float32).astype(np.float64) == mids).all(axis=1)
    cen = t.mean(axis=1).astype(np.float32).astype(np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    d = cen - t[:, 0]
    terms = d * n                                                               # exactly on the plane: every term of the dot product is 0
    cen_ok = (terms == 0).all(axis=1) & (np.linalg.norm(n, axis=1) > 0)
    return np.concatenate([np.ones(len(v), bool), mid_ok, cen_ok])


# ---- binary64 references ----
def winding_number(q, tri):
    """The generalized winding number of the points q [n, 3] about the triangles tri [m, 3, 3]: the sum of the signed solid angles
    2 atan2(det(a, b, c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) over 4 pi (van Oosterom and Strackee)."""
    q = np.asarray(q, np.float64); tri = np.asarray(tri, np.float64)
    w = np.zeros(len(q))
    for t in tri:
        a, b, c = t[0] - q, t[1] - q, t[2] - q
        la, lb, lc = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1), np.linalg.norm(c, axis=1)
        det = (a * np.cross(b, c)).sum(axis=1)
        den = la * lb * lc + (a * b).sum(axis=1) * lc + (b * c).sum(axis=1) * la + (c * a).sum(axis=1) * lb
        w += 2.0 * np.arctan2(det, den)
    return w / (4.0 * np.pi)


def pseudonormals64(face_pos):
    """The table's seven rows per face in binary64, [f, 7, 3], by a computation of its own: corners welded by a dictionary over the position
    words, the corner angle by arccos, sums in any order; zero rows for a face with two equal corners or no area."""
    p = np.asarray(face_pos, np.float32).reshape(-1, 3, 3)
    key = lambda x: tuple((x + np.float32(0.0)).tolist())                        # -0 + 0 = +0
    t = p.astype(np.float64)
    nf = len(t)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    ln = np.linalg.norm(n, axis=1)
    keys = [[key(p[f, k]) for k in range(3)] for f in range(nf)]
    live = [ln[f] > 0 and len(set(keys[f])) == 3 for f in range(nf)]
    un = np.where(ln[:, None] > 0, n / np.maximum(ln, 1e-300)[:, None], 0.0)
    vsum, esum = {}, {}
    for f in range(nf):
        if not live[f]:
            continue
        for k in range(3):
            a, b = t[f, (k + 1) % 3] - t[f, k], t[f, (k + 2) % 3] - t[f, k]
            ang = np.arccos(np.clip((a * b).sum() / (np.linalg.norm(a) * np.linalg.norm(b)), -1.0, 1.0))
            vsum[keys[f][k]] = vsum.get(keys[f][k], 0.0) + ang * un[f]
        for x, y in ((0, 1), (0, 2), (1, 2)):
            e = frozenset((keys[f][x], keys[f][y]))
            esum[e] = esum.get(e, 0.0) + un[f]
    out = np.zeros((nf, 7, 3))
    for f in range(nf):
        if not live[f]:
            continue
        for k in range(3):
            out[f, k] = vsum[keys[f][k]]
        for s, (x, y) in enumerate(((0, 1), (0, 2), (1, 2))):
            out[f, 3 + s] = esum[frozenset((keys[f][x], keys[f][y]))]
        out[f, 6] = un[f]
    return out


# ---- the cases, made once: scene, point set, queries, the leaf-4 mirror handle ----
class SignCase:
    def __init__(self, name):
        self.name = name
        self.v, self.f = MESHES[name]()
        self.hs = mesh_scene(name)
        self.face_pos = self.hs.face_arrays()[0]
        self.tri = self.face_pos.astype(np.float64).reshape(-1, 3, 3)
        self.pts, self.parts, self.scale = mesh_points(self.v, self.f)
        self.on_exact = on_feature_exact(self.v, self.f)
        self.q = with_max(self.pts)
        self.sim = HostsimHandle(self.hs, 4)
        self._ref = None

    def inside64(self):
        """(inside by the winding number, the winding number itself) of the case's points."""
        if self._ref is None:
            w = winding_number(self.pts, self.tri)
            self._ref = (w > 0.5, w)
        return self._ref


_cases = {}


def sign_case(name):
    if name not in _cases:
        _cases[name] = SignCase(name)
    return _cases[name]
