"""Winding-number queries: the CPU mirror (tests/windingsim/libwindingsim.so), a binary64 numpy solid-angle sum that shares no code with
it, the meshes with known winding numbers, and the point sets -- shared by tests/test_winding_cpu.py, tests/test_gpu_winding.py and
tools/winding_bench.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from common import M, REPO, MovedScene, _f32, _ptr, hostsim_handle, hostsim_lib
from point_helpers import Geometry, pointsim      # noqa: F401  (Geometry: for the tests)
from query_helpers import same_bits               # noqa: F401  (for the tests)
from sign_helpers import _mesh_only

INF = np.float32(np.inf)
QNAN = 0x7fc00000                      # what an invalid row gives

_DIR = os.path.join(REPO, "tests", "windingsim")
_windingsim = None


def _lib():
    """tests/windingsim/libwindingsim.so (built here if it is missing, as common.hostsim_lib builds its library) with the signatures of
    its entries.  They take the handles of common.HostsimHandle."""
    global _windingsim
    if _windingsim is None:
        hostsim_lib()
        path = os.path.join(_DIR, "libwindingsim.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _DIR, "-s"])
        L = C.CDLL(path)
        vp, f32p, i64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int64)
        L.windingsim_table.argtypes, L.windingsim_table.restype = [vp, vp], C.c_int
        L.windingsim_query.argtypes, L.windingsim_query.restype = [vp, f32p, C.c_int64, f32p], C.c_int
        L.windingsim_brute.argtypes, L.windingsim_brute.restype = [vp, f32p, C.c_int64, f32p], C.c_int
        L.windingsim_work.argtypes, L.windingsim_work.restype = [vp, f32p, C.c_int64, i64p, i64p, i64p], C.c_int
        L.windingsim_tri.argtypes, L.windingsim_tri.restype = [f32p, f32p, C.c_int64, f32p], C.c_int
        _windingsim = L
    return _windingsim


def rows(points, beta=INF):
    """(n, 3) positions and beta, a scalar or (n,), as contiguous (n, 4) float32 rows x y z beta; (n, 4) rows pass through."""
    p = np.asarray(points, np.float32)
    if p.shape[1] == 4:
        return _f32(p)
    b = np.broadcast_to(np.asarray(beta, np.float32).reshape(-1, 1), (len(p), 1))
    return _f32(np.concatenate([p, b], axis=1))


def windingsim(hs, points, beta=INF, leaf_size=4):
    """moptix_query_winding on the CPU, by the walk: float32 per point.  hs: a scene, or a built one."""
    sim = hostsim_handle(hs, leaf_size)
    q = rows(points, beta)
    out = np.zeros(len(q), np.float32)
    assert _lib().windingsim_query(sim._h, _ptr(q), len(q), _ptr(out)) == 0
    return out


def windingbrute(hs, points, leaf_size=4):
    """The definition: every primitive in id order, the same binary32 terms, a binary64 sum, no tree."""
    sim = hostsim_handle(hs, leaf_size)
    q = rows(points, INF)
    out = np.zeros(len(q), np.float32)
    assert _lib().windingsim_brute(sim._h, _ptr(q), len(q), _ptr(out)) == 0
    return out


def winding_table(hs, leaf_size=4):
    """The mirror's moments table of the tree as it is now, (nNodes, 4, 8) float32: per child slot A, p.xyz, N.xyz, r."""
    sim = hostsim_handle(hs, leaf_size)
    n = _lib().windingsim_table(sim._h, None)
    assert n >= 0
    out = np.zeros((max(n, 1), 4, 8), np.float32)
    assert _lib().windingsim_table(sim._h, C.c_void_p(out.ctypes.data)) == n
    return out[:n]


def winding_work(hs, points, beta, leaf_size=4):
    """(clusters approximated, triangles evaluated, stack depth reached) of the walk, int64 per query."""
    sim = hostsim_handle(hs, leaf_size)
    q = rows(points, beta)
    out = [np.zeros(len(q), np.int64) for _ in range(3)]
    assert _lib().windingsim_work(sim._h, _ptr(q), len(q), *[_ptr(o, C.c_int64) for o in out]) == 0
    return tuple(out)


def tri_term(tris, points):
    """The mirror's triangle term on explicit pairs: tris (n, 3, 3), points (n, 3) -> the signed solid angle, float32."""
    t, p = _f32(np.asarray(tris, np.float32).reshape(-1, 9)), _f32(np.asarray(points, np.float32).reshape(-1, 3))
    assert len(t) == len(p)
    out = np.zeros(len(t), np.float32)
    assert _lib().windingsim_tri(_ptr(t), _ptr(p), len(t), _ptr(out)) == 0
    return out


# ---- the reference: binary64 numpy, no code of the mirror ----
def solid_angle64(tri, q):
    """The signed solid angles of the triangles tri [m, 3, 3] seen from the points q [n, 3], binary64 [n, m] (van Oosterom-Strackee)."""
    tri, q = np.asarray(tri, np.float64), np.asarray(q, np.float64)
    a, b, c = (tri[None, :, k, :] - q[:, None, :] for k in range(3))
    la, lb, lc = (np.sqrt((v * v).sum(axis=-1)) for v in (a, b, c))
    det = (a * np.cross(b, c)).sum(axis=-1)
    den = la * lb * lc + (a * b).sum(axis=-1) * lc + (b * c).sum(axis=-1) * la + (c * a).sum(axis=-1) * lb
    return 2.0 * np.arctan2(det, den)


def winding64(geo, q, chunk=256, want_abs=False):
    """w(q) of a scene's primitives (point_helpers.Geometry) in binary64: triangles and the quads' two triangles by their solid angles,
    spheres by the inside test.  want_abs: (w, s) with s the sum of the terms' absolute values over 4 pi, the scale of the sum's rounding."""
    q = np.asarray(q, np.float32).astype(np.float64)[:, :3]
    tris = [geo.tri]
    if geo.nq:
        c00, c10, c11, c01 = geo.anchor, geo.anchor + geo.E1, geo.anchor + geo.E1 + geo.E2, geo.anchor + geo.E2
        tris.append(np.stack([np.stack([c00, c10, c11], axis=1), np.stack([c00, c11, c01], axis=1)], axis=1).reshape(-1, 3, 3))
    tris = np.concatenate(tris)
    w, s = np.zeros(len(q)), np.zeros(len(q))
    for i in range(0, len(q), chunk):
        if len(tris):
            om = solid_angle64(tris, q[i:i + chunk])
            w[i:i + chunk] = om.sum(axis=1) / (4.0 * np.pi)
            s[i:i + chunk] = np.abs(om).sum(axis=1) / (4.0 * np.pi)
    for k in range(geo.ns):
        inside = ((q - geo.centre[k]) ** 2).sum(axis=1) < geo.radius[k] ** 2
        w += inside; s += inside
    return (w, s) if want_abs else w


# ---- meshes ----
def cube(lo=-0.5, hi=0.5, inward=False, top=True):
    """The cube lo .. hi as 12 triangles wound outwards (inward: the other way); top=False leaves the +y face out (10 triangles)."""
    c = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.float64)      # index = 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]     # -x +x -y +y -z +z, outward
    if not top:
        quads.pop(3)
    f = []
    for a, b, cc, d in quads:
        f += [[c[a], c[b], c[cc]], [c[a], c[cc], c[d]]]
    f = np.array(f)
    return _f32(f[:, ::-1] if inward else f)


def uv_sphere(nu=48, nv=24, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """A UV sphere of nu x nv segments wound outwards, the degenerate triangles at the poles left out: 2 nu (nv - 1) triangles (2,208)."""
    u = np.linspace(0.0, 2.0 * np.pi, nu + 1); v = np.linspace(0.0, np.pi, nv + 1)
    p = lambda i, j: np.array([np.sin(v[j]) * np.cos(u[i % nu]), np.cos(v[j]), np.sin(v[j]) * np.sin(u[i % nu])])
    f = []
    for j in range(nv):
        for i in range(nu):
            a, b, c, d = p(i, j), p(i + 1, j), p(i + 1, j + 1), p(i, j + 1)
            if j > 0:
                f.append([a, b, c])
            if j < nv - 1:
                f.append([a, c, d])
    return _f32(np.array(f) * radius + np.asarray(centre))


_coffee = None


def mesh_scene(faces):
    """The faces (n, 3, 3) alone as a scene in coffee's frame, materials and lights (sign_helpers.mesh_scene's way: without coffee's three
    quads, which lie where the meshes are)."""
    global _coffee
    if _coffee is None:
        _coffee = M.HostScene("file:coffee", 64, 36)
    return _mesh_only(MovedScene(_coffee, np.asarray(faces, np.float32).reshape(-1, 9), new_faces=True))


def spheres_only():
    """The stand-in scene "spheres" without its quads: sphere primitives and nothing else."""
    return _mesh_only(MovedScene(M.HostScene("spheres", 64, 36)))


# ---- point sets ----
def box_points(lo, hi, n, seed, scale=1.5, thin=0.1):
    """n float32 points uniform in the box lo .. hi scaled by `scale` about its centre.  An axis along which the box is thinner than
    `thin` x its largest extent is taken as that thick: the box of a planar mesh has no volume, and every point of it lies on the surface."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = np.maximum(hi - lo, thin * max(float((hi - lo).max()), 1e-30))
    c, h = 0.5 * (lo + hi), 0.5 * scale * ext
    return _f32(np.random.default_rng(seed).uniform(c - h, c + h, (n, 3)))


def off_surface(hs_built, points, extent, share=1e-3):
    """Mask of the points further than share x extent from the surface, by the point queries' mirror: where a sign flip of a tiny det
    cannot move w by a half."""
    q = rows(points, INF)
    return pointsim(hs_built, q, "closest")["dist"] > np.float32(share * extent)
