"""The K-nearest point queries of the CPU mirror (tests/pointmultisim/pointmultisim.cpp, a library of its own beside libhostsim.so): the traversal through the kernel's
per-point code, and the definition itself as a loop over every primitive record; the checks the K-nearest tests share, and a binary64
distance from every point to every primitive that shares no code with the mirror."""
import ctypes as C
import os
import subprocess

import numpy as np

from common import REPO, _f32, _ptr, hostsim_handle, hostsim_lib
from point_helpers import POINT_DTYPE, quad_dist64, same_bits, sphere_dist64, tri_dist64      # noqa: F401  (same_bits: for the tests)

COUNT_ALL = 1                                             # MOPTIX_POINT_MULTI_COUNT_ALL, spelled out here apart from the package's definition
KS = (1, 2, 4, 8, 64)

_DIR = os.path.join(REPO, "tests", "pointmultisim")
_pointmultisim = None


def _lib():
    """tests/pointmultisim/libpointmultisim.so (built here if it is missing, as common.hostsim_lib builds its library) with the signatures
    of its four entries.  They take the handles of common.HostsimHandle."""
    global _pointmultisim
    if _pointmultisim is None:
        hostsim_lib()
        path = os.path.join(_DIR, "libpointmultisim.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _DIR, "-s"])
        L = C.CDLL(path)
        vp, f32p, i32p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.pointmultisim_query.argtypes, L.pointmultisim_query.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int, C.c_uint32, vp, i32p], C.c_int
        L.pointmultisim_brute.argtypes, L.pointmultisim_brute.restype = [vp, f32p, C.c_int64, C.c_int, C.c_uint32, vp, i32p], C.c_int
        L.pointmultisim_keys.argtypes, L.pointmultisim_keys.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int, C.c_uint32, vp, i32p], C.c_int
        L.pointmultisim_stack_depth.argtypes, L.pointmultisim_stack_depth.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int, C.c_uint32], C.c_int
        _pointmultisim = L
    return _pointmultisim


def _points(points):
    return _f32(np.asarray(points, np.float32).reshape(-1, 4))


def _records(n, k):
    """(n, k) zeroed POINT_DTYPE records at a 16-byte aligned address, which the mirror's 16-byte words need and numpy alone does not promise."""
    size = n * k * POINT_DTYPE.itemsize
    raw = np.zeros(size + 16, np.uint8)
    off = -raw.ctypes.data % 16
    return raw[off:off + size].view(POINT_DTYPE).reshape(n, k)


def pointmultisim(hs, points, max_near=4, count_all=False, node_format=64, leaf_size=4):
    """moptix_query_points_multi on the CPU, by the traversal: (hits (n, max_near) POINT_DTYPE, counts int32).  hs: a scene, or a built one."""
    sim = hostsim_handle(hs, leaf_size)
    pts = _points(points)
    hits, counts = _records(len(pts), max_near), np.zeros(len(pts), np.int32)
    rc = _lib().pointmultisim_query(sim._h, int(node_format), _ptr(pts), len(pts), int(max_near), COUNT_ALL if count_all else 0,
                                    hits.ctypes.data if max_near else None, _ptr(counts, C.c_int32))
    assert rc == 0
    return hits, counts


def pointmultibrute(hs, points, max_near=4, count_all=False, leaf_size=4):
    """The same from the definition: every primitive record through its distance function, the near set sorted by (d2, prim)."""
    sim = hostsim_handle(hs, leaf_size)
    pts = _points(points)
    hits, counts = _records(len(pts), max_near), np.zeros(len(pts), np.int32)
    rc = _lib().pointmultisim_brute(sim._h, _ptr(pts), len(pts), int(max_near), COUNT_ALL if count_all else 0,
                                    hits.ctypes.data if max_near else None, _ptr(counts, C.c_int32))
    assert rc == 0
    return hits, counts


def pointmultikeys(hs, points, max_near=4, count_all=False, node_format=64, leaf_size=4):
    """The traversal's list before it is turned into records: (d2 (n, max_near) float32, prim (n, max_near) int32, counts); entries behind
    min(max_near, count) are d2 = 0, prim = -1."""
    sim = hostsim_handle(hs, leaf_size)
    pts = _points(points)
    keys, counts = np.zeros((len(pts), max_near, 4), np.uint32), np.zeros(len(pts), np.int32)
    keys[:, :, 1] = 0xffffffff
    rc = _lib().pointmultisim_keys(sim._h, int(node_format), _ptr(pts), len(pts), int(max_near), COUNT_ALL if count_all else 0,
                                   keys.ctypes.data, _ptr(counts, C.c_int32))
    assert rc == 0
    return np.ascontiguousarray(keys[:, :, 0]).view(np.float32), np.ascontiguousarray(keys[:, :, 1]).view(np.int32), counts


def multi_stack_depth(hs, points, max_near=4, count_all=False, node_format=64, leaf_size=4):
    """Most stack entries the K-nearest walk of any of the points holds."""
    sim = hostsim_handle(hs, leaf_size)
    pts = _points(points)
    d = _lib().pointmultisim_stack_depth(sim._h, int(node_format), _ptr(pts), len(pts), int(max_near), COUNT_ALL if count_all else 0)
    assert d >= 0
    return d


def is_miss_record(h, max_dist):
    """Element-wise: the record is the closest mode's miss record with dist = max_dist's bits (h: (n, k) records, max_dist: (n,) float32)."""
    d_ok = h["dist"].view(np.uint32) == np.ascontiguousarray(max_dist, np.float32).view(np.uint32)[:, None]
    zero = (h["u"].view(np.uint32) == 0) & (h["v"].view(np.uint32) == 0) & (h["p"].view(np.uint32) == 0).all(axis=-1)
    return d_ok & (h["prim"] == -1) & (h["mat"] == -1) & zero


def gpu_point_set(pc):
    """The GPU tests' points of a point_helpers.PointCase: its near and special slices and the first 512 uniform points, as indices."""
    return np.concatenate([np.arange(512), np.arange(pc.parts["near"].start, len(pc.pts))])


def duplicates_scene():
    """lbvh_cases' "duplicates" (one triangle 100 times) alone in coffee's frame, without coffee's quads: prim = face id, triBase = 0."""
    from common import M, MovedScene
    from lbvh_cases import case_faces
    hs = MovedScene(M.HostScene("file:coffee", 64, 36), case_faces("duplicates"), new_faces=True)
    sizes = type(hs.sizes)()                              # a copy: the HostScene's own sizes keep their quads
    C.memmove(C.byref(sizes), C.byref(hs.sizes), C.sizeof(sizes))
    sizes.nQuads = 0
    hs.sizes = sizes
    return hs


class SmallCase:
    """A small scene for the all-pairs binary64 check: its geometry, n points of point_helpers.point_sets spread evenly over the three
    parts, and the two scales point_helpers.PointCase defines for a tolerance -- max(|q|_inf, the largest |coordinate|) of the box the
    points were drawn from, and of every primitive."""

    def __init__(self, hs, lo, hi, n=512):
        from point_helpers import Geometry, point_sets
        self.hs, self.geo = hs, Geometry(hs)
        g = self.geo
        pts, _ = point_sets(g, lo, hi)
        self.pts = pts[np.linspace(0, len(pts) - 1, n).astype(np.int64)]
        far = [np.abs(lo).max(), np.abs(hi).max()]
        if g.nt:
            far.append(np.abs(g.tri).max())
        if g.ns:
            far.append((np.abs(g.centre) + g.radius[:, None]).max())
        for k in range(g.nq):
            far.append(max(np.abs(g.anchor[k] + a * g.E1[k] + b * g.E2[k]).max() for a in (0, 1) for b in (0, 1)))
        qmax = np.abs(self.pts.astype(np.float64)).max(axis=1)
        self.scale_box = np.maximum(qmax, max(np.abs(lo).max(), np.abs(hi).max()))
        self.scale_all = np.maximum(qmax, max(far))


def all_pairs_dist64(geo, q):
    """Binary64 distances from every point q [n, 3] to every primitive of a point_helpers.Geometry, [n, ns + nq + nt] in the queries'
    numbering (spheres, quads, triangles): for small meshes."""
    q = np.asarray(q, np.float64)
    n = len(q)
    cols = [sphere_dist64(q, geo.centre[i], geo.radius[i]) for i in range(geo.ns)]
    cols += [quad_dist64(q, geo.anchor[i][None], geo.E1[i][None], geo.E2[i][None]) for i in range(geo.nq)]
    out = np.zeros((n, geo.ns + geo.nq + geo.nt))
    if cols:
        out[:, :geo.ns + geo.nq] = np.stack(cols, axis=1)
    step = max(1, (1 << 18) // max(n, 1))                 # triangles per chunk: about 2^18 pairs at a time
    for a in range(0, geo.nt, step):
        t = geo.tri[a:a + step]
        d = tri_dist64(np.repeat(q, len(t), axis=0), np.tile(t, (n, 1, 1)))[0]
        out[:, geo.ns + geo.nq + a:geo.ns + geo.nq + a + len(t)] = d.reshape(n, len(t))
    return out
