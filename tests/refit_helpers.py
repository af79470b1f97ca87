"""The refit operations of the CPU mirror (tests/hostsim/refitsim.cpp) on a built scene, the displacement the refit tests move vertices
with, and scenes whose vertices have been moved, for the fresh builds the refitted trees are compared with."""
import ctypes as C

import numpy as np

from common import M, HostsimHandle, MovedScene, RefitsimOut, _f32, _ptr, hostsim_lib, hostsim_render
from query_helpers import querysim


class RefitSim:
    """A scene built by the mirror's builder, then updated and refitted as a context would be.  It stays a built scene like any other:
    render and query are hostsim_render and querysim on the refitted tree."""

    def __init__(self, hs, leaf_size=4, builder=1):
        self._sim = HostsimHandle(hs, leaf_size, builder)
        self.n_faces, self.width, self.height = self._sim.n_faces, hs.width, hs.height

    def close(self):
        self._sim.close()

    def update(self, first, pos, nrm=None):
        pos = _f32(np.asarray(pos, np.float32).reshape(-1, 9))
        nrm = None if nrm is None else _f32(np.asarray(nrm, np.float32).reshape(-1, 9))
        assert hostsim_lib().refitsim_update(self._sim._h, int(first), len(pos), _ptr(pos), None if nrm is None else _ptr(nrm)) == 0

    def refit(self):
        assert hostsim_lib().refitsim_refit(self._sim._h) == 0
        return self

    def read(self):
        """dict(nodes [n, 32], nodes64 [n, 16] or None, tris [m, 12], shade [m, 12] uint32 words; rootRef, sahCost, sahCostBuilt)."""
        nf = max(1, self.n_faces)
        nodes = np.zeros((nf, 32), np.uint32); n64 = np.zeros((nf, 16), np.uint32)
        tris = np.zeros((nf, 12), np.uint32); shade = np.zeros((nf, 12), np.uint32)
        o = RefitsimOut(nodes.ctypes.data, n64.ctypes.data, tris.ctypes.data, shade.ctypes.data)
        assert hostsim_lib().refitsim_read(self._sim._h, C.byref(o)) == 0
        return dict(nodes=nodes[:o.nNodes], nodes64=n64[:o.nNodes] if o.has64 else None, tris=tris[:self.n_faces], shade=shade[:self.n_faces],
                    rootRef=int(o.rootRef), sahCost=float(o.sahCost), sahCostBuilt=float(o.sahCostBuilt))

    def render(self, seeds, node_format=128):
        return hostsim_render(self._sim, seeds, node_format=node_format)

    def query(self, rays, mode="closest", node_format=64):
        return querysim(self._sim, rays, mode, node_format=node_format)


# ---- the displacement: p + a sin(k p.yzx + phi), per vertex position, so vertices that faces share stay shared ----
WAVE_K, WAVE_PHI = np.float32(7.0), np.float32(0.3)


def extent(hs):
    p = hs.flat()["positions"]
    return float((p.max(axis=0) - p.min(axis=0)).max())


def displace(positions, amplitude, k=WAVE_K, phi=WAVE_PHI):
    """float32 in, float32 out; a function of the position alone."""
    p = np.asarray(positions, np.float32)
    arg = (np.float32(k) * p[..., [1, 2, 0]] + np.float32(phi)).astype(np.float32)
    return (p + np.float32(amplitude) * np.sin(arg.astype(np.float64)).astype(np.float32)).astype(np.float32)


def strip_scene(n):
    """n triangles in a zigzag strip with one wide step after the fourth vertex, in coffee's frame, materials and lights: with 7 triangles
    and one per leaf, either builder emits nodes with 2, 3 and 4 children."""
    x = np.cumsum([0.0] + [0.3 if i == 3 else 0.1 for i in range(n + 1)]) - 0.7
    v = np.array([[x[i], 0.2 + 0.3 * (i % 2), 0.05 * i] for i in range(n + 2)], np.float32)
    faces = np.array([[i, i + 1, i + 2] for i in range(n)], np.int32)
    return MovedScene(M.HostScene("file:coffee", 64, 36), v[faces.reshape(-1)].reshape(n, 9), new_faces=True)


def moved_faces(hs, amplitude_share, first=0, count=None):
    """(face_pos [nFaces, 9] of the whole scene after the move, the moved range's rows): the faces first .. first + count displaced by
    amplitude_share of the scene's extent, the others as they are."""
    fp = hs.face_arrays()[0].copy()
    count = len(fp) - first if count is None else count
    fp[first:first + count] = displace(fp[first:first + count].reshape(-1, 3), amplitude_share * extent(hs)).reshape(-1, 9)
    return fp, fp[first:first + count].copy()


def wide_strip(n=7):
    """(strip_scene(n), its face positions with the last vertex moved so far out that a node spanning it is too wide for the 64-byte form's
    grid: 255 steps of at most 6e7 units, pt_lbvh.h kNode64MaxStep)."""
    hs = strip_scene(n)
    fp = hs.face_arrays()[0].copy()
    fp[n - 1, 6] = np.float32(3e10)
    return hs, fp


def new_normals(hs, first=0, count=None):
    """Rows of other unit normals for the faces first .. first + count: the scene's own, tilted by a function of the corner's position;
    the faces without normals get a non-zero vector too, which an update has to ignore."""
    fp, fn, has, _ = hs.face_arrays()
    count = len(fp) - first if count is None else count
    p = fp[first:first + count].reshape(-1, 3).astype(np.float64)
    n = fn[first:first + count].reshape(-1, 3).astype(np.float64) + 0.5 * np.sin(5.0 * p[:, [2, 0, 1]] + 0.7)
    n[np.linalg.norm(n, axis=1) < 0.1] = (0.0, 1.0, 0.0)
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32).reshape(-1, 9)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_words(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()
