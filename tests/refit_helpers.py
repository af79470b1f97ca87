"""Bindings of tests/refitsim (the CPU mirror of the mesh refit), the displacement the refit tests move vertices with, and a scene whose
vertices have been moved, for the fresh builds the refitted trees are compared with."""
import ctypes as C
import os
import subprocess

import numpy as np

from common import M, REPO, HostsimScene, _hostsim_scene, hostsim_lib
from query_helpers import HIT_DTYPE

K = M._capi
_REFITSIM_DIR = os.path.join(REPO, "tests", "refitsim")
_refitsim = None


class RefitsimOut(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("nodes64", C.c_void_p), ("tris", C.c_void_p), ("shade", C.c_void_p),
                ("nNodes", C.c_int32), ("rootRef", C.c_int32), ("has64", C.c_int32), ("sahCost", C.c_double), ("sahCostBuilt", C.c_double)]


def refitsim_lib():
    global _refitsim
    if _refitsim is None:
        path = os.path.join(_REFITSIM_DIR, "librefitsim.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _REFITSIM_DIR, "-s"])
        L = C.CDLL(path)
        f32p, i32p, vp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p
        L.refitsim_create.argtypes = [C.POINTER(HostsimScene), C.c_int]; L.refitsim_create.restype = vp
        L.refitsim_free.argtypes = [vp]; L.refitsim_free.restype = None
        L.refitsim_update.argtypes = [vp, C.c_int32, C.c_int32, f32p, f32p]
        L.refitsim_refit.argtypes = [vp]
        L.refitsim_read.argtypes = [vp, C.POINTER(RefitsimOut)]
        L.refitsim_render.argtypes = [vp, C.c_int, i32p, C.c_int, f32p, C.POINTER(C.c_uint64)]
        L.refitsim_query.argtypes = [vp, C.c_int, f32p, C.c_int64, C.c_int, vp]
        L.hostsim_set_builder.argtypes = [C.c_int]
        _refitsim = L
    return _refitsim


class RefitSim:
    """A scene built by the mirror's builder, then updated and refitted as a context would be."""

    def __init__(self, hs, leaf_size=4, builder=1):
        L = refitsim_lib()
        self._s, self._keep = _hostsim_scene(hs)
        self.n_faces = int(self._s.nFaces)
        L.hostsim_set_builder(int(builder))            # librefitsim's own copy of hostsim's switch
        self._h = L.refitsim_create(C.byref(self._s), int(leaf_size))
        L.hostsim_set_builder(1)
        self.width, self.height = hs.width, hs.height

    def close(self):
        if self._h:
            refitsim_lib().refitsim_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def update(self, first, pos, nrm=None):
        pos = np.ascontiguousarray(np.asarray(pos, np.float32).reshape(-1, 9))
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        nrm = None if nrm is None else np.ascontiguousarray(np.asarray(nrm, np.float32).reshape(-1, 9))
        assert refitsim_lib().refitsim_update(self._h, int(first), len(pos), fp(pos), None if nrm is None else fp(nrm)) == 0

    def refit(self):
        assert refitsim_lib().refitsim_refit(self._h) == 0
        return self

    def read(self):
        """dict(nodes [n, 32], nodes64 [n, 16] or None, tris [m, 12], shade [m, 12] uint32 words; rootRef, sahCost, sahCostBuilt)."""
        nf = max(1, self.n_faces)
        nodes = np.zeros((nf, 32), np.uint32); n64 = np.zeros((nf, 16), np.uint32)
        tris = np.zeros((nf, 12), np.uint32); shade = np.zeros((nf, 12), np.uint32)
        o = RefitsimOut(nodes.ctypes.data, n64.ctypes.data, tris.ctypes.data, shade.ctypes.data)
        assert refitsim_lib().refitsim_read(self._h, C.byref(o)) == 0
        return dict(nodes=nodes[:o.nNodes], nodes64=n64[:o.nNodes] if o.has64 else None, tris=tris[:self.n_faces], shade=shade[:self.n_faces],
                    rootRef=int(o.rootRef), sahCost=float(o.sahCost), sahCostBuilt=float(o.sahCostBuilt))

    def render(self, seeds, node_format=128):
        seeds = np.ascontiguousarray(np.asarray(seeds, np.int32))
        accum = np.zeros((self.height, self.width, 3), np.float32)
        cnt = (C.c_uint64 * 9)()
        assert refitsim_lib().refitsim_render(self._h, int(node_format), seeds.ctypes.data_as(C.POINTER(C.c_int32)), len(seeds),
                                              accum.ctypes.data_as(C.POINTER(C.c_float)), cnt) == 0
        from common import HOSTSIM_COUNTERS
        return accum, dict(zip(HOSTSIM_COUNTERS, [int(x) for x in cnt]))

    def query(self, rays, mode="closest", node_format=64):
        rays = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 8))
        out = np.zeros(len(rays), HIT_DTYPE if mode == "closest" else np.int32)
        assert refitsim_lib().refitsim_query(self._h, int(node_format), rays.ctypes.data_as(C.POINTER(C.c_float)), len(rays),
                                             0 if mode == "closest" else 1, C.c_void_p(out.ctypes.data)) == 0
        return out


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


class MovedScene:
    """hs with other face positions: what the oracle, hostsim and a context's upload see of a HostScene, over a copy of its flat arrays.
    The faces carry the move (one vertex per corner), so a move of a face range may tear vertices apart that faces share, exactly as
    moptix_update_faces on that range does.  face_nrm: other normals too ([nFaces, 9]; a face without normals keeps none, as
    moptix_update_faces leaves it).  drop_normals: a mask of faces that lose their normals (they shade flat).  new_faces: other faces altogether (no normals, no texcoords, material 0)."""

    def __init__(self, hs, face_pos, new_faces=False, face_nrm=None, drop_normals=None):
        self._base = hs
        self.kind, self.sizes, self.params, self.accel = hs.kind, hs.sizes, hs.params, hs.accel
        self.aabb_min, self.aabb_max = hs.aabb_min, hs.aabb_max
        self._face_pos = np.ascontiguousarray(np.asarray(face_pos, np.float32).reshape(-1, 9))
        f = dict(hs.flat())
        nf = len(self._face_pos)
        f["positions"] = np.ascontiguousarray(self._face_pos.reshape(-1, 3))      # one vertex per corner
        f["vIdx"] = np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)
        if drop_normals is not None:
            f["nIdx"] = np.where(np.asarray(drop_normals, bool)[:, None], np.int32(-1), f["nIdx"]).astype(np.int32)
        if face_nrm is not None:
            has = (np.asarray(f["nIdx"]) >= 0).all(axis=1)
            f["normals"] = np.ascontiguousarray(np.asarray(face_nrm, np.float32).reshape(-1, 3))      # one normal per corner
            f["nIdx"] = np.where(has[:, None], np.arange(3 * nf, dtype=np.int32).reshape(nf, 3), np.int32(-1)).astype(np.int32)
        if new_faces:
            f["nIdx"] = np.full((nf, 3), -1, np.int32); f["tIdx"] = np.full((nf, 3), -1, np.int32); f["faceMat"] = np.zeros(nf, np.int32)
        self._flat = f

    width = property(lambda self: int(self.params.width))
    height = property(lambda self: int(self.params.height))

    def flat(self):
        return self._flat

    to_dict = M.HostScene.to_dict
    face_arrays = M.HostScene.face_arrays
    face_uvs = M.HostScene.face_uvs

    def upload(self, ctx):
        """mohost_scene_upload's sequence of calls (host/scenes.cpp upload) from the flat arrays: one moptix_add_mesh per run of faces
        with one material, which numbers the faces as the original upload does."""
        L, h, f, s = K.device_lib(), ctx._h, self._flat, self.sizes
        chk = ctx._chk
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        chk(L.moptix_clear_scene(h)); chk(L.moptix_set_params(h, C.byref(self.params)))
        for t in f["textures"]:
            t = np.ascontiguousarray(t, np.float32)
            chk(L.moptix_add_texture(h, fp(t), t.shape[1], t.shape[0], None))
        for i in range(s.nMaterials):
            chk(L.moptix_add_material(h, C.byref(f["materials"][i]), None))
        if s.nSpheres:
            chk(L.moptix_add_spheres(h, f["spheres"], ip(np.ascontiguousarray(f["sphereMat"], np.int32)), s.nSpheres))
        if s.nQuads:
            chk(L.moptix_add_quads(h, f["quads"], ip(np.ascontiguousarray(f["quadMat"], np.int32)), s.nQuads))
        pos = np.ascontiguousarray(f["positions"], np.float32); nrm = np.ascontiguousarray(f["normals"], np.float32)
        uv = np.ascontiguousarray(f["texcoords"], np.float32)
        fm = np.asarray(f["faceMat"], np.int32)
        cuts = [0] + [i for i in range(1, len(fm)) if fm[i] != fm[i - 1]] + [len(fm)] if len(fm) else [0]
        for a, b in zip(cuts[:-1], cuts[1:]):
            vi = np.ascontiguousarray(f["vIdx"][a:b], np.int32); ni = np.ascontiguousarray(f["nIdx"][a:b], np.int32)
            ti = np.ascontiguousarray(f["tIdx"][a:b], np.int32)
            chk(L.moptix_add_mesh(h, fp(pos), len(pos), fp(nrm) if len(nrm) else None, len(nrm), fp(uv) if len(uv) else None, len(uv),
                                  ip(vi), ip(ni), ip(ti), b - a, int(fm[a])))
        chk(L.moptix_set_lights(h, f["lights"] if s.nLights else None, s.nLights))
        chk(L.moptix_build_accel(h, self.accel.encode()))


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
