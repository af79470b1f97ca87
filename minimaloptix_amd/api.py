"""Thin Python wrappers over the C ABI (include/moptix.h, include/moptix_host.h)."""
import ctypes as C
import os

import numpy as np

from . import _capi as K
from ._capi import MoptixError


# moptix_hit as a numpy record (include/moptix.h "ray queries")
HIT_DTYPE = np.dtype([("t", np.float32), ("prim", np.int32), ("mat", np.int32), ("u", np.float32), ("v", np.float32), ("ng", np.float32, (3,))])
assert HIT_DTYPE.itemsize == C.sizeof(K.Hit) == 32
POINT_DTYPE = np.dtype([("dist", np.float32), ("prim", np.int32), ("mat", np.int32), ("u", np.float32), ("v", np.float32), ("p", np.float32, (3,))])
assert POINT_DTYPE.itemsize == C.sizeof(K.PointHit) == 32
# moptix_sweep_hit as a numpy record (include/moptix.h "sweep queries")
SWEEP_DTYPE = np.dtype([("t", np.float32), ("prim", np.int32), ("mat", np.int32), ("u", np.float32), ("v", np.float32), ("p", np.float32, (3,))])
assert SWEEP_DTYPE.itemsize == 32
SEGMENT_DTYPE = np.dtype([("dist", np.float32), ("prim", np.int32), ("mat", np.int32), ("s", np.float32), ("p", np.float32, (3,)), ("feature", np.int32)])
assert SEGMENT_DTYPE.itemsize == 32


def scenes_dir():
    """Folder holding `<name>/<name>.scene` (the reference's baseSceneFolder "scenes/")."""
    return os.path.join(K.REPO_ROOT, "scenes") + "/"


def _tea16(v0, v1):
    """utils_device.h:8-22 (integer; used only for the seed schedule on the host)."""
    v0 &= 0xffffffff; v1 &= 0xffffffff; s0 = 0
    for _ in range(16):
        s0 = (s0 + 0x9e3779b9) & 0xffffffff
        v0 = (v0 + ((((v1 << 4) + 0xa341316c) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4)) & 0xffffffff)) & 0xffffffff
        v1 = (v1 + ((((v0 << 4) + 0xad90777d) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761e)) & 0xffffffff)) & 0xffffffff
    return v0


def launch_seeds(n, base_seed=0, first=0):
    """Seed schedule: launchSeed(i) = (int)tea<16>(i, baseSeed)."""
    return np.array([_tea16(first + i, base_seed) for i in range(n)], dtype=np.uint32).view(np.int32)


def _check_tensor(who, name, t, dtypes, shape, expect, device=None, on_gpu=True):
    """ValueError unless `t`, the argument `name` of the method `who`, is a torch tensor whose data_ptr a kernel can take: on the GPU
    (on_gpu) and there on GPU `device` (an index, or None for any), contiguous, of `shape` -- an element count or a predicate, worded for
    the message by `expect` -- and of one of `dtypes`."""
    if on_gpu and (not hasattr(t, "data_ptr") or not t.is_cuda):
        raise ValueError("%s: %s must live on the GPU (its data_ptr is handed to a kernel); numpy arrays take the host path" % (who, name))
    if not t.is_contiguous() or not (shape(t) if callable(shape) else t.numel() == shape):
        raise ValueError("%s: %s must be a contiguous tensor of %s" % (who, name, expect))
    if str(t.dtype) not in dtypes:
        raise ValueError("%s: %s has dtype %s" % (who, name, t.dtype))
    if device is not None and t.device.index != device:
        raise ValueError("%s: %s is on %s, the context on GPU %d" % (who, name, t.device, device))


def _rows(k):
    """_check_tensor's shape predicate for an (n, k) tensor."""
    return lambda t: t.dim() == 2 and t.shape[1] == k


def _record_views(out, first, last):
    """The (n, 8) -- or, for a multi-hit query, (n, k, 8) -- float32 tensor of moptix_hit / moptix_point_hit records as a dict of views:
    "records" itself, word 0 under the name `first`, prim, mat, u, v, and words 5 .. 7 under the name `last`."""
    import torch
    ints = out.view(torch.int32)
    return {"records": out, first: out[..., 0], "prim": ints[..., 1], "mat": ints[..., 2], "u": out[..., 3], "v": out[..., 4], last: out[..., 5:8]}


def _point_rows(who, points, max_dist):
    """The host path's queries of the point queries `who`: (n, 3) positions with max_dist a scalar or an (n,) array, or (n, 4) rows
    x y z maxDist, as one contiguous (n, 4) float32 array."""
    pts = np.asarray(points, np.float32)
    if pts.ndim != 2 or pts.shape[1] not in (3, 4):
        raise ValueError("%s: points must be (n, 3) or (n, 4), not %r" % (who, pts.shape))
    if pts.shape[1] == 3:
        md = np.asarray(max_dist, np.float32)
        if md.ndim > 1 or (md.ndim == 1 and len(md) != len(pts)):
            raise ValueError("%s: max_dist must be a scalar or one value per point" % who)
        pts = np.concatenate([pts, np.broadcast_to(md.reshape(-1, 1) if md.ndim else md, (len(pts), 1))], axis=1)
    return np.ascontiguousarray(pts, np.float32)


def occupancy_boxes(lo, hi, dims):
    """The cells of the regular grid of dims = (nx, ny, nz) cells between the corners lo and hi as (nx * ny * nz, 6) float32 boxes
    lox loy loz hix hiy hiz, x slowest (row i * ny * nz + j * nz + k is cell (i, j, k)).  The cell planes come from one float32 linspace
    per axis, so neighbouring cells share their planes exactly: a primitive on a shared plane meets both."""
    lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError("occupancy_boxes: dims %r (three cell counts >= 1)" % (dims,))
    planes = [np.linspace(lo[a], hi[a], dims[a] + 1, dtype=np.float32) for a in range(3)]
    cells_lo = np.stack(np.meshgrid(*[p[:-1] for p in planes], indexing="ij"), axis=-1).reshape(-1, 3)
    cells_hi = np.stack(np.meshgrid(*[p[1:] for p in planes], indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([cells_lo, cells_hi], axis=1), np.float32)


def oriented_boxes(centre, half, rotation):
    """Oriented boxes as the (n, 16) float32 rows Context.query_obbs takes: centre (n, 3); half (n, 3) or (3,), the half-extents along the
    box's own axes; rotation (n, 3, 3) or (3, 3), the usual local-to-world matrix, whose columns are the box axes as world-space
    directions -- floats 6..14 of a row are its transpose, axis by axis.  The sixteenth float is 0 and is not read."""
    c = np.asarray(centre, np.float32)
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError("oriented_boxes: centre must be (n, 3), not %r" % (c.shape,))
    n = len(c)
    h, r = np.asarray(half, np.float32), np.asarray(rotation, np.float32)
    if h.shape not in ((n, 3), (3,)):
        raise ValueError("oriented_boxes: half must be (n, 3) or (3,), not %r" % (h.shape,))
    if r.shape not in ((n, 3, 3), (3, 3)):
        raise ValueError("oriented_boxes: rotation must be (n, 3, 3) or (3, 3), not %r" % (r.shape,))
    out = np.zeros((n, 16), np.float32)
    out[:, 0:3] = c
    out[:, 3:6] = h
    out[:, 6:15] = np.swapaxes(np.broadcast_to(r, (n, 3, 3)), 1, 2).reshape(n, 9)
    return out


def frustum_planes(matrix, depth="gl"):
    """The six inward planes of a clip matrix as the (n, 24) float32 rows Context.query_frusta takes (Gribb-Hartmann): matrix (4, 4) or
    (n, 4, 4) with clip = M @ (x, y, z, 1); a single matrix gives one row.  The order is left, right, bottom, top, near, far: -w <= x <= w,
    -w <= y <= w, and for depth="gl" -w <= z <= w, for depth="zero" 0 <= z <= w.  The planes are the sums and differences of the matrix
    rows, computed in binary64 and rounded to binary32 once; they are not normalised (the queries do not need it)."""
    if depth not in ("gl", "zero"):
        raise ValueError("frustum_planes: depth %r (\"gl\" or \"zero\")" % (depth,))
    m = np.asarray(matrix, np.float64)
    if m.shape[-2:] != (4, 4) or m.ndim not in (2, 3):
        raise ValueError("frustum_planes: matrix must be (4, 4) or (n, 4, 4), not %r" % (m.shape,))
    m = m.reshape(-1, 4, 4)
    x, y, z, w = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
    planes = np.stack([w + x, w - x, w + y, w - y, w + z if depth == "gl" else z, w - z], axis=1)
    return np.ascontiguousarray(planes.reshape(-1, 24), np.float32)


def camera_frusta(cam, rects, near=0.0, far=float("inf")):
    """The regions the renderer's own camera sees through rectangles of its screen, as (n, 24) float32 rows for Context.query_frusta.
    cam: a moptix_cam_params (HostScene.params.cam) or the mapping HostScene.to_dict()["cam"] gives; rects (n, 4) x0 y0 x1 y1 in screen
    fractions [0, 1] -- the xy that the renderer multiplies `horizontal` and `vertical` by, so (0, 0, 1, 1) is the whole frame and pixel
    (i, j) of a W x H frame is (i / W, j / H, (i + 1) / W, (j + 1) / H).  The order is left, right, bottom, top, near, far.  The four
    side planes go through `origin` and the corner directions (scrLowerLeftCorner + horizontal x + vertical y) - origin; near and far are
    perpendicular to the view axis (the screen's normal) at those distances from the origin: near = 0 is the plane through the origin,
    far = inf a zero plane, which constrains nothing.  Planes are computed in binary64 with unit normals, oriented inwards and rounded to
    binary32 once.  lensRadius plays no part: this is the pinhole camera's region, and rays of a thin lens leave it near the camera."""
    get = (lambda k: cam[k]) if isinstance(cam, dict) or hasattr(cam, "keys") else (lambda k: _f3(getattr(cam, k)))
    o, h, v, ll = (np.asarray(get(k), np.float64).reshape(3) for k in ("origin", "horizontal", "vertical", "scrLowerLeftCorner"))
    r = np.asarray(rects, np.float64)
    if r.ndim != 2 or r.shape[1] != 4:
        raise ValueError("camera_frusta: rects must be (n, 4) x0 y0 x1 y1, not %r" % (r.shape,))
    near, far = float(near), float(far)
    if not (np.isfinite(r).all() and (r[:, 0] <= r[:, 2]).all() and (r[:, 1] <= r[:, 3]).all() and 0.0 <= near <= far):
        raise ValueError("camera_frusta: rects need finite x0 <= x1 and y0 <= y1, and 0 <= near <= far")
    corner = lambda x, y: (ll - o)[None, :] + x[:, None] * h[None, :] + y[:, None] * v[None, :]
    c00, c01, c10, c11 = corner(r[:, 0], r[:, 1]), corner(r[:, 0], r[:, 3]), corner(r[:, 2], r[:, 1]), corner(r[:, 2], r[:, 3])

    def side(a, b, inward, sign):
        n = np.cross(a, b)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        n *= np.where(sign * (n @ inward) >= 0, 1.0, -1.0)[:, None]
        return np.concatenate([n, -(n @ o)[:, None]], axis=1)
    axis = np.cross(h, v)
    axis /= np.linalg.norm(axis)
    if axis @ (ll + 0.5 * h + 0.5 * v - o) < 0:
        axis = -axis
    n = len(r)
    near_p = np.broadcast_to(np.concatenate([axis, [-(axis @ o) - near]]), (n, 4))
    far_p = np.broadcast_to(np.concatenate([-axis, [(axis @ o) + far]]) if np.isfinite(far) else np.zeros(4), (n, 4))
    planes = np.stack([side(c00, c01, h, 1.0), side(c10, c11, h, -1.0), side(c00, c10, v, 1.0), side(c01, c11, v, -1.0), near_p, far_p], axis=1)
    return np.ascontiguousarray(planes.reshape(n, 24), np.float32)


def _f3(v):
    return [float(v.x), float(v.y), float(v.z)]


class HostScene:
    """A scene built by the C++ host library (scene.cpp/tinyobj/setupScene equivalents)."""

    def __init__(self, kind, width, height, iarg=0, farg=0.0, base_folder=None, skip_missing=True):
        L = K.host_lib()
        self._h = C.c_void_p()
        base = (base_folder or scenes_dir()).encode()
        rc = L.mohost_scene_build(kind.encode(), base, width, height, int(iarg), float(farg), 1 if skip_missing else 0,
                                  C.byref(self._h))
        if rc != K.MOPTIX_OK:
            raise MoptixError(rc, L.mohost_last_error().decode())
        self.kind = kind
        self.sizes = K.SceneSizes()
        L.mohost_scene_get_sizes(self._h, C.byref(self.sizes))
        self.params = K.Params()
        amin, amax, accel = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_char * 16)()
        L.mohost_scene_get_params(self._h, C.byref(self.params), amin, amax, accel)
        self.aabb_min, self.aabb_max = np.array(list(amin), np.float32), np.array(list(amax), np.float32)
        self.accel = accel.value.decode()
        self.warnings = [L.mohost_scene_warning(self._h, i).decode() for i in range(self.sizes.nWarnings)]
        self._flat = None

    def __del__(self):
        try:
            if self._h:
                K.host_lib().mohost_scene_free(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def width(self):
        return int(self.params.width)

    @property
    def height(self):
        return int(self.params.height)

    def upload(self, ctx):
        rc = K.host_lib().mohost_scene_upload(self._h, ctx._h)
        if rc != K.MOPTIX_OK:
            raise MoptixError(rc, ctx.last_error())

    def flat(self):
        """Flattened arrays (ctypes records + numpy) of the whole scene."""
        if self._flat is None:
            s = self.sizes
            mats = (K.Material * max(1, s.nMaterials))()
            sph = (K.SphereParams * max(1, s.nSpheres))(); smat = np.zeros(max(1, s.nSpheres), np.int32)
            quads = (K.QuadParams * max(1, s.nQuads))(); qmat = np.zeros(max(1, s.nQuads), np.int32)
            lights = (K.LightParams * max(1, s.nLights))()
            pos = np.zeros((max(1, s.nVerts), 3), np.float32); nrm = np.zeros((max(1, s.nNormals), 3), np.float32)
            vi = np.zeros((max(1, s.nFaces), 3), np.int32); ni = np.zeros((max(1, s.nFaces), 3), np.int32)
            fm = np.zeros(max(1, s.nFaces), np.int32)
            ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
            fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
            K.host_lib().mohost_scene_copy(self._h, mats, sph, ip(smat), quads, ip(qmat), lights, fp(pos), fp(nrm),
                                           ip(vi), ip(ni), ip(fm))
            uv = np.zeros((max(1, s.nTexcoords), 2), np.float32); ti = np.full((max(1, s.nFaces), 3), -1, np.int32)
            K.host_lib().mohost_scene_copy_texcoords(self._h, fp(uv), ip(ti))
            textures = []
            for t in range(s.nTextures):
                w, h = C.c_int32(), C.c_int32()
                K.host_lib().mohost_scene_texture(self._h, t, C.byref(w), C.byref(h), None)
                px = np.zeros((h.value, w.value, 4), np.float32)
                K.host_lib().mohost_scene_texture(self._h, t, None, None, fp(px))
                textures.append(px)
            self._flat = dict(materials=mats, spheres=sph, sphereMat=smat[:s.nSpheres], quads=quads, quadMat=qmat[:s.nQuads],
                              lights=lights, positions=pos[:s.nVerts], normals=nrm[:s.nNormals], vIdx=vi[:s.nFaces],
                              nIdx=ni[:s.nFaces], faceMat=fm[:s.nFaces], texcoords=uv[:s.nTexcoords], tIdx=ti[:s.nFaces],
                              textures=textures)
        return self._flat

    def to_dict(self):
        """Plain-python description (what oracle.oracle.Scene consumes)."""
        f, s, p = self.flat(), self.sizes, self.params
        mats = []
        for i in range(s.nMaterials):
            m = f["materials"][i]; d = m.disney
            e = _f3(d.emission) if m.kind == K.MAT_DISNEY else _f3(m.emission)
            mats.append(dict(kind=int(m.kind), albedo=_f3(m.albedo), fuzz=float(m.fuzz), refIdx=float(m.refIdx), emission=e,
                             color=_f3(d.color), metallic=d.metallic, subsurface=d.subsurface, specular=d.specular,
                             roughness=d.roughness, specularTint=d.specularTint, anisotropic=d.anisotropic, sheen=d.sheen,
                             sheenTint=d.sheenTint, clearcoat=d.clearcoat, clearcoatGloss=d.clearcoatGloss,
                             brdfType=int(d.brdfType), albedoID=int(d.albedoID)))
        spheres = np.array([[*_f3(f["spheres"][i].center), f["spheres"][i].radius] for i in range(s.nSpheres)], np.float32).reshape(-1, 4)
        quads = np.array([[q.plane.x, q.plane.y, q.plane.z, q.plane.w, *_f3(q.v1), *_f3(q.v2), *_f3(q.anchor)]
                          for q in (f["quads"][i] for i in range(s.nQuads))], np.float32).reshape(-1, 13)
        lights = [dict(position=_f3(l.position), normal=_f3(l.normal), emission=_f3(l.emission), u=_f3(l.u), v=_f3(l.v),
                       area=float(l.area), radius=float(l.radius), shape=int(l.shape))
                  for l in (f["lights"][i] for i in range(s.nLights))]
        cam = p.cam
        return dict(width=int(p.width), height=int(p.height),
                    cam=dict(origin=_f3(cam.origin), horizontal=_f3(cam.horizontal), vertical=_f3(cam.vertical),
                             scrLowerLeftCorner=_f3(cam.scrLowerLeftCorner), u=_f3(cam.u), v=_f3(cam.v),
                             lensRadius=float(cam.lensRadius)),
                    bgColor=_f3(p.bgColor), rayMaxDepth=int(p.rayMaxDepth), rayMinIntensity=float(p.rayMinIntensity),
                    rayEpsilonT=float(p.rayEpsilonT), materials=mats, spheres=spheres, sphereMat=f["sphereMat"],
                    quads=quads, quadMat=f["quadMat"], lights=lights, positions=f["positions"], normals=f["normals"],
                    vIdx=f["vIdx"], nIdx=f["nIdx"], faceMat=f["faceMat"], texcoords=f["texcoords"], tIdx=f["tIdx"],
                    textures=f["textures"])

    def face_arrays(self):
        """Per-face positions / normals (9 floats each) + flags, as moptix_add_mesh flattens them."""
        f = self.flat()
        vi, ni = f["vIdx"], f["nIdx"]
        nf = len(vi)
        face_pos = np.ascontiguousarray(f["positions"][vi.reshape(-1)].reshape(nf, 9)) if nf else np.zeros((0, 9), np.float32)
        has = (ni >= 0).all(axis=1).astype(np.int32) if nf else np.zeros(0, np.int32)
        face_nrm = np.zeros((nf, 9), np.float32)
        if nf and has.any():
            idx = np.where(has.astype(bool))[0]
            face_nrm[idx] = f["normals"][ni[idx].reshape(-1)].reshape(-1, 9)
        return face_pos, face_nrm, has, f["faceMat"]

    def face_uvs(self):
        """Per-face texcoords (6 floats: u0 v0 u1 v1 u2 v2) + flags, as moptix_add_mesh flattens them."""
        f = self.flat()
        ti = f["tIdx"]
        nf = len(ti)
        has = (ti >= 0).all(axis=1).astype(np.int32) if nf else np.zeros(0, np.int32)
        uv = np.zeros((nf, 6), np.float32)
        if nf and has.any():
            idx = np.where(has.astype(bool))[0]
            uv[idx] = f["texcoords"][ti[idx].reshape(-1)].reshape(-1, 6)
        return uv, has


class Context:
    """One moptix_context (one GPU)."""

    def __init__(self, device=0):
        self._L = K.device_lib()
        self._h = C.c_void_p()
        rc = self._L.moptix_create(C.byref(self._h), device)
        if rc != K.MOPTIX_OK:
            raise MoptixError(rc, self._L.moptix_last_error(None).decode())
        self.device = int(device)
        self.width = self.height = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.moptix_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return self._L.moptix_last_error(self._h).decode()

    def _chk(self, rc):
        if rc != K.MOPTIX_OK:
            raise MoptixError(rc, self.last_error())

    def load(self, scene):
        """Upload a HostScene (set_params + add_* + build_accel) and validate."""
        scene.upload(self)
        self.width, self.height = scene.width, scene.height
        self._chk(self._L.moptix_validate(self._h))

    def set_params(self, params):
        self._chk(self._L.moptix_set_params(self._h, C.byref(params)))
        self.width, self.height = int(params.width), int(params.height)

    def set_option(self, name, value):
        self._chk(self._L.moptix_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int32()
        self._chk(self._L.moptix_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def set_partition(self, rank, nranks):
        self._chk(self._L.moptix_set_partition(self._h, rank, nranks))

    def update_spheres(self, first, spheres, n):
        """spheres: ctypes array of SphereParams (updateVideo, MinimalOptiX.cpp:763-764)."""
        self._chk(self._L.moptix_update_spheres(self._h, int(first), spheres, int(n)))

    def build_accel(self, kind):
        self._chk(self._L.moptix_build_accel(self._h, kind.encode()))

    def accel_info(self):
        a = K.AccelInfo()
        self._chk(self._L.moptix_get_accel_info(self._h, C.byref(a)))
        return a

    def _frame(self, k=3, dtype=np.float32):
        """An (H, W, k) output array, (H, W) for k = 0, and its pointer as the C ABI takes it."""
        out = np.empty((self.height, self.width, k) if k else (self.height, self.width), dtype)
        return out, out.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dtype)))

    @staticmethod
    def _seeds(seeds):
        s = np.ascontiguousarray(np.asarray(seeds, dtype=np.int32))
        return s, s.ctypes.data_as(C.POINTER(C.c_int32))

    def launch(self, seed):
        self._chk(self._L.moptix_launch(self._h, int(seed)))

    def render(self, seeds):
        s, p = self._seeds(seeds)
        self._chk(self._L.moptix_render(self._h, p, len(s)))

    def render_async(self, seeds):
        s, p = self._seeds(seeds)
        self._chk(self._L.moptix_render_async(self._h, p, len(s)))

    def sync(self):
        self._chk(self._L.moptix_sync(self._h))

    def render_counted(self, seeds):
        s, p = self._seeds(seeds)
        st = K.Stats()
        self._chk(self._L.moptix_render_counted(self._h, p, len(s), C.byref(st)))
        return st

    def accum_read(self):
        out, p = self._frame()
        self._chk(self._L.moptix_accum_read(self._h, p))
        return out

    def accum_clear(self):
        self._chk(self._L.moptix_accum_clear(self._h))

    def accum_device_ptr(self):
        p = C.c_void_p()
        self._chk(self._L.moptix_accum_device_ptr(self._h, C.byref(p)))
        return p.value

    def accum_bind(self, dev_ptr):
        self._chk(self._L.moptix_accum_bind(self._h, C.c_void_p(dev_ptr)))

    def set_stream(self, hip_stream):
        self._chk(self._L.moptix_set_stream(self._h, C.c_void_p(hip_stream)))
        self._stream = int(hip_stream or 0)      # query_winding: a tensor call on this very stream needs no wait on either side

    def resolve_rgb8(self, n_accumulation, clear=False):
        out, p = self._frame(3, np.uint8)
        self._chk(self._L.moptix_resolve_rgb8(self._h, float(n_accumulation), 1 if clear else 0, p))
        return out

    def kernel_time(self, reset=False):
        ms, n = C.c_double(), C.c_uint64()
        self._chk(self._L.moptix_kernel_time(self._h, C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value

    def reduce_time(self):
        ms = C.c_double()
        self._chk(self._L.moptix_reduce_time(self._h, C.byref(ms)))
        return ms.value

    # ---- multi-GPU collectives on RCCL, behind the C ABI (include/moptix.h "Multi-GPU collectives") ----
    @staticmethod
    def comm_unique_id():
        """ncclGetUniqueId as 128 bytes: made by one rank, handed to the others by the host (bench.py: torch.distributed)."""
        buf = (C.c_uint8 * 128)()
        rc = K.device_lib().moptix_comm_unique_id(buf)
        if rc != K.MOPTIX_OK:
            raise MoptixError(rc, K.device_lib().moptix_last_error(None).decode())
        return bytes(buf)

    def comm_init(self, unique_id, rank, nranks):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._chk(self._L.moptix_comm_init(self._h, buf, int(rank), int(nranks)))

    def comm_destroy(self):
        self._chk(self._L.moptix_comm_destroy(self._h))

    def gather_tiles(self, dst=0):
        """Tile split: every rank's tiles into rank dst's accuBuffer (grouped ncclSend / ncclRecv + unpack on the device)."""
        self._chk(self._L.moptix_gather_tiles(self._h, int(dst)))

    def reduce_frame(self, dst=0):
        """Sample split: ncclReduce(sum) of the accuBuffers into rank dst's."""
        self._chk(self._L.moptix_reduce_frame(self._h, int(dst)))

    def packed_tile_floats(self, nranks):
        n = C.c_uint64()
        self._chk(self._L.moptix_packed_tile_floats(self._h, int(nranks), C.byref(n)))
        return int(n.value)

    def pack_tiles(self, rank, nranks, dst_device_ptr):
        self._chk(self._L.moptix_pack_tiles(self._h, int(rank), int(nranks), C.c_void_p(dst_device_ptr)))

    def unpack_tiles(self, rank, nranks, src_device_ptr):
        self._chk(self._L.moptix_unpack_tiles(self._h, int(rank), int(nranks), C.c_void_p(src_device_ptr)))

    # ---- first-hit AOVs (include/moptix.h "first-hit AOVs") ----
    AOV_NAMES = ("albedo", "normal", "depth", "hits", "primId", "matId")
    AOV_CHANNELS = dict(albedo=3, normal=3, depth=1, hits=1, primId=1, matId=1)

    def render_aovs(self, seeds):
        """Adds one first-hit sample per seed to every pixel's AOV sums (whole frame; blocking)."""
        s, p = self._seeds(seeds)
        self._chk(self._L.moptix_render_aovs(self._h, p, len(s)))

    def aov_clear(self):
        self._chk(self._L.moptix_aov_clear(self._h))

    def aov_samples(self):
        n = C.c_uint64()
        self._chk(self._L.moptix_aov_samples(self._h, C.byref(n)))
        return int(n.value)

    def aov_read(self):
        """{name: (H, W, k) array} in the accumulation buffer's row order (row 0 = bottom): albedo, normal (k = 3), depth, hits
        (float32, k = 1), primId, matId (int32, k = 1)."""
        out = {n: self._frame(self.AOV_CHANNELS[n], np.int32 if n in ("primId", "matId") else np.float32)[0] for n in self.AOV_NAMES}
        b = K.AovBuffers(*[out[n].ctypes.data for n in self.AOV_NAMES])
        self._chk(self._L.moptix_aov_read(self._h, C.byref(b)))
        return out

    def aov_bind(self, tensors):
        """tensors: {name: torch tensor on this context's device, contiguous, (H, W, k) of float32 (int32 for the ids)}; a missing
        name keeps the context's own buffer, None restores all of them.  Call aov_clear() before the first render into them."""
        if tensors is None:
            self._chk(self._L.moptix_aov_bind(self._h, None))
            return
        ptrs = []
        for n in self.AOV_NAMES:
            t = tensors.get(n)
            if t is None:
                ptrs.append(None)
                continue
            k = self.AOV_CHANNELS[n]
            _check_tensor("aov_bind", n, t, ("torch.int32" if n in ("primId", "matId") else "torch.float32",), self.height * self.width * k,
                          "%d x %d x %d elements" % (self.height, self.width, k), on_gpu=False)
            ptrs.append(t.data_ptr())
        b = K.AovBuffers(*ptrs)
        self._chk(self._L.moptix_aov_bind(self._h, C.byref(b)))

    def aov_means(self):
        """albedo / samples, normal / samples, depth / hits (inf where hits == 0), as (H, W, k) float32 arrays."""
        a = self.aov_read()
        n = np.float32(max(1, self.aov_samples()))
        hits = a["hits"]
        with np.errstate(divide="ignore", invalid="ignore"):
            depth = np.where(hits > 0, a["depth"] / np.where(hits > 0, hits, np.float32(1)), np.float32(np.inf)).astype(np.float32)
        return dict(albedo=(a["albedo"] / n).astype(np.float32), normal=(a["normal"] / n).astype(np.float32), depth=depth)

    # ---- denoiser (include/moptix.h "denoiser") ----
    def denoise_defaults(self):
        """moptix_denoise_defaults as a dict: iterations, normal_power, sigma_luminance, sigma_depth, demodulate."""
        p = K.DenoiseParams()
        self._chk(self._L.moptix_denoise_defaults(C.byref(p)))
        return dict(iterations=int(p.iterations), normal_power=int(p.normalPower), sigma_luminance=float(p.sigmaLuminance),
                    sigma_depth=float(p.sigmaDepth), demodulate=bool(p.demodulate))

    def denoise(self, n_accumulation, iterations=5, normal_power=128, sigma_luminance=4.0, sigma_depth=1.0, demodulate=False):
        """The accumulation buffer's mean (accum / n_accumulation) filtered under the guidance of the AOVs (render_aovs first);
        blocking.  Returns an (H, W, 3) float32 array in accum_read's row order (row 0 = bottom)."""
        p = K.DenoiseParams(int(iterations), int(normal_power), 1 if demodulate else 0, float(sigma_luminance), float(sigma_depth))
        self._chk(self._L.moptix_denoise(self._h, C.byref(p), float(n_accumulation)))
        out, op = self._frame()
        self._chk(self._L.moptix_denoise_read(self._h, op))
        return out

    def denoise_bind(self, tensor):
        """tensor: torch float32 tensor on this context's device, contiguous, H*W*3 elements, that later denoise calls write; None
        restores the context's own output buffer."""
        if tensor is None:
            self._chk(self._L.moptix_denoise_bind(self._h, None))
            return
        _check_tensor("denoise_bind", "the tensor", tensor, ("torch.float32",), self.height * self.width * 3,
                      "%d x %d x 3 elements" % (self.height, self.width), on_gpu=False)
        self._chk(self._L.moptix_denoise_bind(self._h, C.c_void_p(tensor.data_ptr())))

    # ---- temporal accumulation (include/moptix.h "denoiser: temporal accumulation") ----
    def temporal_defaults(self):
        """moptix_temporal_defaults as a dict: alpha, alpha_moments, depth_tolerance, normal_threshold, max_history, variance_frames."""
        p = K.TemporalParams()
        self._chk(self._L.moptix_temporal_defaults(C.byref(p)))
        return dict(alpha=float(p.alpha), alpha_moments=float(p.alphaMoments), depth_tolerance=float(p.depthTolerance),
                    normal_threshold=float(p.normalThreshold), max_history=int(p.maxHistory), variance_frames=int(p.varianceFrames))

    def denoise_temporal(self, n_accumulation, temporal=None, iterations=5, normal_power=128, sigma_luminance=4.0, sigma_depth=1.0,
                         demodulate=False):
        """denoise() with the temporal stage in front: last call's accumulation is reprojected through the AOVs (depth, normal, ids),
        the camera of set_params and the spheres as update_spheres left them (with set_option("temporal_face_motion", 1) also
        through the motion of the faces that update_faces moved since the last call), and blended with this frame.  temporal: a dict with
        some of temporal_defaults()'s keys (the rest keep their defaults).  Returns an (H, W, 3) float32 array as denoise()."""
        t = self.temporal_defaults()
        for k, v in (temporal or {}).items():
            if k not in t:
                raise ValueError("denoise_temporal: unknown temporal parameter %r" % k)
            t[k] = v
        tp = K.TemporalParams(float(t["alpha"]), float(t["alpha_moments"]), float(t["depth_tolerance"]), float(t["normal_threshold"]),
                              int(t["max_history"]), int(t["variance_frames"]))
        p = K.DenoiseParams(int(iterations), int(normal_power), 1 if demodulate else 0, float(sigma_luminance), float(sigma_depth))
        self._chk(self._L.moptix_denoise_temporal(self._h, C.byref(p), C.byref(tp), float(n_accumulation)))
        out, op = self._frame()
        self._chk(self._L.moptix_denoise_read(self._h, op))
        return out

    def temporal_reset(self):
        """Drops the history: the next denoise_temporal call is a first frame."""
        self._chk(self._L.moptix_temporal_reset(self._h))

    def temporal_info(self):
        """dict: frames since the last drop; of the last call geometry_pixels, history_pixels, disoccluded_pixels, mean_history."""
        s = K.TemporalStats()
        self._chk(self._L.moptix_temporal_info(self._h, C.byref(s)))
        return dict(frames=int(s.frames), geometry_pixels=int(s.geometryPixels), history_pixels=int(s.historyPixels),
                    disoccluded_pixels=int(s.disoccludedPixels), mean_history=float(s.meanHistory))

    def temporal_face_info(self):
        """dict of the last denoise_temporal call under set_option("temporal_face_motion", 1): tracked_faces (faces that had a
        snapshot to compare with), moved_faces, moved_pixels.  Zeros with the option off."""
        s = K.TemporalFaceStats()
        self._chk(self._L.moptix_temporal_face_info(self._h, C.byref(s)))
        return dict(tracked_faces=int(s.trackedFaces), moved_faces=int(s.movedFaces), moved_pixels=int(s.movedPixels))

    def temporal_read(self):
        """Of the last denoise_temporal call: dict(motion=(H, W, 2) float32 pixel motion vectors, history=(H, W) float32 lengths)."""
        motion, history = self._frame(2)[0], self._frame(0)[0]
        b = K.TemporalBuffers(motion.ctypes.data, history.ctypes.data)
        self._chk(self._L.moptix_temporal_read(self._h, C.byref(b)))
        return dict(motion=motion, history=history)

    # ---- adaptive sampling (include/moptix.h "adaptive sampling") ----
    @staticmethod
    def adaptive_defaults():
        """moptix_adaptive_defaults as a dict: threshold, min_samples, batch.  Pure host: works without a device."""
        p = K.AdaptiveParams()
        rc = K.device_lib().moptix_adaptive_defaults(C.byref(p))
        if rc != K.MOPTIX_OK:
            raise MoptixError(rc, K.device_lib().moptix_last_error(None).decode())
        return dict(threshold=float(p.threshold), min_samples=int(p.minSamples), batch=int(p.batch))

    def render_adaptive(self, seeds, threshold=None, min_samples=None, batch=None):
        """Renders `seeds` like render(), but after a first pass of min_samples seeds over the whole frame only the pixels whose
        relative standard error (3x3 maximum) is above `threshold` get the following passes of `batch` seeds each; blocking.  None
        keeps a parameter's default.  Returns the stats dict: passes, samples_traced, samples_uniform, active_pixels_last,
        converged_pixels, min_count, max_count."""
        d = self.adaptive_defaults()
        p = K.AdaptiveParams(float(d["threshold"] if threshold is None else threshold),
                             int(d["min_samples"] if min_samples is None else min_samples), int(d["batch"] if batch is None else batch))
        s, sp = self._seeds(seeds)
        st = K.AdaptiveStats()
        self._chk(self._L.moptix_render_adaptive(self._h, sp, len(s), C.byref(p), C.byref(st)))
        return st.as_dict()

    def adaptive_clear(self):
        """Zeroes the per-pixel counts, moments and converged flags AND the accumulation buffer."""
        self._chk(self._L.moptix_adaptive_clear(self._h))

    def adaptive_read(self):
        """dict(count=(H, W) uint32, moments=(H, W, 2) float32, error=(H, W) float32, converged=(H, W) uint8) in accum_read's row
        order (row 0 = bottom)."""
        out = dict(count=self._frame(0, np.uint32)[0], moments=self._frame(2)[0], error=self._frame(0)[0], converged=self._frame(0, np.uint8)[0])
        b = K.AdaptiveBuffers(*[out[n].ctypes.data for n in ("count", "moments", "error", "converged")])
        self._chk(self._L.moptix_adaptive_read(self._h, C.byref(b)))
        return out

    def adaptive_mean(self):
        """accum / count per pixel (0 where count is 0): an (H, W, 3) float32 array in accum_read's row order."""
        out, p = self._frame()
        self._chk(self._L.moptix_adaptive_mean(self._h, p))
        return out

    def adaptive_mean_into(self, tensor):
        """The same into a torch float32 tensor on this context's device, contiguous, H*W*3 elements."""
        _check_tensor("adaptive_mean_into", "the tensor", tensor, ("torch.float32",), self.height * self.width * 3,
                      "%d x %d x 3 elements" % (self.height, self.width))      # any GPU, as before: device is left None
        self._chk(self._L.moptix_adaptive_mean_device(self._h, C.c_void_p(tensor.data_ptr())))

    def adaptive_resolve_rgb8(self):
        """resolve_rgb8 with each pixel's own count as the divisor: (H, W, 3) uint8, row 0 = top."""
        out, p = self._frame(3, np.uint8)
        self._chk(self._L.moptix_adaptive_resolve_rgb8(self._h, p))
        return out

    # ---- ray queries (include/moptix.h "ray queries") ----
    QUERY_MODES = dict(closest=K.QUERY_CLOSEST, any=K.QUERY_ANY)

    def query_rays(self, rays, mode="closest"):
        """Closest hit ("closest") or occlusion ("any") of the caller's rays, n x 8 floats o, d, tmin, tmax; blocking.
        A numpy array takes the host path: "closest" returns a HIT_DTYPE record array (t, prim, mat, u, v, ng), "any" an int32 array.
        A contiguous (n, 8) float32 torch tensor on this context's device is read where it is, and the results are tensors on that device:
        "any" an int32 tensor; "closest" a dict of views t, prim, mat, u, v, ng into "records", the (n, 8) float32 tensor of the raw
        moptix_hit records."""
        if mode not in self.QUERY_MODES:
            raise ValueError("query_rays: mode %r (closest or any)" % (mode,))
        m = self.QUERY_MODES[mode]
        if isinstance(rays, np.ndarray) or not hasattr(rays, "data_ptr"):
            rays = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 8))
            out = np.zeros(len(rays), HIT_DTYPE if m == K.QUERY_CLOSEST else np.int32)
            self._chk(self._L.moptix_query_rays(self._h, rays.ctypes.data_as(C.POINTER(C.c_float)), len(rays), m, C.c_void_p(out.ctypes.data)))
            return out
        import torch
        _check_tensor("query_rays", "rays", rays, ("torch.float32",), _rows(8), "shape (n, 8)", self.device)
        n = rays.shape[0]
        if m == K.QUERY_ANY:
            out = torch.empty(n, dtype=torch.int32, device=rays.device)
        else:
            out = torch.empty((n, 8), dtype=torch.float32, device=rays.device)
        torch.cuda.current_stream(rays.device).synchronize()      # the rays are ready before the context's stream reads them
        self._chk(self._L.moptix_query_rays_device(self._h, C.c_void_p(rays.data_ptr()), n, m, C.c_void_p(out.data_ptr())))
        self.sync()
        if m == K.QUERY_ANY:
            return out
        return _record_views(out, "t", "ng")

    def query_rays_multi(self, rays, max_hits=4, count_all=False):
        """The first max_hits hits along each of the caller's rays, n x 8 floats o, d, tmin, tmax, in order of (t, prim); blocking.  Returns
        (hits, counts): per ray max_hits records, the hits first and miss records behind them, and how many are hits -- with count_all
        the number of all hits along the ray instead, however many were kept (the walk then cannot prune); max_hits 1..64, with
        count_all also 0: the pure crossing count.
        A numpy array takes the host path: hits is an (n, max_hits) HIT_DTYPE array, counts an int32 array.
        A contiguous (n, 8) float32 torch tensor on this context's device is read where it is, and the results are tensors on that device:
        hits the dict of views t, prim, mat, u, v, ng of query_rays into "records", here the (n, max_hits, 8) float32 tensor of the raw
        moptix_hit records, and counts an int32 tensor."""
        k = int(max_hits)
        flags = K.MULTI_COUNT_ALL if count_all else 0
        if k < (0 if count_all else 1) or k > K.MULTI_MAX_HITS:
            raise ValueError("query_rays_multi: max_hits %r (1..%d; 0 only with count_all)" % (max_hits, K.MULTI_MAX_HITS))
        if isinstance(rays, np.ndarray) or not hasattr(rays, "data_ptr"):
            rays = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 8))
            hits = np.zeros((len(rays), k), HIT_DTYPE)
            counts = np.zeros(len(rays), np.int32)
            self._chk(self._L.moptix_query_rays_multi(self._h, rays.ctypes.data_as(C.POINTER(C.c_float)), len(rays), k, flags,
                                                      C.c_void_p(hits.ctypes.data) if k else None, counts.ctypes.data_as(C.POINTER(C.c_int32))))
            return hits, counts
        import torch
        _check_tensor("query_rays_multi", "rays", rays, ("torch.float32",), _rows(8), "shape (n, 8)", self.device)
        n = rays.shape[0]
        out = torch.empty((n, k, 8), dtype=torch.float32, device=rays.device)
        counts = torch.empty(n, dtype=torch.int32, device=rays.device)
        torch.cuda.current_stream(rays.device).synchronize()      # the rays are ready before the context's stream reads them
        self._chk(self._L.moptix_query_rays_multi_device(self._h, C.c_void_p(rays.data_ptr()), n, k, flags,
                                                         C.c_void_p(out.data_ptr()) if k else None, C.c_void_p(counts.data_ptr())))
        self.sync()
        return _record_views(out, "t", "ng"), counts

    def query_radiance(self, rays, seeds=None, states=None, clamp=False, index_base=0):
        """Path-traced radiance along the caller's rays, n x 8 floats o, d, tmin, tmax with UNIT directions; blocking.  Returns (n, 4)
        float32 r, g, b, t: rgb the sum (not the mean) of the ray's samples in order, t the first hit's distance (tmax on a miss).
        seeds: a list of launch seeds, one sample each -- sample s of ray i starts from tea16(index_base + i, seeds[s]); or
        states: (n, nSamples) uint32 RNG states, taken as they are.  clamp: each sample clamped to [0, 1] as a frame's are.
        A numpy array takes the host path.  A contiguous (n, 8) float32 torch tensor on this context's device is read where it is (states
        then a contiguous uint32 or int32 tensor on that device) and the result is a tensor on that device."""
        if (seeds is None) == (states is None):
            raise ValueError("query_radiance: give either seeds or states")
        flags = K.RADIANCE_CLAMP if clamp else 0
        base = int(index_base) & 0xffffffff
        sd = None
        if seeds is not None:
            sd = np.ascontiguousarray((np.asarray(seeds).astype(np.int64).reshape(-1) & 0xffffffff).astype(np.uint32)).view(np.int32)
            if len(sd) < 1:
                raise ValueError("query_radiance: an empty seed list")
        sp = None if sd is None else sd.ctypes.data_as(C.POINTER(C.c_int32))
        if isinstance(rays, np.ndarray) or not hasattr(rays, "data_ptr"):
            rays = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 8))
            n = len(rays)
            st = None
            if states is not None:
                if hasattr(states, "data_ptr"):
                    raise ValueError("query_radiance: states follow the rays: a numpy array for numpy rays")
                st = np.asarray(states)
                if st.dtype not in (np.dtype(np.uint32), np.dtype(np.int32)) or st.ndim != 2 or st.shape[0] != n or st.shape[1] < 1:
                    raise ValueError("query_radiance: states must be (n, nSamples) uint32")
                st = np.ascontiguousarray(st).view(np.uint32)
            ns = len(sd) if sd is not None else st.shape[1]
            out = np.zeros((n, 4), np.float32)
            self._chk(self._L.moptix_query_radiance(self._h, rays.ctypes.data_as(C.POINTER(C.c_float)), n, sp,
                                                    None if st is None else st.ctypes.data_as(C.POINTER(C.c_uint32)), ns, base, flags,
                                                    out.ctypes.data_as(C.POINTER(C.c_float))))
            return out
        import torch
        _check_tensor("query_radiance", "rays", rays, ("torch.float32",), _rows(8), "shape (n, 8)", self.device)
        n = rays.shape[0]
        if states is not None:
            if not hasattr(states, "data_ptr"):
                raise ValueError("query_radiance: states follow the rays: a tensor on the rays' device")
            _check_tensor("query_radiance", "states", states, ("torch.uint32", "torch.int32"),
                          lambda t: t.dim() == 2 and t.shape[0] == n and t.shape[1] >= 1, "shape (n, nSamples)", self.device)
        ns = len(sd) if sd is not None else states.shape[1]
        out = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
        torch.cuda.current_stream(rays.device).synchronize()      # the rays are ready before the context's stream reads them
        self._chk(self._L.moptix_query_radiance_device(self._h, C.c_void_p(rays.data_ptr()), n, sp,
                                                       None if states is None else C.c_void_p(states.data_ptr()), ns, base, flags,
                                                       C.c_void_p(out.data_ptr())))
        self.sync()
        return out

    # ---- point queries (include/moptix.h "point queries") ----
    POINT_MODES = dict(closest=K.POINT_CLOSEST, any=K.POINT_ANY, signed=K.POINT_SIGNED)

    def query_points(self, points, mode="closest", max_dist=np.inf):
        """The nearest surface point ("closest"), the same with dist negative inside a closed mesh or a sphere ("signed": sign_info() says
        whether the mesh is closed), or "is anything within max_dist" ("any") for the caller's points; blocking.
        A numpy array takes the host path: (n, 3) positions with max_dist a scalar or an (n,) array, or (n, 4) rows x y z maxDist
        (max_dist is then not consulted).  "closest" and "signed" return a POINT_DTYPE record array (dist, prim, mat, u, v, p), "any" an int32 array.
        A contiguous (n, 4) float32 torch tensor on this context's device is read where it is, and the results are tensors on that device:
        "any" an int32 tensor; "closest" and "signed" a dict of views dist, prim, mat, u, v, p into "records", the (n, 8) float32 tensor of the raw
        moptix_point_hit records."""
        if mode not in self.POINT_MODES:
            raise ValueError("query_points: mode %r (closest, signed or any)" % (mode,))
        m = self.POINT_MODES[mode]
        if isinstance(points, np.ndarray) or not hasattr(points, "data_ptr"):
            pts = _point_rows("query_points", points, max_dist)
            out = np.zeros(len(pts), np.int32 if m == K.POINT_ANY else POINT_DTYPE)
            pp = pts.ctypes.data_as(C.POINTER(C.c_float))
            if m == K.POINT_SIGNED:
                self._chk(self._L.moptix_query_points_signed(self._h, pp, len(pts), C.c_void_p(out.ctypes.data)))
            else:
                self._chk(self._L.moptix_query_points(self._h, pp, len(pts), m, C.c_void_p(out.ctypes.data)))
            return out
        import torch
        _check_tensor("query_points", "points", points, ("torch.float32",), _rows(4), "shape (n, 4), x y z maxDist", self.device)
        n = points.shape[0]
        if m == K.POINT_ANY:
            out = torch.empty(n, dtype=torch.int32, device=points.device)
        else:
            out = torch.empty((n, 8), dtype=torch.float32, device=points.device)
        torch.cuda.current_stream(points.device).synchronize()      # the points are ready before the context's stream reads them
        self._chk(self._L.moptix_query_points_device(self._h, C.c_void_p(points.data_ptr()), n, m, C.c_void_p(out.data_ptr())))
        self.sync()
        if m == K.POINT_ANY:
            return out
        return _record_views(out, "dist", "p")

    def query_points_multi(self, points, max_near=4, count_all=False, max_dist=np.inf):
        """The max_near nearest primitives to each of the caller's points, in order of (distance, prim); blocking.  Returns (hits, counts):
        per point max_near records, the nearest first and miss records behind them, and how many are primitives -- with count_all the
        number of all primitives within max_dist instead, however many were kept (the walk then prunes at max_dist alone); max_near
        1..64, with count_all also 0: the pure in-range count.
        A numpy array takes the host path: (n, 3) positions with max_dist a scalar or an (n,) array, or (n, 4) rows x y z maxDist (max_dist
        is then not consulted); hits is an (n, max_near) POINT_DTYPE array, counts an int32 array.
        A contiguous (n, 4) float32 torch tensor on this context's device is read where it is, and the results are tensors on that device:
        hits the dict of views dist, prim, mat, u, v, p of query_points into "records", here the (n, max_near, 8) float32 tensor of the raw
        moptix_point_hit records, and counts an int32 tensor."""
        k = int(max_near)
        flags = K.POINT_MULTI_COUNT_ALL if count_all else 0
        if k < (0 if count_all else 1) or k > K.POINT_MULTI_MAX_NEAR:
            raise ValueError("query_points_multi: max_near %r (1..%d; 0 only with count_all)" % (max_near, K.POINT_MULTI_MAX_NEAR))
        if isinstance(points, np.ndarray) or not hasattr(points, "data_ptr"):
            pts = _point_rows("query_points_multi", points, max_dist)
            hits = np.zeros((len(pts), k), POINT_DTYPE)
            counts = np.zeros(len(pts), np.int32)
            self._chk(self._L.moptix_query_points_multi(self._h, pts.ctypes.data_as(C.POINTER(C.c_float)), len(pts), k, flags,
                                                        C.c_void_p(hits.ctypes.data) if k else None, counts.ctypes.data_as(C.POINTER(C.c_int32))))
            return hits, counts
        import torch
        _check_tensor("query_points_multi", "points", points, ("torch.float32",), _rows(4), "shape (n, 4), x y z maxDist", self.device)
        n = points.shape[0]
        out = torch.empty((n, k, 8), dtype=torch.float32, device=points.device)
        counts = torch.empty(n, dtype=torch.int32, device=points.device)
        torch.cuda.current_stream(points.device).synchronize()      # the points are ready before the context's stream reads them
        self._chk(self._L.moptix_query_points_multi_device(self._h, C.c_void_p(points.data_ptr()), n, k, flags,
                                                           C.c_void_p(out.data_ptr()) if k else None, C.c_void_p(counts.data_ptr())))
        self.sync()
        return _record_views(out, "dist", "p"), counts

    # ---- box queries (include/moptix.h "box queries") ----
    BOX_MODES = dict(any=K.BOX_ANY, count=K.BOX_COUNT)

    def query_boxes(self, boxes, mode="any", max_prims=None):
        """The primitives that meet each of the caller's axis-aligned boxes lox loy loz hix hiy hiz (closed sets: touching counts);
        blocking.  "any": int32, 1 where anything meets the box; "count": int32, how many primitives do; "list": which.
        "list" with max_prims=None is two passes -- count, an int64 cumulative sum, fill -- and returns (prims, offsets), a CSR pair: the
        ids of box i, ascending, are prims[offsets[i]:offsets[i + 1]].  "list" with max_prims=K is one pass with K slots per box and
        returns (prims (n, K), counts): where counts[i] <= K the row holds the ids ascending and -1 behind them, else -1 throughout.
        A numpy (n, 6) or (n, 2, 3) array takes the host path and the results are numpy arrays.  A contiguous (n, 6) float32 torch tensor
        on this context's device is read where it is, and the results are tensors on that device."""
        return self._query_box_family("query_boxes", "moptix_query_boxes", boxes, 6, (2, 3), "lox loy loz hix hiy hiz", mode, max_prims)

    def query_obbs(self, obbs, mode="any", max_prims=None):
        """The primitives that meet each of the caller's oriented boxes (closed sets: touching counts); blocking.  A box is the sixteen
        floats of oriented_boxes: centre, half-extents along the box's own axes, the three axes as world-space directions, one float that
        is not read.  A box whose axes are further than 2^-10 from orthonormal, with a negative half-extent or a non-finite float meets
        nothing.  Modes and return values are query_boxes': "any" and "count" give int32 per box; "list" gives the CSR pair (prims,
        offsets), or with max_prims=K (prims (n, K), counts).
        A numpy (n, 16) array takes the host path and the results are numpy arrays.  A contiguous (n, 16) float32 torch tensor on this
        context's device is read where it is, and the results are tensors on that device."""
        return self._query_box_family("query_obbs", "moptix_query_obbs", obbs, 16, None, "centre, half-extents, three axes, one unused", mode, max_prims)

    def query_frusta(self, frusta, mode="any", max_prims=None):
        """The primitives that meet each of the caller's six-plane regions (closed sets: touching counts); blocking.  A query is 24 floats,
        six planes nx ny nz d with the normals pointing inwards: the region is { x : dot(n_j, x) + d_j >= 0 for all six }.  Normals need
        not be unit length; a plane 0 0 0 d with d >= 0 constrains nothing, so fewer planes (a wedge, a slab, a half-space) are padded
        with zeros; a query with a non-finite float meets nothing.  frustum_planes makes the rows from a clip matrix, camera_frusta from
        the renderer's camera and screen rectangles.  Triangles and quads are tested exactly up to rounding; a sphere by the plane rule
        on its ball (conservative at the region's edges and corners).  Modes and return values are query_boxes': "any" and "count" give
        int32 per query; "list" gives the CSR pair (prims, offsets), or with max_prims=K (prims (n, K), counts).
        A numpy (n, 24) or (n, 6, 4) array takes the host path and the results are numpy arrays.  A contiguous (n, 24) float32 torch
        tensor on this context's device is read where it is, and the results are tensors on that device."""
        return self._query_box_family("query_frusta", "moptix_query_frusta", frusta, 24, (6, 4), "six planes nx ny nz d", mode, max_prims)

    def query_tris(self, tris, mode="any", max_prims=None):
        """The primitives that meet each of the caller's triangles (closed sets: touching counts); blocking.  A query is nine floats, the
        three vertices ax ay az bx by bz cx cy cz -- a row of vertices[faces].  A zero-area query (a segment, a point) is valid; a query
        with a non-finite float meets nothing.  Triangles and quads are tested exactly up to rounding wherever one of the two triangles
        has non-zero area (two zero-area triangles: a superset); a sphere by its surface.  Modes and return values are query_boxes':
        "any" and "count" give int32 per query; "list" gives the CSR pair (prims, offsets), or with max_prims=K (prims (n, K), counts).
        A numpy (n, 9) or (n, 3, 3) array takes the host path and the results are numpy arrays.  A contiguous (n, 9) or (n, 3, 3) float32
        torch tensor on this context's device is read where it is, and the results are tensors on that device."""
        if hasattr(tris, "data_ptr") and tris.dim() == 3 and tuple(tris.shape[1:]) == (3, 3) and tris.is_contiguous():
            tris = tris.view(-1, 9)                                  # the same memory, read in place
        return self._query_box_family("query_tris", "moptix_query_tris", tris, 9, (3, 3), "ax ay az bx by bz cx cy cz", mode, max_prims)

    def _first_face_id(self, n_faces):
        """The primitive id of face 0, nSpheres + nQuads: what a box holding every scene within 1e30 units counts, less the triangles."""
        n_tris = int(self.accel_info().nTriangles)
        if n_faces != n_tris:
            raise ValueError("self_intersections: %d faces, but the tree was built on %d" % (n_faces, n_tris))
        everything = np.array([[-1e30, -1e30, -1e30, 1e30, 1e30, 1e30]], np.float32)
        return int(self.query_boxes(everything, "count")[0]) - n_tris

    def self_intersections(self, vertices, faces, max_prims=None):
        """The pairs of faces of the uploaded mesh that meet without sharing a vertex: vertices (V, 3) float32 and faces (F, 3) integer
        are the mesh as uploaded (and as last updated), whose face f is primitive nSpheres + nQuads + f; blocking.  Runs the list form of
        query_tris on vertices[faces] and returns the sorted unique pairs (i, j), i < j, of face ids as a (P, 2) int64 array -- numpy for
        numpy input, a tensor on the device for tensors on this context's device.  A pair is reported if either direction reports it:
        the uploaded record's second and third vertex are two roundings away from the caller's, so one direction alone may not be
        symmetric in the last bit.  Pairs with a common vertex index touch by construction and are left out, a face against itself too.
        max_prims=K: one pass with K slots per face instead of two passes; ValueError if a face meets more than K primitives."""
        on_device = hasattr(vertices, "data_ptr")
        if on_device:
            import torch
            if not hasattr(faces, "data_ptr"):
                faces = torch.as_tensor(np.asarray(faces), device=vertices.device)
            if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or vertices.dtype != torch.float32:
                raise ValueError("self_intersections: vertices must be (V, 3) float32 and faces (F, 3) integer")
            f = faces.to(torch.int64)
            tris = vertices[f].contiguous()
        else:
            v, f = np.asarray(vertices, np.float32), np.asarray(faces)
            if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
                raise ValueError("self_intersections: vertices must be (V, 3) float32 and faces (F, 3) integer")
            f = f.astype(np.int64)
            tris = np.ascontiguousarray(v[f])
        n = int(f.shape[0])
        if n == 0:
            return torch.zeros((0, 2), dtype=torch.int64, device=vertices.device) if on_device else np.zeros((0, 2), np.int64)
        base = self._first_face_id(n)
        if max_prims is None:
            prims, offsets = self.query_tris(tris, "list")
            counts = offsets[1:] - offsets[:-1]
        else:
            rows, counts = self.query_tris(tris, "list", max_prims=max_prims)
            if int(counts.max()) > int(max_prims):
                raise ValueError("self_intersections: a face meets %d primitives, more than max_prims = %d" % (int(counts.max()), int(max_prims)))
            prims = rows[rows >= 0]                                  # row-major: face by face, ascending within a face
        if on_device:
            i = torch.repeat_interleave(torch.arange(n, device=f.device), counts.to(torch.int64))
            j = prims.to(torch.int64) - base
            keep = j >= 0
            i, j = i[keep], j[keep]
            keep = ~(f[i][:, :, None] == f[j][:, None, :]).any(dim=2).any(dim=1)
            i, j = i[keep], j[keep]
            pairs = torch.stack([torch.minimum(i, j), torch.maximum(i, j)], dim=1)
            return torch.unique(pairs, dim=0) if len(pairs) else pairs
        i = np.repeat(np.arange(n, dtype=np.int64), np.asarray(counts, np.int64))
        j = prims.astype(np.int64) - base
        keep = j >= 0
        i, j = i[keep], j[keep]
        keep = ~(f[i][:, :, None] == f[j][:, None, :]).any(axis=(1, 2))
        i, j = i[keep], j[keep]
        pairs = np.stack([np.minimum(i, j), np.maximum(i, j)], axis=1)
        return np.unique(pairs, axis=0) if len(pairs) else pairs.reshape(0, 2)

    def _query_box_family(self, who, entry, boxes, width, folded, layout, mode, max_prims):
        """query_boxes, query_obbs, query_frusta and query_tris: `entry`, `entry`_device, `entry`_list and `entry`_list_device on (n, width) float32 rows; a numpy
        array may also have the shape (n,) + folded."""
        fn = lambda suffix: getattr(self._L, entry + suffix)      # looked up after the arguments are checked
        if mode not in self.BOX_MODES and mode != "list":
            raise ValueError("%s: mode %r (any, count or list)" % (who, mode))
        if max_prims is not None and (mode != "list" or int(max_prims) < 0):
            raise ValueError("%s: max_prims %r (a capacity >= 0, with mode \"list\" only)" % (who, max_prims))
        if isinstance(boxes, np.ndarray) or not hasattr(boxes, "data_ptr"):
            b = np.asarray(boxes, np.float32)
            if not ((b.ndim == 2 and b.shape[1] == width) or (folded is not None and b.ndim == 3 and b.shape[1:] == folded)):
                raise ValueError("%s: boxes must be (n, %d)%s, not %r" % (who, width, " or (n, %d, %d)" % folded if folded else "", b.shape))
            b = np.ascontiguousarray(b.reshape(-1, width), np.float32)
            n = len(b)
            bp, i32p = b.ctypes.data_as(C.POINTER(C.c_float)), lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
            counts = np.zeros(n, np.int32)
            if mode != "list" or max_prims is None:
                self._chk(fn("")(self._h, bp, n, self.BOX_MODES.get(mode, K.BOX_COUNT), i32p(counts)))
                if mode != "list":
                    return counts
                offsets = np.zeros(n + 1, np.int64)
                np.cumsum(counts, dtype=np.int64, out=offsets[1:])
            else:
                offsets = np.arange(n + 1, dtype=np.int64) * int(max_prims)
            prims = np.zeros(int(offsets[-1]), np.int32)
            self._chk(fn("_list")(self._h, bp, n, offsets.ctypes.data_as(C.POINTER(C.c_int64)), i32p(prims), i32p(counts)))
            return (prims, offsets) if max_prims is None else (prims.reshape(n, int(max_prims)), counts)
        import torch
        _check_tensor(who, "boxes", boxes, ("torch.float32",), _rows(width), "shape (n, %d), %s" % (width, layout), self.device)
        n = boxes.shape[0]
        dev = boxes.device
        ptr = lambda t: C.c_void_p(t.data_ptr())
        counts = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()      # the boxes are ready before the context's stream reads them
        if mode != "list" or max_prims is None:
            self._chk(fn("_device")(self._h, ptr(boxes), n, self.BOX_MODES.get(mode, K.BOX_COUNT), ptr(counts)))
            self.sync()
            if mode != "list":
                return counts
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
        else:
            offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * int(max_prims)
        total = int(offsets[-1]) if n else 0
        room = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)      # an empty list still needs an address: an empty view has none
        prims = room[:total]
        torch.cuda.current_stream(dev).synchronize()      # offsets and the zeroed outputs too
        self._chk(fn("_list_device")(self._h, ptr(boxes), n, ptr(offsets), ptr(room) if n else None, ptr(counts)))
        self.sync()
        return (prims, offsets) if max_prims is None else (prims.reshape(n, int(max_prims)), counts)

    def occupancy(self, lo, hi, dims):
        """The (nx, ny, nz) bool grid of query_boxes "any" over occupancy_boxes(lo, hi, dims): which cells of the regular grid between
        the corners lo and hi anything of the scene meets; blocking, host path."""
        nx, ny, nz = (int(d) for d in dims)
        return self.query_boxes(occupancy_boxes(lo, hi, (nx, ny, nz)), "any").reshape(nx, ny, nz) != 0

    # ---- sweep queries (include/moptix.h "sweep queries") ----
    SWEEP_MODES = dict(closest=K.SWEEP_CLOSEST, any=K.SWEEP_ANY)

    def query_sweeps(self, sweeps, mode="closest"):
        """The first contact of a sphere of radius `radius` whose centre moves from o along d, c(t) = o + d * t for t in [0, tmax]
        ("closest"), or "does it touch anything on the way" ("any"), for the caller's sweeps ox oy oz dx dy dz radius tmax; blocking.
        A numpy (n, 8) array takes the host path: "closest" returns a SWEEP_DTYPE record array (t, prim, mat, u, v, p: the time of
        contact and the contact point; the contact normal is (o + d * t - p) / radius; a miss has prim -1 and t = tmax), "any" an int32
        array.  A contiguous (n, 8) float32 torch tensor on this context's device is read where it is, and the results are tensors on
        that device: "any" an int32 tensor; "closest" a dict of views t, prim, mat, u, v, p into "records", the (n, 8) float32 tensor of
        the raw moptix_sweep_hit records."""
        if mode not in self.SWEEP_MODES:
            raise ValueError("query_sweeps: mode %r (closest or any)" % (mode,))
        m = self.SWEEP_MODES[mode]
        if isinstance(sweeps, np.ndarray) or not hasattr(sweeps, "data_ptr"):
            s = np.asarray(sweeps, np.float32)
            if s.ndim != 2 or s.shape[1] != 8:
                raise ValueError("query_sweeps: sweeps must be (n, 8), not %r" % (s.shape,))
            s = np.ascontiguousarray(s)
            out = np.zeros(len(s), np.int32 if m == K.SWEEP_ANY else SWEEP_DTYPE)
            self._chk(self._L.moptix_query_sweeps(self._h, s.ctypes.data_as(C.POINTER(C.c_float)), len(s), m, C.c_void_p(out.ctypes.data)))
            return out
        import torch
        _check_tensor("query_sweeps", "sweeps", sweeps, ("torch.float32",), _rows(8), "shape (n, 8), ox oy oz dx dy dz radius tmax", self.device)
        n = sweeps.shape[0]
        if m == K.SWEEP_ANY:
            out = torch.empty(n, dtype=torch.int32, device=sweeps.device)
        else:
            out = torch.empty((n, 8), dtype=torch.float32, device=sweeps.device)
        torch.cuda.current_stream(sweeps.device).synchronize()      # the sweeps are ready before the context's stream reads them
        self._chk(self._L.moptix_query_sweeps_device(self._h, C.c_void_p(sweeps.data_ptr()), n, m, C.c_void_p(out.data_ptr())))
        self.sync()
        if m == K.SWEEP_ANY:
            return out
        return _record_views(out, "t", "p")

    # ---- segment queries (include/moptix.h "segment queries") ----
    SEGMENT_MODES = dict(closest=K.SEGMENT_CLOSEST, any=K.SEGMENT_ANY)

    def query_segments(self, segments, mode="closest", max_dist=None):
        """The nearest surface point to each of the caller's segments ("closest"), or "is anything within maxDist of it" ("any");
        blocking.  segments: (n, 8) rows ax ay az bx by bz maxDist pad (max_dist is then not consulted), or the end points alone as
        (n, 2, 3) or (n, 6) together with max_dist, a scalar or one value per segment (+inf = no limit).
        A numpy array takes the host path: "closest" returns a SEGMENT_DTYPE record array (dist; prim, mat; s, the parameter of the
        nearest point a + (b - a) * s on the segment; p, the nearest point on the primitive; feature, what was nearest: 0 end a, 1 end b,
        2-4 an edge of the triangle, 5 the segment crosses the primitive; a miss has prim -1 and dist = maxDist), "any" an int32 array.
        A float32 torch tensor on this context's device -- a contiguous (n, 8) one is read where it is -- gives tensors on that device:
        "any" an int32 tensor; "closest" a dict of views dist, prim, mat, s, p, feature into "records", the (n, 8) float32 tensor of the
        raw moptix_segment_hit records."""
        if mode not in self.SEGMENT_MODES:
            raise ValueError("query_segments: mode %r (closest or any)" % (mode,))
        m = self.SEGMENT_MODES[mode]
        if isinstance(segments, np.ndarray) or not hasattr(segments, "data_ptr"):
            s = np.asarray(segments, np.float32)
            if s.ndim == 3 and s.shape[1:] == (2, 3):
                s = s.reshape(-1, 6)
            if s.ndim != 2 or s.shape[1] not in (6, 8):
                raise ValueError("query_segments: segments must be (n, 8), or (n, 2, 3) / (n, 6) with max_dist, not %r" % (s.shape,))
            if s.shape[1] == 6:
                if max_dist is None:
                    raise ValueError("query_segments: end points alone need max_dist")
                md = np.asarray(max_dist, np.float32)
                if md.ndim > 1 or (md.ndim == 1 and len(md) != len(s)):
                    raise ValueError("query_segments: max_dist must be a scalar or one value per segment")
                s = np.concatenate([s, np.broadcast_to(md.reshape(-1, 1) if md.ndim else md, (len(s), 1)), np.zeros((len(s), 1), np.float32)], axis=1)
            s = np.ascontiguousarray(s, np.float32)
            out = np.zeros(len(s), np.int32 if m == K.SEGMENT_ANY else SEGMENT_DTYPE)
            self._chk(self._L.moptix_query_segments(self._h, s.ctypes.data_as(C.POINTER(C.c_float)), len(s), m, C.c_void_p(out.ctypes.data)))
            return out
        import torch
        if segments.dim() == 3 and tuple(segments.shape[1:]) == (2, 3):
            segments = segments.reshape(-1, 6)
        if segments.dim() == 2 and segments.shape[1] == 6:
            if max_dist is None:
                raise ValueError("query_segments: end points alone need max_dist")
            md = torch.as_tensor(max_dist, dtype=torch.float32, device=segments.device)
            if md.dim() > 1 or (md.dim() == 1 and md.shape[0] != segments.shape[0]):
                raise ValueError("query_segments: max_dist must be a scalar or one value per segment")
            n = segments.shape[0]
            segments = torch.cat([segments, md.reshape(-1, 1).expand(n, 1), torch.zeros((n, 1), dtype=segments.dtype, device=segments.device)], dim=1).contiguous()
        _check_tensor("query_segments", "segments", segments, ("torch.float32",), _rows(8), "shape (n, 8), ax ay az bx by bz maxDist pad, or (n, 2, 3) / (n, 6) with max_dist", self.device)
        n = segments.shape[0]
        if m == K.SEGMENT_ANY:
            out = torch.empty(n, dtype=torch.int32, device=segments.device)
        else:
            out = torch.empty((n, 8), dtype=torch.float32, device=segments.device)
        torch.cuda.current_stream(segments.device).synchronize()      # the segments are ready before the context's stream reads them
        self._chk(self._L.moptix_query_segments_device(self._h, C.c_void_p(segments.data_ptr()), n, m, C.c_void_p(out.data_ptr())))
        self.sync()
        if m == K.SEGMENT_ANY:
            return out
        ints = out.view(torch.int32)
        return {"records": out, "dist": out[:, 0], "prim": ints[:, 1], "mat": ints[:, 2], "s": out[:, 3], "p": out[:, 4:7], "feature": ints[:, 7]}

    def edge_proximity(self, vertices, edges, max_dist):
        """The nearest surface point to every edge of a mesh: vertices (V, 3) float32 and edges (E, 2) integer, max_dist a scalar or one
        value per edge; the closest records of query_segments on the segments vertices[edges] -- numpy for numpy input, the dict of
        tensors for tensors on this context's device.  The edge-edge half of a proximity narrow phase beside query_points, the
        vertex-face half.  An edge of the uploaded mesh itself is at distance 0 from the faces it belongs to."""
        if hasattr(vertices, "data_ptr"):
            import torch
            if not hasattr(edges, "data_ptr"):
                edges = torch.as_tensor(np.asarray(edges), device=vertices.device)
            if vertices.dim() != 2 or vertices.shape[1] != 3 or edges.dim() != 2 or edges.shape[1] != 2 or vertices.dtype != torch.float32:
                raise ValueError("edge_proximity: vertices must be (V, 3) float32 and edges (E, 2) integer")
            return self.query_segments(vertices[edges.to(torch.int64)].contiguous(), "closest", max_dist)
        v, e = np.asarray(vertices, np.float32), np.asarray(edges)
        if v.ndim != 2 or v.shape[1] != 3 or e.ndim != 2 or e.shape[1] != 2 or e.dtype.kind not in "iu":
            raise ValueError("edge_proximity: vertices must be (V, 3) float32 and edges (E, 2) integer")
        return self.query_segments(v[e.astype(np.int64)], "closest", max_dist)

    # ---- winding-number queries (include/moptix.h "winding-number queries") ----
    def query_winding(self, points, beta=2.0):
        """The generalised winding number of the caller's points: 1 inside and 0 outside a closed mesh wound outwards, and a smooth
        function across holes, flipped and duplicated faces (inside() thresholds it at 0.5).  beta is +inf (exact: every
        primitive's solid angle is summed) or >= 1: a cluster of the tree further away than beta times its radius is replaced by its
        dipole.  For a finite beta the value depends on the tree (leaf size, builder), not on the node format.
        A numpy array takes the host path: (n, 3) positions with beta a scalar or an (n,) array, or (n, 4) rows x y z beta (beta is then
        not consulted); the result is a float32 array.  A float32 torch tensor on this context's device, (n, 3) with beta a scalar or an
        (n,) tensor, or a contiguous (n, 4) one that is read where it is, gives a float32 tensor on that device -- asynchronously, with
        no wait on the host, when torch's current stream is the stream this context was given (set_stream): the call is then ordered
        like any torch operation.  On any other stream the call waits for the points before and for the result after, as query_points
        does.  A row with a non-finite coordinate or a beta below 1 gives NaN.  The numpy path is blocking."""
        if isinstance(points, np.ndarray) or not hasattr(points, "data_ptr"):
            pts = _point_rows("query_winding", points, beta)
            out = np.zeros(len(pts), np.float32)
            self._chk(self._L.moptix_query_winding(self._h, pts.ctypes.data_as(C.POINTER(C.c_float)), len(pts), out.ctypes.data_as(C.POINTER(C.c_float))))
            return out
        import torch
        if points.dim() == 2 and points.shape[1] == 3:
            b = torch.as_tensor(beta, dtype=torch.float32, device=points.device)
            if b.dim() > 1 or (b.dim() == 1 and b.shape[0] != points.shape[0]):
                raise ValueError("query_winding: beta must be a scalar or one value per point")
            points = torch.cat([points, b.reshape(-1, 1).expand(points.shape[0], 1)], dim=1).contiguous()
        _check_tensor("query_winding", "points", points, ("torch.float32",), _rows(4), "shape (n, 3), or (n, 4) rows x y z beta", self.device)
        n = points.shape[0]
        out = torch.empty(n, dtype=torch.float32, device=points.device)
        cur = torch.cuda.current_stream(points.device)
        same = getattr(self, "_stream", 0) != 0 and self._stream == cur.cuda_stream
        if not same:
            cur.synchronize()                                       # the points are ready before the context's stream reads them
        self._chk(self._L.moptix_query_winding_device(self._h, C.c_void_p(points.data_ptr()), n, C.c_void_p(out.data_ptr())))
        if not same:
            self.sync()
        return out

    def inside(self, points, beta=2.0):
        """query_winding(points, beta) > 0.5, on the same side: a bool numpy array for numpy input, a bool tensor for a tensor."""
        return self.query_winding(points, beta) > 0.5

    def winding_info(self):
        """dict of the winding queries' table of cluster moments: tableBuilds (moments passes this context has enqueued), nodes (of the
        built tree), tableBytes (as allocated; 0 before the first winding query on a tree), stale (1: the next query runs the pass)."""
        r = K.WindingInfo()
        self._chk(self._L.moptix_get_winding_info(self._h, C.byref(r)))
        return r.as_dict()

    def winding_table_read(self):
        """A test aid: the device's table of cluster moments, (nNodes, 4, 8) float32 -- per child slot A, p.xyz, N.xyz, r."""
        n = self.winding_info()["nodes"]
        out = np.zeros((max(1, n), 4, 8), np.float32)
        self._chk(self._L.moptix_debug_read_winding_table(self._h, C.c_void_p(out.ctypes.data)))
        return out[:n]

    def sign_info(self):
        """dict of what the signed mode rests on: weldedVerts, edges, boundaryEdges, nonManifoldEdges, flippedEdges, degenerateFaces, closed
        (1: the faces form a closed, consistently wound surface), signedVolume (negative: wound inwards, every sign flipped), tableBuilds.
        Works from the moment faces are uploaded."""
        r = K.SignInfo()
        self._chk(self._L.moptix_get_sign_info(self._h, C.byref(r)))
        return r.as_dict()

    def sign_table_read(self):
        """A test aid: the device's table of pseudonormals, (nFaces, 24) float32 -- v0 v1 v2 e01 e02 e12, the unit face normal, padding."""
        out = np.zeros((max(1, self.accel_info().nTriangles), 24), np.float32)
        self._chk(self._L.moptix_debug_read_sign_table(self._h, C.c_void_p(out.ctypes.data)))
        return out[:self.accel_info().nTriangles]

    # ---- mesh updates and refit (include/moptix.h "mesh updates and refit") ----
    def update_faces(self, first, positions, normals=None):
        """New positions (and normals) of the faces first .. first + n, numbered in upload order: (n, 3, 3) or (n, 9) float32, p0 p1 p2
        per face (from indexed data: verts[faces]).  A numpy array goes through the host entry.  A contiguous float32 torch tensor on this
        context's device is read where it is (moptix_update_faces_device).  On a built scene, refit_accel() or build_accel() must follow
        before anything traces."""
        if isinstance(positions, np.ndarray) or not hasattr(positions, "data_ptr"):
            pos = np.ascontiguousarray(np.asarray(positions, np.float32).reshape(-1, 9))
            nrm = None if normals is None else np.ascontiguousarray(np.asarray(normals, np.float32).reshape(-1, 9))
            if nrm is not None and len(nrm) != len(pos):
                raise ValueError("update_faces: %d faces of positions, %d of normals" % (len(pos), len(nrm)))
            fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
            self._chk(self._L.moptix_update_faces(self._h, int(first), len(pos), fp(pos), None if nrm is None else fp(nrm)))
            return
        import torch
        for name, t in (("positions", positions), ("normals", normals)):
            if t is None:
                continue
            _check_tensor("update_faces", name, t, ("torch.float32",), lambda t: t.numel() % 9 == 0 and t.numel() == positions.numel(),
                          "9 floats per face, as many faces as the positions", self.device)
        n = positions.numel() // 9
        torch.cuda.current_stream(positions.device).synchronize()      # the values are ready before the context's stream copies them
        self._chk(self._L.moptix_update_faces_device(self._h, int(first), n, C.c_void_p(positions.data_ptr() if n else None),
                                                     C.c_void_p(normals.data_ptr()) if normals is not None and n else None))
        self.sync()                                                    # the caller may free or overwrite the tensors now

    def refit_accel(self):
        """Fits the built tree to the updated faces in place (topology kept); blocking.  Returns refit_info()."""
        self._chk(self._L.moptix_refit_accel(self._h))
        return self.refit_info()

    def refit_info(self):
        """dict of the last refit on this tree: refitMs, sahCost, sahCostBuilt (their ratio is the quality signal), has64."""
        r = K.RefitInfo()
        self._chk(self._L.moptix_get_refit_info(self._h, C.byref(r)))
        return r.as_dict()

    def debug_buffer_addresses(self):
        """A test aid: dict(query_overflow=address, refit_plan=(7 addresses)) of buffers that a refit and a query on a refitted tree keep."""
        a = (C.c_uint64 * 8)()
        self._chk(self._L.moptix_debug_buffer_addresses(self._h, a))
        return dict(query_overflow=int(a[0]), refit_plan=tuple(int(x) for x in a[1:]))

    def debug_read_accel(self):
        a = self.accel_info()
        nodes = np.zeros((max(1, a.nNodes), 32), np.uint32)     # Node128 = 32 words
        tris = np.zeros((max(1, a.nTriangles), 12), np.uint32)
        prim = np.zeros(max(1, a.nTriangles), np.int32)
        self._chk(self._L.moptix_debug_read_accel(self._h, nodes.ctypes.data, tris.ctypes.data,
                                                  prim.ctypes.data_as(C.POINTER(C.c_int32))))
        return nodes[:a.nNodes], tris[:a.nTriangles], prim[:a.nTriangles]

    def debug_read_nodes64(self):
        """The nodes as the trace kernels fetch them: [nNodes, 16] words (Node64: corner xyz, step xyz, 6 plane words, 4 refs)."""
        a = self.accel_info()
        nodes = np.zeros((max(1, a.nNodes), 16), np.uint32)
        self._chk(self._L.moptix_debug_read_nodes64(self._h, nodes.ctypes.data))
        return nodes[:a.nNodes]

    def debug_trace(self, rays):
        rays = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 8))
        n = len(rays)
        t = np.zeros(n, np.float32); prim = np.zeros(n, np.int32)
        self._chk(self._L.moptix_debug_trace(self._h, rays.ctypes.data_as(C.POINTER(C.c_float)), n,
                                             t.ctypes.data_as(C.POINTER(C.c_float)), prim.ctypes.data_as(C.POINTER(C.c_int32))))
        return t, prim
