"""Bindings of tests/facemotionsim (the CPU mirror of moptix_denoise_temporal with the option "temporal_face_motion") and scene helpers
for the face-motion tests."""
import ctypes as C
import os
import subprocess

import numpy as np

from common import M, REPO, K
from denoise_helpers import DEFAULTS, _f32, _ptr
from temporal_helpers import temporal_params
from refit_helpers import MovedScene

_DIR = os.path.join(REPO, "tests", "facemotionsim")
_lib = None


def facemotionsim_lib():
    global _lib
    if _lib is None:
        path = os.path.join(_DIR, "libfacemotionsim.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _DIR, "-s"])
        L = C.CDLL(path)
        f32p, i32p, vp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p
        L.facemotionsim_create.restype = vp
        for name in ("destroy", "reset", "clear_scene", "faces_changed"):
            getattr(L, "facemotionsim_" + name).argtypes = [vp]
            getattr(L, "facemotionsim_" + name).restype = None
        L.facemotionsim_set_option.argtypes = [vp, C.c_int]; L.facemotionsim_set_option.restype = None
        L.facemotionsim_frames.argtypes = [vp]; L.facemotionsim_frames.restype = C.c_uint64
        L.facemotionsim_run.argtypes = [vp, C.c_int, C.c_int, f32p, f32p, f32p, f32p, f32p, i32p, i32p, C.c_float, C.c_float,
                                        C.POINTER(K.CamParams), f32p, C.c_int, f32p, C.c_int, C.c_int, C.POINTER(K.DenoiseParams),
                                        C.POINTER(K.TemporalParams), f32p, f32p, f32p, f32p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


class FaceMotionSim:
    """A context's temporal state with the face snapshot on the CPU.  run() is Context.denoise_temporal over host arrays and the faces as
    they stand on the device; set_option() is set_option("temporal_face_motion", v); faces_changed() is what update_faces and
    build_accel do to that state, clear_scene() what moptix_clear_scene does, reset() is temporal_reset."""

    def __init__(self, option=1):
        self._h = C.c_void_p(facemotionsim_lib().facemotionsim_create())
        self.set_option(option)

    def __del__(self):
        if getattr(self, "_h", None):
            facemotionsim_lib().facemotionsim_destroy(self._h)
            self._h = None

    def reset(self):
        facemotionsim_lib().facemotionsim_reset(self._h)

    def clear_scene(self):
        facemotionsim_lib().facemotionsim_clear_scene(self._h)

    def faces_changed(self):
        facemotionsim_lib().facemotionsim_faces_changed(self._h)

    def set_option(self, value):
        facemotionsim_lib().facemotionsim_set_option(self._h, int(value))

    @property
    def frames(self):
        return int(facemotionsim_lib().facemotionsim_frames(self._h))

    def run(self, accum, aovs, n_accumulation, n_samples, cam, centres=None, face_pos=None, first_face=0, temporal=None, **denoise):
        """As TemporalSim.run, plus face_pos (nFaces, 9): the faces on the device now, and first_face = nSpheres + nQuads.  Returns
        dict(out, motion, history, pre, info, face_info)."""
        accum = _f32(accum)
        h, w = accum.shape[:2]
        ins = [_f32(aovs[n]) for n in ("albedo", "normal", "depth", "hits")]
        ids = [np.ascontiguousarray(aovs[n], np.int32) for n in ("primId", "matId")]
        assert ins[0].size == ins[1].size == 3 * h * w and ins[2].size == ins[3].size == ids[0].size == ids[1].size == h * w
        centres = np.zeros((0, 3), np.float32) if centres is None else _f32(centres).reshape(-1, 3)
        faces = np.zeros((0, 9), np.float32) if face_pos is None else _f32(face_pos).reshape(-1, 9)
        d = dict(DEFAULTS); d.update(denoise)
        p = K.DenoiseParams(int(d["iterations"]), int(d["normal_power"]), 1 if d["demodulate"] else 0, float(d["sigma_luminance"]), float(d["sigma_depth"]))
        t = temporal_params(temporal)
        out = np.empty((h, w, 3), np.float32); motion = np.empty((h, w, 2), np.float32); hist = np.empty((h, w), np.float32)
        pre = np.empty((h, w, 4), np.float32)
        cnt = (C.c_uint64 * 4)(); fs = (C.c_uint64 * 3)()
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        rc = facemotionsim_lib().facemotionsim_run(self._h, w, h, _ptr(accum), *[_ptr(a) for a in ins], i32(ids[0]), i32(ids[1]),
                                                   float(n_accumulation), float(n_samples), C.byref(cam), _ptr(centres), len(centres),
                                                   _ptr(faces), len(faces), int(first_face), C.byref(p), C.byref(t),
                                                   _ptr(out), _ptr(motion), _ptr(hist), _ptr(pre), cnt, fs)
        assert rc == 0
        geo = int(cnt[0])
        info = dict(frames=self.frames, geometry_pixels=geo, history_pixels=int(cnt[1]), disoccluded_pixels=int(cnt[2]),
                    mean_history=float(np.float32(int(cnt[3]) / geo)) if geo else 0.0)
        face_info = dict(tracked_faces=int(fs[0]), moved_faces=int(fs[1]), moved_pixels=int(fs[2]))
        return dict(out=out, motion=motion, history=hist, pre=pre, info=info, face_info=face_info)


def first_face(hs):
    """primId of face 0: ids are spheres, quads, triangles in upload order."""
    return int(hs.sizes.nSpheres) + int(hs.sizes.nQuads)


def with_params(scene, params):
    """`scene` (a refit_helpers.MovedScene) under another camera."""
    scene.params = params
    return scene


def translated(face_pos, offset):
    """(nFaces, 9) float32: every vertex moved by `offset`, one binary32 addition per component."""
    fp = np.asarray(face_pos, np.float32).reshape(-1, 3, 3)
    return (fp + np.asarray(offset, np.float32)[None, None, :]).astype(np.float32).reshape(-1, 9)


def grid_mesh_scene(nx, ny, x0, x1, y0, y1, z, width=64, height=36):
    """A flat nx x ny grid of quads, two triangles each, in the plane at depth `z` of coffee's frame (its camera, materials and lights;
    none of its own faces): triangles a few pixels wide when nx, ny are large.  Returns the MovedScene."""
    xs = np.linspace(x0, x1, nx + 1, dtype=np.float32); ys = np.linspace(y0, y1, ny + 1, dtype=np.float32)
    faces = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = (xs[i], ys[j], z), (xs[i + 1], ys[j], z), (xs[i + 1], ys[j + 1], z), (xs[i], ys[j + 1], z)
            faces.append(a + b + c); faces.append(a + c + d)
    return MovedScene(M.HostScene("file:coffee", width, height), np.asarray(faces, np.float32), new_faces=True)
