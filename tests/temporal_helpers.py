"""Bindings of tests/temporalsim (the CPU mirror of moptix_denoise_temporal) and scene helpers for the temporal-accumulation tests."""
import ctypes as C
import os
import subprocess

import numpy as np

from common import REPO, K
from denoise_helpers import DEFAULTS, _f32, _ptr

_DIR = os.path.join(REPO, "tests", "temporalsim")
_lib = None

TEMPORAL_DEFAULTS = dict(alpha=0.2, alpha_moments=0.2, depth_tolerance=0.2, normal_threshold=0.5, max_history=32, variance_frames=4)


def temporalsim_lib():
    global _lib
    if _lib is None:
        path = os.path.join(_DIR, "libtemporalsim.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _DIR, "-s"])
        L = C.CDLL(path)
        f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.temporalsim_create.restype = C.c_void_p
        L.temporalsim_destroy.argtypes = [C.c_void_p]
        L.temporalsim_reset.argtypes = [C.c_void_p]
        L.temporalsim_frames.argtypes = [C.c_void_p]; L.temporalsim_frames.restype = C.c_uint64
        L.temporalsim_run.argtypes = [C.c_void_p, C.c_int, C.c_int, f32p, f32p, f32p, f32p, f32p, i32p, i32p, C.c_float, C.c_float,
                                      C.POINTER(K.CamParams), f32p, C.c_int, C.POINTER(K.DenoiseParams), C.POINTER(K.TemporalParams),
                                      f32p, f32p, f32p, f32p, C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


def temporal_params(temporal=None):
    t = dict(TEMPORAL_DEFAULTS)
    t.update(temporal or {})
    return K.TemporalParams(float(t["alpha"]), float(t["alpha_moments"]), float(t["depth_tolerance"]), float(t["normal_threshold"]),
                            int(t["max_history"]), int(t["variance_frames"]))


def cam_params(origin, horizontal, vertical, lower_left):
    c = K.CamParams()
    for name, v in (("origin", origin), ("horizontal", horizontal), ("vertical", vertical), ("scrLowerLeftCorner", lower_left)):
        setattr(c, name, K.Float3(*[float(np.float32(x)) for x in v]))
    return c


class TemporalSim:
    """A context's temporal state on the CPU: run() is Context.denoise_temporal over host arrays, reset() is temporal_reset (and what
    moptix_clear_scene does to the history)."""

    def __init__(self):
        self._h = C.c_void_p(temporalsim_lib().temporalsim_create())

    def __del__(self):
        if getattr(self, "_h", None):
            temporalsim_lib().temporalsim_destroy(self._h)
            self._h = None

    def reset(self):
        temporalsim_lib().temporalsim_reset(self._h)

    @property
    def frames(self):
        return int(temporalsim_lib().temporalsim_frames(self._h))

    def run(self, accum, aovs, n_accumulation, n_samples, cam, centres=None, temporal=None, **denoise):
        """accum (H, W, 3) sums; aovs as aov_read / aovsim_render return them (albedo, normal, depth, hits, primId, matId); cam a
        K.CamParams; centres (nSpheres, 3).  Returns dict(out, motion, history, pre, info)."""
        accum = _f32(accum)
        h, w = accum.shape[:2]
        ins = [_f32(aovs[n]) for n in ("albedo", "normal", "depth", "hits")]
        ids = [np.ascontiguousarray(aovs[n], np.int32) for n in ("primId", "matId")]
        assert ins[0].size == ins[1].size == 3 * h * w and ins[2].size == ins[3].size == ids[0].size == ids[1].size == h * w
        centres = np.zeros((0, 3), np.float32) if centres is None else _f32(centres).reshape(-1, 3)
        d = dict(DEFAULTS); d.update(denoise)
        p = K.DenoiseParams(int(d["iterations"]), int(d["normal_power"]), 1 if d["demodulate"] else 0, float(d["sigma_luminance"]), float(d["sigma_depth"]))
        t = temporal_params(temporal)
        out = np.empty((h, w, 3), np.float32); motion = np.empty((h, w, 2), np.float32); hist = np.empty((h, w), np.float32)
        pre = np.empty((h, w, 4), np.float32)
        cnt = (C.c_uint64 * 4)()
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        rc = temporalsim_lib().temporalsim_run(self._h, w, h, _ptr(accum), *[_ptr(a) for a in ins], i32(ids[0]), i32(ids[1]), float(n_accumulation),
                                               float(n_samples), C.byref(cam), _ptr(centres), len(centres), C.byref(p), C.byref(t),
                                               _ptr(out), _ptr(motion), _ptr(hist), _ptr(pre), cnt)
        assert rc == 0
        geo = int(cnt[0])
        info = dict(frames=self.frames, geometry_pixels=geo, history_pixels=int(cnt[1]), disoccluded_pixels=int(cnt[2]),
                    mean_history=float(np.float32(int(cnt[3]) / geo)) if geo else 0.0)
        return dict(out=out, motion=motion, history=hist, pre=pre, info=info)


class MovedScene:
    """A HostScene with other spheres and / or another camera, for the CPU renderers (hostsim_render, aovsim_render read a scene
    through params, sizes, flat(), face_arrays() and face_uvs())."""

    def __init__(self, hs, spheres=None, params=None):
        self._hs, self._spheres = hs, spheres
        self.params = hs.params if params is None else params
        self.width, self.height, self.sizes = hs.width, hs.height, hs.sizes

    def flat(self):
        f = dict(self._hs.flat())
        if self._spheres is not None:
            f["spheres"] = self._spheres
        return f

    def face_arrays(self):
        return self._hs.face_arrays()

    def face_uvs(self):
        return self._hs.face_uvs()


def sphere_array(hs):
    n = hs.sizes.nSpheres
    sph = (K.SphereParams * max(1, n))()
    for i in range(n):
        sph[i] = hs.flat()["spheres"][i]
    return sph, n


def copy_spheres(sph, n):
    out = (K.SphereParams * max(1, n))()
    C.memmove(out, sph, C.sizeof(K.SphereParams) * n)
    return out


def centres_of(sph, n):
    return np.array([[sph[i].center.x, sph[i].center.y, sph[i].center.z] for i in range(n)], np.float32).reshape(-1, 3)


def cam_of(params):
    return K.CamParams.from_buffer_copy(params.cam)


def moved_camera(params, offset):
    """A copy of `params` whose camera is translated by `offset` (origin and screen corner move together: the view direction stays)."""
    p = K.Params.from_buffer_copy(params)
    for name in ("origin", "scrLowerLeftCorner"):
        v = getattr(p.cam, name)
        setattr(p.cam, name, K.Float3(*[float(np.float32(a) + np.float32(b)) for a, b in zip(v.tolist(), offset)]))
    return p
