"""The temporal accumulation of the CPU mirror (tests/hostsim/temporalsim.cpp: moptix_denoise_temporal, with or without the option
"temporal_face_motion") and scene helpers for the temporal-accumulation tests."""
import ctypes as C

import numpy as np

from common import K, _f32, _ptr, hostsim_lib
from denoise_helpers import DEFAULTS

TEMPORAL_DEFAULTS = dict(alpha=0.2, alpha_moments=0.2, depth_tolerance=0.2, normal_threshold=0.5, max_history=32, variance_frames=4)


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
    """A context's temporal state, with the face snapshot, on the CPU.  run() is Context.denoise_temporal over host arrays and the faces as
    they stand on the device; set_option() is set_option("temporal_face_motion", v), off by default; faces_changed() is what update_faces
    and build_accel do to that state, clear_scene() what moptix_clear_scene does, reset() is temporal_reset."""

    def __init__(self, option=0):
        self._h = C.c_void_p(hostsim_lib().temporalsim_create())
        self.set_option(option)

    def __del__(self):
        if getattr(self, "_h", None):
            hostsim_lib().temporalsim_destroy(self._h)
            self._h = None

    def reset(self):
        hostsim_lib().temporalsim_reset(self._h)

    def clear_scene(self):
        hostsim_lib().temporalsim_clear_scene(self._h)

    def faces_changed(self):
        hostsim_lib().temporalsim_faces_changed(self._h)

    def set_option(self, value):
        hostsim_lib().temporalsim_set_option(self._h, int(value))

    @property
    def frames(self):
        return int(hostsim_lib().temporalsim_frames(self._h))

    def run(self, accum, aovs, n_accumulation, n_samples, cam, centres=None, face_pos=None, first_face=0, temporal=None, **denoise):
        """accum (H, W, 3) sums; aovs as aov_read / aovsim_render return them (albedo, normal, depth, hits, primId, matId); cam a
        K.CamParams; centres (nSpheres, 3); face_pos (nFaces, 9): the faces on the device now, and first_face = nSpheres + nQuads.
        Returns dict(out, motion, history, pre, info, face_info); face_info is all zeros with the option off."""
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
        rc = hostsim_lib().temporalsim_run(self._h, w, h, _ptr(accum), *[_ptr(a) for a in ins], _ptr(ids[0], C.c_int32), _ptr(ids[1], C.c_int32),
                                           float(n_accumulation), float(n_samples), C.byref(cam), _ptr(centres), len(centres),
                                           _ptr(faces), len(faces), int(first_face), C.byref(p), C.byref(t),
                                           _ptr(out), _ptr(motion), _ptr(hist), _ptr(pre), cnt, fs)
        assert rc == 0
        geo = int(cnt[0])
        info = dict(frames=self.frames, geometry_pixels=geo, history_pixels=int(cnt[1]), disoccluded_pixels=int(cnt[2]),
                    mean_history=float(np.float32(int(cnt[3]) / geo)) if geo else 0.0)
        face_info = dict(tracked_faces=int(fs[0]), moved_faces=int(fs[1]), moved_pixels=int(fs[2]))
        return dict(out=out, motion=motion, history=hist, pre=pre, info=info, face_info=face_info)


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
