"""Bindings of tests/aovsim (the CPU mirror of the AOV kernel) for the AOV tests."""
import ctypes as C
import os
import subprocess

import numpy as np

from common import REPO, HostsimScene, _hostsim_scene

_AOVSIM_DIR = os.path.join(REPO, "tests", "aovsim")
_aovsim = None

AOV_NAMES = ("albedo", "normal", "depth", "hits", "primId", "matId")
AOV_CHANNELS = dict(albedo=3, normal=3, depth=1, hits=1, primId=1, matId=1)


class AovsimBuffers(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in AOV_NAMES] + [("samples", C.c_uint64)]


def aovsim_lib():
    global _aovsim
    if _aovsim is None:
        path = os.path.join(_AOVSIM_DIR, "libaovsim.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _AOVSIM_DIR, "-s"])
        L = C.CDLL(path)
        L.aovsim_render_aovs.argtypes = [C.POINTER(HostsimScene), C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(AovsimBuffers)]
        L.aovsim_camera_rays.argtypes = [C.POINTER(HostsimScene), C.c_int32, C.POINTER(C.c_float)]
        _aovsim = L
    return _aovsim


def empty_aovs(h, w):
    """The buffers of a cleared context: sums 0, ids -1."""
    out = {n: np.zeros((h, w, AOV_CHANNELS[n]), np.int32 if n in ("primId", "matId") else np.float32) for n in AOV_NAMES}
    out["primId"][:] = -1
    out["matId"][:] = -1
    out["samples"] = 0
    return out


def aovsim_render(hs, seeds, leaf_size=4, node_format=64, aovs=None):
    """moptix_render_aovs on the CPU: adds the seeds to `aovs` (a dict as empty_aovs returns; a fresh one by default) and returns it."""
    if aovs is None:
        aovs = empty_aovs(hs.height, hs.width)
    s, keep = _hostsim_scene(hs)
    seeds = np.ascontiguousarray(np.asarray(seeds, np.int32))
    b = AovsimBuffers(*[aovs[n].ctypes.data for n in AOV_NAMES], aovs["samples"])
    rc = aovsim_lib().aovsim_render_aovs(C.byref(s), int(leaf_size), int(node_format), seeds.ctypes.data_as(C.POINTER(C.c_int32)), len(seeds), C.byref(b))
    assert rc == 0
    aovs["samples"] = int(b.samples)
    return aovs


def camera_rays(hs, seed):
    """begin_sample's primary rays of one seed, (H * W, 8) = o, d, tmin, tmax (moptix_debug_trace's layout), pixel order = row 0 first."""
    s, keep = _hostsim_scene(hs)
    rays = np.zeros((hs.height * hs.width, 8), np.float32)
    rc = aovsim_lib().aovsim_camera_rays(C.byref(s), int(seed), rays.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0
    return rays
