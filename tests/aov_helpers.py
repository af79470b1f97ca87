"""The AOV render of the CPU mirror (tests/hostsim/aovsim.cpp) for the AOV tests."""
import ctypes as C

import numpy as np

from common import AOV_NAMES, AovsimBuffers, _hostsim_scene, _ptr, hostsim_handle, hostsim_lib

AOV_CHANNELS = dict(albedo=3, normal=3, depth=1, hits=1, primId=1, matId=1)


def empty_aovs(h, w):
    """The buffers of a cleared context: sums 0, ids -1."""
    out = {n: np.zeros((h, w, AOV_CHANNELS[n]), np.int32 if n in ("primId", "matId") else np.float32) for n in AOV_NAMES}
    out["primId"][:] = -1
    out["matId"][:] = -1
    out["samples"] = 0
    return out


def aovsim_render(hs, seeds, leaf_size=4, node_format=64, aovs=None):
    """moptix_render_aovs on the CPU: adds the seeds to `aovs` (a dict as empty_aovs returns; a fresh one by default) and returns it.
    hs: a scene, or a built one."""
    sim = hostsim_handle(hs, leaf_size)
    if aovs is None:
        aovs = empty_aovs(sim.height, sim.width)
    seeds = np.ascontiguousarray(np.asarray(seeds, np.int32))
    b = AovsimBuffers(*[aovs[n].ctypes.data for n in AOV_NAMES], aovs["samples"])
    rc = hostsim_lib().aovsim_render_aovs(sim._h, int(node_format), _ptr(seeds, C.c_int32), len(seeds), C.byref(b))
    assert rc == 0
    aovs["samples"] = int(b.samples)
    return aovs


def camera_rays(hs, seed):
    """begin_sample's primary rays of one seed, (H * W, 8) = o, d, tmin, tmax (moptix_debug_trace's layout), pixel order = row 0 first."""
    s, keep = _hostsim_scene(hs)
    rays = np.zeros((hs.height * hs.width, 8), np.float32)
    rc = hostsim_lib().aovsim_camera_rays(C.byref(s), int(seed), _ptr(rays))
    assert rc == 0
    return rays
