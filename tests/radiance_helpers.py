"""The radiance queries of the CPU mirror (tests/hostsim/radiancesim.cpp, in libhostsim.so), and the camera's rays and RNG states the
radiance tests start from."""
import ctypes as C

import numpy as np

from common import K, _f32, _hostsim_scene, _ptr, hostsim_handle, hostsim_lib
from query_helpers import same_bits      # noqa: F401  (for the tests)

CLAMP = K.RADIANCE_CLAMP


def as_seeds(seeds):
    """Launch seeds as the int32 words the C entries take (values above 2^31 wrap, as M.launch_seeds' do)."""
    return np.ascontiguousarray((np.asarray(seeds).astype(np.int64).reshape(-1) & 0xffffffff).astype(np.uint32)).view(np.int32)


def radiancesim(hs, rays, seeds=None, states=None, clamp=False, index_base=0, node_format=64, leaf_size=4):
    """moptix_query_radiance on the CPU: (n, 4) float32 r g b t.  hs: a scene, or a built one."""
    sim = hostsim_handle(hs, leaf_size)
    rays = _f32(np.asarray(rays, np.float32).reshape(-1, 8))
    n = len(rays)
    out = np.zeros((n, 4), np.float32)
    sd = None if seeds is None else as_seeds(seeds)
    st = None if states is None else np.ascontiguousarray(np.asarray(states).view(np.uint32).reshape(n, -1))
    ns = len(sd) if sd is not None else st.shape[1]
    rc = hostsim_lib().radiancesim_query(sim._h, int(node_format), _ptr(rays), n, None if sd is None else _ptr(sd, C.c_int32),
                                         None if st is None else _ptr(st, C.c_uint32), ns, int(index_base) & 0xffffffff,
                                         CLAMP if clamp else 0, _ptr(out))
    assert rc == 0
    return out


def shadow_rule(sim, rule):
    """moptix option "shadow_rule" on a built scene of the mirror (a HostsimHandle)."""
    assert hostsim_lib().radiancesim_shadow_rule(sim._h, int(rule)) == 0


def tea16(v0, v1):
    """pt_rng.h tea16 on uint32 arrays (broadcast): the RNG state of ray index v0 under launch seed v1."""
    v0 = np.asarray(v0).astype(np.uint32); v1 = np.asarray(v1).astype(np.uint32)
    v0, v1 = np.broadcast_arrays(v0, v1)
    v0 = v0.copy(); v1 = v1.copy()
    s0 = np.uint32(0)
    with np.errstate(over="ignore"):
        for _ in range(16):
            s0 = np.uint32((int(s0) + 0x9e3779b9) & 0xffffffff)
            v0 += ((v1 << np.uint32(4)) + np.uint32(0xa341316c)) ^ (v1 + s0) ^ ((v1 >> np.uint32(5)) + np.uint32(0xc8013ea4))
            v1 += ((v0 << np.uint32(4)) + np.uint32(0xad90777d)) ^ (v0 + s0) ^ ((v0 >> np.uint32(5)) + np.uint32(0x7e95761e))
    return v0


def seed_states(n, seeds, index_base=0):
    """The (n, nSamples) states that seeds mode starts the samples of rays index_base .. index_base + n from."""
    idx = ((np.arange(n, dtype=np.int64) + int(index_base)) & 0xffffffff).astype(np.uint32)
    return np.ascontiguousarray(tea16(idx[:, None], as_seeds(seeds).view(np.uint32)[None, :]))


def camera_rays_states(hs, seed):
    """begin_sample's primary rays of one launch seed, (H * W, 8), and the RNG state each leaves behind after the lens and jitter draws,
    (H * W, 1) uint32; pixel order = row 0 first."""
    s, keep = _hostsim_scene(hs)
    rays = np.zeros((hs.height * hs.width, 8), np.float32)
    states = np.zeros((hs.height * hs.width, 1), np.uint32)
    rc = hostsim_lib().radiancesim_camera(C.byref(s), int(as_seeds([seed])[0]), _ptr(rays), _ptr(states, C.c_uint32))
    assert rc == 0
    return rays, states


def camera_sum(query, hs, seeds):
    """The frame a camera's own paths give through a radiance query: per launch seed one clamped sample per pixel, added per pixel in seed
    order in float32, (H, W, 3).  query(rays, states) -> (n, 4)."""
    acc = np.zeros((hs.height * hs.width, 3), np.float32)
    for seed in seeds:
        rays, states = camera_rays_states(hs, seed)
        acc = (acc + np.asarray(query(rays, states))[:, :3]).astype(np.float32)
    return acc.reshape(hs.height, hs.width, 3)
