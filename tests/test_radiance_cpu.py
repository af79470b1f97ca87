"""Radiance queries on the CPU: the mirror of the kernel's per-sample code (tests/hostsim/radiancesim.cpp) against the render's mirror -- a camera's own
rays and RNG states give the frame, bit for bit -- and against the recursive oracle's orc_trace_one, which nothing else uses; then the
contract of the entry: seeds and states, chunking, sample lists, the t channel, invalid rays, the depth cap, bad arguments."""
import ctypes as C

import numpy as np
import pytest

from common import K, M, HostsimHandle, MovedScene, hostsim_render, oracle_scene, rmse
from oracle import oracle as O
from query_helpers import box_rays, coffee_rays, invalid_rays, querysim
from radiance_helpers import as_seeds, camera_sum, radiancesim, same_bits

SCENES = [("spheres", dict(farg=0.5)), ("cornell_quads", {}), ("file:coffee", {}), ("random_spheres", dict(iarg=60))]
IDS = [s[0].replace("file:", "") for s in SCENES]


@pytest.fixture(scope="module")
def coffee():
    hs = M.HostScene("file:coffee", 32, 18)
    sim = HostsimHandle(hs)
    yield hs, sim, coffee_rays(n=256)
    sim.close()


def _unit_tmin(hs, rays):
    """The rays as the oracle's orc_trace_one walks them: from the scene's rayEpsilonT to its default far end."""
    r = rays.copy()
    r[:, 6] = np.float32(hs.params.rayEpsilonT); r[:, 7] = np.float32(1e27)
    return r


@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("kind,kw", SCENES, ids=IDS)
def test_camera_rays_and_states_give_the_renders_accumulation_buffer(kind, kw, fmt):
    hs = M.HostScene(kind, 32, 18, **kw)
    sim = HostsimHandle(hs)
    seeds = M.launch_seeds(3)
    want, _ = hostsim_render(sim, seeds, node_format=fmt)
    got = camera_sum(lambda rays, states: radiancesim(sim, rays, states=states, clamp=True, node_format=fmt), hs, seeds)
    assert want.any() and same_bits(got, want)
    sim.close()


@pytest.mark.parametrize("kind,kw", SCENES, ids=IDS)
def test_mirror_equals_the_oracles_trace_one(kind, kw):
    """RMSE over all rays and channels, both results clamped to [0, 1], below 2e-6: the bound test_hostsim_vs_oracle.py holds the same
    pair of codes to.  No ray is left out."""
    hs = M.HostScene(kind, 32, 18, **kw)
    rays = _unit_tmin(hs, coffee_rays(n=256) if kind == "file:coffee" else box_rays(hs, n=2048))
    n = len(rays)
    states = np.random.default_rng(5).integers(0, 2 ** 31, n, dtype=np.int64).astype(np.uint32).reshape(n, 1)
    got = radiancesim(hs, rays, states=states)[:, :3]
    osc = oracle_scene(hs)
    want = np.zeros((n, 3), np.float32)
    f3 = C.c_float * 3
    for i in range(n):
        out = f3()
        O.lib().orc_trace_one(C.byref(osc.c), f3(*rays[i, 0:3]), f3(*rays[i, 3:6]), int(states[i, 0]), out)
        want[i] = out[:]
    assert np.isfinite(got).all() and want.any()
    err = rmse(np.clip(got, 0, 1), np.clip(want, 0, 1))
    print("%s: %d rays, RMSE %.3g, largest difference %.3g" % (kind, n, err, float(np.abs(np.clip(got, 0, 1) - np.clip(want, 0, 1)).max())))
    assert err < 2e-6


def test_seeds_mode_is_states_mode_with_tea16(coffee):
    hs, sim, rays = coffee
    seeds = [11, 0x9e3779b9, 7]
    base = 0xfffffff0                      # the ray index wraps mod 2^32 inside the batch
    states = np.array([[M.api._tea16((base + i) & 0xffffffff, int(s) & 0xffffffff) for s in seeds] for i in range(len(rays))], np.uint32)
    for clamp in (False, True):
        a = radiancesim(sim, rays, seeds=seeds, index_base=base, clamp=clamp)
        assert same_bits(a, radiancesim(sim, rays, states=states, clamp=clamp))
    assert not same_bits(a, radiancesim(sim, rays, seeds=seeds, index_base=0, clamp=True))


def test_two_calls_on_halves_equal_one_call(coffee):
    hs, sim, rays = coffee
    seeds, h = [3, 4], len(rays) // 2
    whole = radiancesim(sim, rays, seeds=seeds)
    parts = np.concatenate([radiancesim(sim, rays[:h], seeds=seeds, index_base=0), radiancesim(sim, rays[h:], seeds=seeds, index_base=h)])
    assert same_bits(whole, parts)


def test_sample_list_is_the_ordered_sum_of_one_sample_calls(coffee):
    hs, sim, rays = coffee
    seeds = [1, 2, 3, 4, 5]
    whole = radiancesim(sim, rays, seeds=seeds)
    acc = np.zeros((len(rays), 3), np.float32)
    for s in seeds:
        acc = (acc + radiancesim(sim, rays, seeds=[s])[:, :3]).astype(np.float32)
    assert same_bits(whole[:, :3], acc) and (whole[:, :3].max(axis=1) > 1.0).any()      # unclamped: a light seen directly is above 1


def test_t_is_the_closest_querys_t(coffee):
    hs, sim, rays = coffee
    short = rays.copy(); short[::2, 7] = 0.3; short[1::4, 6] = -1.0
    for r in (rays, short):
        for fmt in (64, 128):
            got = radiancesim(sim, r, seeds=[9], node_format=fmt)
            hit = querysim(sim, r, "closest", node_format=fmt)
            assert same_bits(got[:, 3], hit["t"])
            assert (hit["prim"] >= 0).sum() > 50 and (hit["prim"] < 0).sum() > 10


def test_invalid_rays_give_zero_and_the_closest_querys_t(coffee):
    hs, sim, _ = coffee
    bad, base = invalid_rays()
    got = radiancesim(sim, bad, seeds=[1, 2], clamp=False)
    assert not got[:, :3].any() and same_bits(got[:, 3], querysim(sim, bad, "closest")["t"])
    assert radiancesim(sim, base[None, :], seeds=[1, 2])[:, :3].any()              # the ray they are made from sees the lit floor


def test_depth_cap_acts_as_in_a_render():
    hs = M.HostScene("cornell_quads", 32, 18)
    rays = box_rays(hs, n=512)
    deep = radiancesim(hs, rays, seeds=[1, 2])
    p = K.Params.from_buffer_copy(hs.params); p.rayMaxDepth = 3
    shallow = radiancesim(MovedScene(hs, params=p), rays, seeds=[1, 2])
    assert hs.params.rayMaxDepth == 256 and np.isfinite(shallow).all()
    assert same_bits(deep[:, 3], shallow[:, 3]) and not same_bits(deep[:, :3], shallow[:, :3])


def test_bad_arguments_without_a_device():
    L = K.device_lib()
    rays = np.zeros((4, 8), np.float32); rays[:, 5] = 1; rays[:, 7] = 1
    out = np.zeros((4, 4), np.float32)
    seeds = as_seeds([1]); states = np.zeros((4, 1), np.uint32)
    rp, op = rays.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float))
    sp, tp = seeds.ctypes.data_as(C.POINTER(C.c_int32)), states.ctypes.data_as(C.POINTER(C.c_uint32))
    assert K.RADIANCE_CLAMP == 1
    assert L.moptix_query_radiance(None, rp, 4, sp, None, 1, 0, 0, op) == K.ERR_INVALID          # NULL context
    assert L.moptix_query_radiance(None, rp, -1, sp, None, 1, 0, 0, op) == K.ERR_INVALID
    assert L.moptix_query_radiance(None, rp, 4, sp, tp, 1, 0, 0, op) == K.ERR_INVALID            # both
    assert L.moptix_query_radiance(None, rp, 4, None, None, 1, 0, 0, op) == K.ERR_INVALID        # neither
    assert L.moptix_query_radiance(None, rp, 4, sp, None, 0, 0, 0, op) == K.ERR_INVALID          # no samples
    assert L.moptix_query_radiance(None, rp, 4, sp, None, 1, 0, 2, op) == K.ERR_INVALID          # unknown flag
    assert L.moptix_query_radiance(None, None, 4, sp, None, 1, 0, 0, None) == K.ERR_INVALID
    assert L.moptix_query_radiance_device(None, None, 4, sp, None, 1, 0, 0, None) == K.ERR_INVALID
    assert L.moptix_query_radiance_device(None, None, 0, None, None, 1, 0, 0, None) == K.ERR_INVALID      # n == 0 still needs a context
