"""Multi-hit ray queries on the MI355X (querykernel.hip pt_rayquery_multi): bit for bit the CPU mirror of the kernel's code
(tests/hostsim/multihitsim.cpp), whole buffers -- hit records, miss records behind them, counts -- on the host path and the tensor path."""
import ctypes as C

import numpy as np
import pytest

from common import M, HostsimHandle
from multihit_helpers import HIT_DTYPE, multisim, same_bits, scene_and_rays
from query_helpers import SCENES, coffee_rays
from refit_helpers import RefitSim, moved_faces
from sign_helpers import mesh_scene

pytestmark = pytest.mark.gpu
K = M._capi


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0)
    gpu_ctx.set_option("query_blocks_per_cu", 32)


def _load(ctx, hs, node_format=0):
    ctx.set_option("node_format", node_format)
    ctx.load(hs)


def _records(t):
    """A tensor path's hits as the host path's array."""
    r = t["records"]
    return r.cpu().numpy().view(HIT_DTYPE).reshape(r.shape[0], r.shape[1])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("kind,iarg", SCENES, ids=[s[0].replace("file:", "") for s in SCENES])
def test_device_is_the_cpu_mirrors_bits(ctx, kind, iarg, fmt):
    import torch
    hs, rays = scene_and_rays(kind, iarg)
    _load(ctx, hs, fmt)
    sim = HostsimHandle(hs, 4)
    rt = torch.from_numpy(rays).to("cuda:0")
    for k in (1, 4, 64):
        for count_all in (False, True):
            want_h, want_c = multisim(sim, rays, k, count_all, node_format=fmt)
            h, c = ctx.query_rays_multi(rays, k, count_all)
            assert h.shape == (len(rays), k) and h.dtype == HIT_DTYPE and c.dtype == np.int32
            assert same_bits(c, want_c), (k, count_all, np.where(c != want_c)[0][:8])
            assert same_bits(h, want_h), (k, count_all)
            th, tc = ctx.query_rays_multi(rt, k, count_all)
            assert th["records"].shape == (len(rays), k, 8) and th["records"].is_cuda and tc.dtype == torch.int32
            assert same_bits(tc.cpu().numpy(), want_c) and same_bits(_records(th), want_h), (k, count_all)
            assert np.array_equal(th["prim"].cpu().numpy(), want_h["prim"]) and same_bits(th["ng"].cpu().numpy(), want_h["ng"])
    assert (want_c > 0).sum() > 100


@pytest.mark.timeout(300)
def test_capped_grid_walks_several_rays_per_lane(ctx):
    """One workgroup per CU and more rays than that grid has lanes, with a partial last block: lanes walk a second ray through the same
    stack columns and list slices of their own.  The mirror's bits, and the bits at the default grid."""
    hs = mesh_scene("torus")
    cus = ctx.get_option("num_cus")
    n = 256 * cus + 257
    rng = np.random.default_rng(31)
    org = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32); org[:, 2] = rng.uniform(-0.8, 0.8, n)
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays = np.ascontiguousarray(np.concatenate([org, d, np.zeros((n, 1), np.float32), np.full((n, 1), 1e27, np.float32)], axis=1))
    _load(ctx, hs)
    default = ctx.query_rays_multi(rays, 3)
    ctx.set_option("query_blocks_per_cu", 1)
    capped = ctx.query_rays_multi(rays, 3)
    want = multisim(hs, rays, 3)
    assert (want[1] == 3).sum() > 500 and (want[1] == 0).sum() > 500 and ((want[1] > 0) & (want[1] < 3)).sum() > 500
    for got in (capped, default):
        assert same_bits(got[1], want[1]) and same_bits(got[0], want[0])
    # coffee's tree is deeper than the LDS stack: the overflow columns of the capped grid, every lane walking many rays
    coffee = M.HostScene("file:coffee", 64, 36)
    _load(ctx, coffee)
    assert 3 * ctx.accel_info().treeDepth + 1 > 32
    crays = coffee_rays(n=n, seed=3)
    got, want = ctx.query_rays_multi(crays, 3, True), multisim(coffee, crays, 3, True)
    assert same_bits(got[1], want[1]) and same_bits(got[0], want[0])


@pytest.mark.timeout(300)
def test_pure_crossing_count(ctx):
    import torch
    hs, rays = scene_and_rays("file:coffee", 0)
    _load(ctx, hs)
    h4, c4 = ctx.query_rays_multi(rays, 4, True)
    h0, c0 = ctx.query_rays_multi(rays, 0, True)
    assert h0.shape == (len(rays), 0) and same_bits(c0, c4) and c4.max() > 4
    counts = np.full(len(rays), -7, np.int32)
    rc = K.device_lib().moptix_query_rays_multi(ctx._h, rays.ctypes.data_as(C.POINTER(C.c_float)), len(rays), 0, K.MULTI_COUNT_ALL, None,
                                                counts.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == K.MOPTIX_OK and same_bits(counts, c4)
    th, tc = ctx.query_rays_multi(torch.from_numpy(rays).to("cuda:0"), 0, True)
    assert th["records"].shape == (len(rays), 0, 8) and same_bits(tc.cpu().numpy(), c4)


@pytest.mark.timeout(300)
def test_leaves_the_context_alone(ctx):
    hs, rays = scene_and_rays("file:coffee", 0)
    _load(ctx, hs)
    seeds = M.launch_seeds(1)
    ctx.accum_clear(); ctx.render(seeds)
    accum = ctx.accum_read()
    before = ctx.query_rays(rays)
    addr = ctx.debug_buffer_addresses()
    assert addr["query_overflow"] != 0
    h, c = ctx.query_rays_multi(rays, 8, True)
    assert ctx.debug_buffer_addresses() == addr
    assert same_bits(ctx.query_rays(rays), before) and same_bits(np.ascontiguousarray(h[:, 0]), before)
    assert same_bits(ctx.accum_read(), accum)
    assert np.array_equal(c > 0, ctx.query_rays(rays, "any") == 1)


@pytest.mark.timeout(300)
def test_after_update_faces(ctx):
    hs, rays = scene_and_rays("file:coffee", 0)
    _load(ctx, hs)
    fp, rows = moved_faces(hs, 0.05)
    ctx.update_faces(0, rows)
    with pytest.raises(M.MoptixError) as e:
        ctx.query_rays_multi(rays, 4)
    assert e.value.code == K.ERR_STATE
    ctx.refit_accel()
    sim = RefitSim(hs, 4, 1)
    sim.update(0, rows); sim.refit()
    for count_all in (False, True):
        got = ctx.query_rays_multi(rays, 4, count_all)
        want = multisim(sim._sim, rays, 4, count_all)
        assert same_bits(got[1], want[1]) and same_bits(got[0], want[0]), count_all
    assert not same_bits(want[0], multisim(hs, rays, 4, True)[0])      # the move changed the answer


@pytest.mark.timeout(300)
def test_argument_errors(ctx):
    import torch
    hs, rays = scene_and_rays("spheres", 0)
    _load(ctx, hs)
    L, h = K.device_lib(), ctx._h
    hits, counts = np.zeros((4, 65), HIT_DTYPE), np.zeros(4, np.int32)
    rp, hp, cp = rays.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(hits.ctypes.data), counts.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.moptix_query_rays_multi(h, rp, 4, 4, 0, hp, cp) == K.MOPTIX_OK
    assert L.moptix_query_rays_multi(h, rp, 4, 0, 0, hp, cp) == K.ERR_INVALID              # maxHits 0 without the flag
    assert L.moptix_query_rays_multi(h, rp, 4, 0, K.MULTI_COUNT_ALL, None, cp) == K.MOPTIX_OK
    assert L.moptix_query_rays_multi(h, rp, 4, 65, 0, hp, cp) == K.ERR_INVALID
    assert L.moptix_query_rays_multi(h, rp, 4, 65, K.MULTI_COUNT_ALL, hp, cp) == K.ERR_INVALID
    assert L.moptix_query_rays_multi(h, rp, 4, -1, K.MULTI_COUNT_ALL, hp, cp) == K.ERR_INVALID
    assert L.moptix_query_rays_multi(h, rp, 4, 4, 2, hp, cp) == K.ERR_INVALID              # an unknown flag
    assert L.moptix_query_rays_multi(h, rp, 4, 4, 0x80000001, hp, cp) == K.ERR_INVALID
    assert L.moptix_query_rays_multi(h, rp, -1, 4, 0, hp, cp) == K.ERR_INVALID
    assert L.moptix_query_rays_multi(h, None, 4, 4, 0, hp, cp) == K.ERR_INVALID
    assert L.moptix_query_rays_multi(h, rp, 4, 4, 0, None, cp) == K.ERR_INVALID
    assert L.moptix_query_rays_multi(h, rp, 4, 4, 0, hp, None) == K.ERR_INVALID
    assert L.moptix_query_rays_multi(h, None, 0, 4, 0, None, None) == K.MOPTIX_OK
    assert L.moptix_query_rays_multi_device(h, None, 0, 4, 0, None, None) == K.MOPTIX_OK
    dev = torch.device("cuda", 0)
    dr = torch.from_numpy(rays[:4].copy()).to(dev)
    dh = torch.zeros((4 * 4 * 8 + 8,), dtype=torch.float32, device=dev)
    dc = torch.zeros(8, dtype=torch.int32, device=dev)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    assert L.moptix_query_rays_multi_device(h, vp(dr), 4, 4, 0, vp(dh), vp(dc)) == K.MOPTIX_OK
    ctx.sync()
    assert L.moptix_query_rays_multi_device(h, vp(dr), 4, 4, 0, vp(dh, 4), vp(dc)) == K.ERR_INVALID      # misaligned hits
    assert L.moptix_query_rays_multi_device(h, vp(dr), 4, 4, 0, vp(dh), vp(dc, 2)) == K.ERR_INVALID      # misaligned counts
    assert L.moptix_query_rays_multi_device(h, vp(dr, 4), 3, 4, 0, vp(dh), vp(dc)) == K.ERR_INVALID      # misaligned rays
    assert L.moptix_query_rays_multi_device(h, vp(dr), 4, 4, 0, None, vp(dc)) == K.ERR_INVALID
    assert L.moptix_query_rays_multi_device(h, vp(dr), 4, 0, 0, vp(dh), vp(dc)) == K.ERR_INVALID
    assert L.moptix_query_rays_multi_device(h, vp(dr), 4, 65, 0, vp(dh), vp(dc)) == K.ERR_INVALID
    assert L.moptix_query_rays_multi_device(h, vp(dr), 4, 4, 4, vp(dh), vp(dc)) == K.ERR_INVALID
    for bad in (dr[:, :7], dr.cpu(), dr.double(), dr.reshape(-1)):
        with pytest.raises(ValueError):
            ctx.query_rays_multi(bad, 4)
    with pytest.raises(ValueError):
        ctx.query_rays_multi(dr, 0)
    fresh = M.Context(0)
    try:
        assert L.moptix_query_rays_multi(fresh._h, rp, 4, 4, 0, hp, cp) == K.ERR_STATE      # no params, no tree
    finally:
        fresh.close()
