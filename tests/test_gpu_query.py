"""Ray queries on the MI355X (querykernel.hip): bit for bit the CPU mirror of the kernel's code (tests/hostsim/querysim.cpp), the oracle's closest
hits, the AOV pass's ids on the camera rays and moptix_debug_trace's answers -- every ray, exactly."""
import ctypes as C

import numpy as np
import pytest

from common import M, oracle_scene
from aov_helpers import camera_rays
from query_helpers import HIT_DTYPE, SCENES, coffee_rays, invalid_rays, querysim, same_bits, scene_and_rays, shortened

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


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("kind,iarg", SCENES, ids=[s[0].replace("file:", "") for s in SCENES])
def test_gpu_queries_are_the_cpu_mirrors_bits(ctx, kind, iarg, fmt):
    hs, rays = scene_and_rays(kind, iarg)
    _load(ctx, hs, fmt)
    op, ot = oracle_scene(hs).closest_hits(rays)
    bad, _ = invalid_rays()
    neg = rays.copy(); neg[:, 6] = -1.0                                  # walked as tmin = 0
    for r in (rays, shortened(rays, ot, op), bad, neg):
        for mode in ("closest", "any"):
            assert same_bits(ctx.query_rays(r, mode), querysim(hs, r, mode, node_format=fmt)), mode


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind,iarg", SCENES, ids=[s[0].replace("file:", "") for s in SCENES])
def test_gpu_queries_equal_the_oracle(ctx, kind, iarg):
    hs, rays = scene_and_rays(kind, iarg)
    _load(ctx, hs)
    op, ot = oracle_scene(hs).closest_hits(rays)
    hit = op >= 0
    assert hit.sum() > 100
    if kind == "file:coffee":
        assert hit.sum() > 1000 and (~hit).sum() > 100
    h = ctx.query_rays(rays)
    assert np.array_equal(h["prim"], op) and np.array_equal(h["t"][hit], ot[hit])
    assert np.array_equal(ctx.query_rays(rays, "any"), hit.astype(np.int32))
    short = shortened(rays, ot, op)
    sp, st = oracle_scene(hs).closest_hits(short)
    assert np.array_equal(ctx.query_rays(short, "any"), (sp >= 0).astype(np.int32))
    assert np.array_equal(ctx.query_rays(short)["prim"], sp)


@pytest.mark.timeout(300)
def test_grid_size_does_not_change_a_bit(ctx):
    hs, rays = scene_and_rays("file:coffee", 0)
    _load(ctx, hs)
    want = {m: querysim(hs, rays, m) for m in ("closest", "any")}
    for bpc in (1, 4, 64):
        ctx.set_option("query_blocks_per_cu", bpc)
        for m in ("closest", "any"):
            assert same_bits(ctx.query_rays(rays, m), want[m]), (bpc, m)


@pytest.mark.timeout(300)
def test_torch_device_path_returns_the_host_paths_bits(ctx):
    import torch
    hs, rays = scene_and_rays("file:coffee", 0)
    _load(ctx, hs)
    want, want_any = ctx.query_rays(rays), ctx.query_rays(rays, "any")
    dev = torch.device("cuda", 0)
    rt = torch.from_numpy(rays).to(dev)
    got = ctx.query_rays(rt)
    assert got["records"].shape == (len(rays), 8) and got["records"].is_cuda
    assert same_bits(got["records"].cpu().numpy().view(HIT_DTYPE).reshape(-1), want)
    assert np.array_equal(got["prim"].cpu().numpy(), want["prim"]) and np.array_equal(got["mat"].cpu().numpy(), want["mat"])
    assert same_bits(got["t"].cpu().numpy(), want["t"]) and same_bits(got["ng"].cpu().numpy(), want["ng"])
    ga = ctx.query_rays(rt, "any")
    assert ga.dtype == torch.int32 and same_bits(ga.cpu().numpy(), want_any)
    # a slice of a wider tensor, made contiguous
    wide = torch.zeros((len(rays), 10), dtype=torch.float32, device=dev)
    wide[:, 1:9] = rt
    sl = wide[:, 1:9]
    assert same_bits(ctx.query_rays(sl.contiguous())["records"].cpu().numpy().view(HIT_DTYPE).reshape(-1), want)
    for bad in (sl, rt.cpu(), rt.double(), rt.to(torch.float16), rt.reshape(8, -1), rt.reshape(-1)):
        with pytest.raises(ValueError):
            ctx.query_rays(bad)
    with pytest.raises(ValueError):
        ctx.query_rays(rt, "nearest")


@pytest.mark.timeout(300)
def test_odd_sizes(ctx):
    import torch
    hs, rays = scene_and_rays("file:coffee", 0)
    _load(ctx, hs)
    want, want_any = querysim(hs, rays, "closest"), querysim(hs, rays, "any")
    for n in (1000, 65, 63, 1, 0):
        h, a = ctx.query_rays(rays[:n]), ctx.query_rays(rays[:n], "any")
        assert len(h) == n and len(a) == n
        assert same_bits(h, want[:n]) and same_bits(a, want_any[:n])
        rt = torch.from_numpy(rays[:n].copy()).to("cuda:0")
        assert same_bits(ctx.query_rays(rt)["records"].cpu().numpy().view(HIT_DTYPE).reshape(-1), want[:n])
        assert same_bits(ctx.query_rays(rt, "any").cpu().numpy(), want_any[:n])


@pytest.mark.timeout(300)
def test_bad_arguments(ctx):
    hs, rays = scene_and_rays("spheres", 0)
    _load(ctx, hs)
    L, h = K.device_lib(), ctx._h
    out = np.zeros(4, HIT_DTYPE)
    rp, op = rays.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(out.ctypes.data)
    assert L.moptix_query_rays(h, rp, -1, 0, op) == K.ERR_INVALID
    assert L.moptix_query_rays(h, rp, 4, 2, op) == K.ERR_INVALID
    assert L.moptix_query_rays(h, None, 4, 0, op) == K.ERR_INVALID
    assert L.moptix_query_rays(h, rp, 4, 0, None) == K.ERR_INVALID
    assert L.moptix_query_rays(h, None, 0, 0, None) == K.MOPTIX_OK
    assert L.moptix_query_rays_device(h, None, 0, 1, None) == K.MOPTIX_OK
    assert L.moptix_query_rays_device(h, None, 4, 0, None) == K.ERR_INVALID
    assert L.moptix_query_rays(None, rp, 4, 0, op) == K.ERR_INVALID
    fresh = M.Context(0)
    try:
        assert L.moptix_query_rays(fresh._h, rp, 4, 0, op) == K.ERR_STATE          # no params, no tree
    finally:
        fresh.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["file:coffee", "cornell_quads"])
def test_primary_rays_give_the_aov_ids(ctx, kind):
    hs = M.HostScene(kind, 64, 36)
    seed = int(M.launch_seeds(1)[0])
    _load(ctx, hs)
    ctx.aov_clear()
    ctx.render_aovs([seed])
    g = ctx.aov_read()
    h = ctx.query_rays(camera_rays(hs, seed))
    assert (h["prim"] >= 0).sum() > 500
    assert np.array_equal(h["prim"], g["primId"].reshape(-1)) and np.array_equal(h["mat"], g["matId"].reshape(-1))


@pytest.mark.timeout(300)
def test_query_sees_updated_spheres(ctx):
    hs = M.HostScene("random_spheres", 64, 36, iarg=60)
    _load(ctx, hs)
    n = hs.sizes.nSpheres
    sph = (K.SphereParams * n)()
    for i in range(n):
        sph[i] = hs.flat()["spheres"][i]
    c = np.array([[s.center.x, s.center.y, s.center.z] for s in sph], np.float32)
    r = np.array([s.radius for s in sph], np.float32)
    org = c.copy(); org[:, 1] += r + np.float32(0.5)
    rays = np.concatenate([org, np.tile(np.float32([0, -1, 0]), (n, 1)), np.full((n, 1), 1e-3, np.float32), np.full((n, 1), 1e27, np.float32)], axis=1)
    before = ctx.query_rays(rays)
    own = np.where(before["prim"] == np.arange(n))[0]
    assert len(own) > 0
    i = int(own[0])
    assert abs(float(before["t"][i]) - 0.5) < 1e-3
    one = (K.SphereParams * 1)(sph[i])
    one[0].center.y += 0.125                                            # towards the ray's origin
    ctx.update_spheres(i, one, 1)
    after = ctx.query_rays(rays[i:i + 1])
    assert after["prim"][0] == i and abs(float(after["t"][0]) - 0.375) < 1e-3
    assert ctx.query_rays(rays[i:i + 1], "any")[0] == 1
    # moptix_debug_trace, which has always read the spheres as they are, agrees on the whole batch
    t1, p1 = ctx.debug_trace(rays)
    h = ctx.query_rays(rays)
    assert np.array_equal(h["prim"], p1) and same_bits(h["t"][p1 >= 0], t1[p1 >= 0])


@pytest.mark.timeout(600)
def test_a_million_rays_through_a_capped_grid(ctx):
    """2^20 incoherent rays on coffee through a grid of one workgroup per CU: every lane walks many rays one after the other, and the tree
    is deeper than the LDS stack, so the overflow columns are in use.  A 1-in-64 stride against the mirror, and the whole occlusion
    output against the whole closest one."""
    hs = M.HostScene("file:coffee", 64, 36)
    _load(ctx, hs)
    ctx.set_option("query_blocks_per_cu", 1)
    assert 3 * ctx.accel_info().treeDepth + 1 > 32                      # the stack bound of this tree: deeper than the LDS part
    rays = coffee_rays(n=1 << 20, seed=3)
    h, a = ctx.query_rays(rays), ctx.query_rays(rays, "any")
    assert np.array_equal(a, (h["prim"] >= 0).astype(np.int32))
    assert (a == 1).sum() > 100000 and (a == 0).sum() > 10000
    sub = rays[::64]
    assert same_bits(h[::64], querysim(hs, sub, "closest")) and same_bits(a[::64], querysim(hs, sub, "any"))
    miss = h[h["prim"] < 0]
    assert (miss["t"] == np.float32(1e27)).all() and (miss["mat"] == -1).all() and not miss["ng"].any()


@pytest.mark.timeout(300)
def test_debug_trace_still_gives_its_old_answer(ctx):
    hs, rays = scene_and_rays("file:coffee", 0)
    _load(ctx, hs)
    t, prim = ctx.debug_trace(rays)
    op, ot = oracle_scene(hs).closest_hits(rays)
    assert np.array_equal(prim, op) and np.array_equal(t[op >= 0], ot[op >= 0])
    h = ctx.query_rays(rays)
    assert np.array_equal(h["prim"], prim) and same_bits(h["t"], t)
