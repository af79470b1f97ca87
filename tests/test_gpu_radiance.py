"""Radiance queries on the MI355X (radiancekernel.hip): bit for bit the CPU mirror of the kernel's per-sample code (tests/hostsim/radiancesim.cpp), the
frame of moptix_render from the camera's own rays and states, and the contract of the entry: sizes, scheduling, stream, state, and a
context that is otherwise untouched."""
import ctypes as C

import numpy as np
import pytest

from common import K, M, HostsimHandle, textured_scene, write_glass_over_opaque_scene
from query_helpers import box_rays, coffee_rays, querysim
from radiance_helpers import camera_sum, radiancesim, same_bits, seed_states, shadow_rule
from refit_helpers import RefitSim, moved_faces

pytestmark = pytest.mark.gpu

SEEDS = [5, 0x9e3779b9, 77, 12345]


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    for name, v in (("leaf_size", 4), ("node_format", 0), ("query_blocks_per_cu", 32), ("radiance_buffer_mb", 256), ("shadow_rule", 1)):
        gpu_ctx.set_option(name, v)


@pytest.fixture(scope="module")
def coffee():
    hs = M.HostScene("file:coffee", 64, 36)
    sim = HostsimHandle(hs)
    yield hs, sim
    sim.close()


def _scene(case, tmp_path):
    """(scene, rays, shadow rule) of a case of the mirror comparison."""
    if case == "glass_rule0" or case == "glass_rule1":
        hs = M.HostScene("file:cornell", 64, 36, base_folder=write_glass_over_opaque_scene(tmp_path, True))
        return hs, box_rays(hs), int(case[-1])
    if case == "textured":
        hs = textured_scene(tmp_path, 64, 36)
        return hs, box_rays(hs), 1
    kind, kw = {"spheres": ("spheres", dict(farg=0.5)), "cornell_quads": ("cornell_quads", {}), "coffee": ("file:coffee", {}),
                "random_spheres": ("random_spheres", dict(iarg=60))}[case]
    hs = M.HostScene(kind, 64, 36, **kw)
    return hs, (coffee_rays(n=2048) if case == "coffee" else box_rays(hs)), 1


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("case", ["spheres", "cornell_quads", "coffee", "random_spheres", "glass_rule0", "glass_rule1", "textured"])
def test_gpu_radiance_is_the_cpu_mirrors_bits(ctx, tmp_path, case, fmt):
    """2048 rays by 4 samples, with and without the clamp, in seeds mode and in states mode."""
    import torch
    hs, rays, rule = _scene(case, tmp_path)
    ctx.set_option("node_format", fmt); ctx.set_option("shadow_rule", rule)
    ctx.load(hs)
    sim = HostsimHandle(hs)
    shadow_rule(sim, rule)
    base = 1000
    states = seed_states(len(rays), SEEDS, base)
    for clamp in (False, True):
        want = radiancesim(sim, rays, states=states, clamp=clamp, node_format=fmt)
        assert want[:, :3].any() and np.isfinite(want).all()
        assert same_bits(ctx.query_radiance(rays, seeds=SEEDS, index_base=base, clamp=clamp), want), ("seeds", clamp)
        assert same_bits(ctx.query_radiance(rays, states=states, clamp=clamp), want), ("states", clamp)
    got = ctx.query_radiance(torch.from_numpy(rays).to("cuda:0"), states=torch.from_numpy(states.view(np.int32)).to("cuda:0"), clamp=True)
    assert got.is_cuda and same_bits(got.cpu().numpy(), want)
    if case == "glass_rule0":      # the two rules differ on this scene: the option reached the kernel
        shadow_rule(sim, 1)
        assert not same_bits(radiancesim(sim, rays, states=states, clamp=True, node_format=fmt), want)
    sim.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind,kw", [("file:coffee", {}), ("spheres", dict(farg=0.5))], ids=["coffee", "spheres_lens"])
def test_camera_rays_and_states_give_the_rendered_frame(ctx, kind, kw):
    hs = M.HostScene(kind, 64, 36, **kw)
    seeds = M.launch_seeds(3)
    ctx.load(hs)
    ctx.accum_clear(); ctx.render(seeds)
    want = ctx.accum_read()
    got = camera_sum(lambda rays, states: ctx.query_radiance(rays, states=states, clamp=True), hs, seeds)
    assert want.any() and same_bits(got, want)
    assert same_bits(ctx.accum_read(), want)


@pytest.mark.timeout(300)
def test_sizes(ctx, coffee):
    import torch
    hs, sim = coffee
    ctx.load(hs)
    rays = coffee_rays(n=1000, seed=21)
    for ns in (1, 5):
        seeds = SEEDS[:1] if ns == 1 else SEEDS + [99]
        want = radiancesim(sim, rays, seeds=seeds)
        for n in (1000, 65, 63, 1, 0):
            a = ctx.query_radiance(rays[:n], seeds=seeds)
            assert a.shape == (n, 4) and a.dtype == np.float32 and same_bits(a, want[:n]), (n, ns)
            t = ctx.query_radiance(torch.from_numpy(rays[:n].copy()).to("cuda:0"), seeds=seeds)
            assert tuple(t.shape) == (n, 4) and t.dtype == torch.float32 and same_bits(t.cpu().numpy(), a), (n, ns)


@pytest.mark.timeout(300)
def test_scheduling_and_passes_do_not_change_a_bit(ctx, coffee):
    """8192 rays by 16 samples.  With the grid capped at one workgroup per CU the lanes walk many samples one after the other and coffee's
    tree, deeper than the LDS stack, puts the overflow columns to use; a scratch of 1 MB holds 65536 records, so the call runs in two
    passes over the samples; 70000 rays do not fit it with even one sample each and run ray range after ray range."""
    hs, sim = coffee
    ctx.load(hs)
    assert 3 * ctx.accel_info().treeDepth + 1 > 32
    rays = coffee_rays(n=8192, seed=3)
    states = np.random.default_rng(8).integers(0, 2 ** 32, (len(rays), 16), dtype=np.uint64).astype(np.uint32)
    first = ctx.query_radiance(rays, states=states)
    assert same_bits(first[::16], radiancesim(sim, rays[::16], states=states[::16]))
    for bpc in (1, 4, 64):
        ctx.set_option("query_blocks_per_cu", bpc)
        assert same_bits(ctx.query_radiance(rays, states=states), first), bpc
    ctx.set_option("query_blocks_per_cu", 32); ctx.set_option("radiance_buffer_mb", 1)
    assert same_bits(ctx.query_radiance(rays, states=states), first)
    many = coffee_rays(n=70000, seed=4)
    small = ctx.query_radiance(many, seeds=SEEDS[:2], index_base=7)
    ctx.set_option("radiance_buffer_mb", 256)
    assert same_bits(ctx.query_radiance(many, seeds=SEEDS[:2], index_base=7), small)
    sub = slice(65000, 70000, 10)      # rays of the second range: their index is index_base + i
    assert same_bits(small[sub], radiancesim(sim, many[sub], states=seed_states(len(many), SEEDS[:2], 7)[sub]))


@pytest.mark.timeout(300)
def test_device_form_is_asynchronous_on_the_contexts_stream(ctx, coffee):
    import torch
    hs, sim = coffee
    ctx.load(hs)
    rays = coffee_rays(n=4096, seed=5)
    want = ctx.query_radiance(rays, seeds=SEEDS)
    L, h, dev = K.device_lib(), ctx._h, torch.device("cuda", 0)
    seeds = np.asarray(SEEDS, np.uint32).view(np.int32)
    sp = seeds.ctypes.data_as(C.POINTER(C.c_int32))
    rt = torch.from_numpy(rays).to(dev)
    out = torch.zeros((len(rays), 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    # the context's own stream: moptix_sync makes the result readable
    assert L.moptix_query_radiance_device(h, C.c_void_p(rt.data_ptr()), len(rays), sp, None, len(SEEDS), 0, 0, C.c_void_p(out.data_ptr())) == K.MOPTIX_OK
    ctx.sync()
    assert same_bits(out.cpu().numpy(), want)
    # (a stream of the caller's, busy, with the rays arriving behind the delay: test_gpu_async.py, the radiance cases)
    misaligned = C.c_void_p(rt.data_ptr() + 4)
    assert L.moptix_query_radiance_device(h, misaligned, 8, sp, None, len(SEEDS), 0, 0, C.c_void_p(out.data_ptr())) == K.ERR_INVALID
    assert L.moptix_query_radiance_device(h, C.c_void_p(rt.data_ptr()), 8, sp, None, len(SEEDS), 0, 0, C.c_void_p(out.data_ptr() + 8)) == K.ERR_INVALID
    assert L.moptix_query_radiance_device(h, C.c_void_p(rt.data_ptr()), 8, None, C.c_void_p(rt.data_ptr() + 2), 1, 0, 0, C.c_void_p(out.data_ptr())) == K.ERR_INVALID
    assert L.moptix_query_radiance_device(h, C.c_void_p(rt.data_ptr()), 8, sp, None, len(SEEDS), 0, 2, C.c_void_p(out.data_ptr())) == K.ERR_INVALID
    assert L.moptix_query_radiance_device(h, None, 0, None, None, 1, 0, 0, None) == K.MOPTIX_OK
    for bad in (dict(rays=rt[:, :7].contiguous()), dict(rays=rt.double()), dict(rays=rt[::2]), dict(rays=rt.cpu()), dict(rays=rt, states=np.zeros((len(rays), 1), np.uint32)),
                dict(rays=rays, states=np.zeros((3, 1), np.uint32)), dict(rays=rays, states=np.zeros((len(rays), 1), np.float32))):
        with pytest.raises(ValueError):
            ctx.query_radiance(bad["rays"], seeds=None if "states" in bad else SEEDS, states=bad.get("states"))
    with pytest.raises(ValueError):
        ctx.query_radiance(rays)
    with pytest.raises(ValueError):
        ctx.query_radiance(rays, seeds=SEEDS, states=np.zeros((len(rays), 1), np.uint32))


@pytest.mark.timeout(300)
def test_state_and_refit(ctx, coffee):
    hs, _ = coffee
    ctx.load(hs)
    rays = coffee_rays(n=1024, seed=6)
    fp, rows = moved_faces(hs, 0.02)
    ctx.update_faces(0, rows)
    with pytest.raises(M.MoptixError) as e:
        ctx.query_radiance(rays, seeds=SEEDS)
    assert e.value.code == K.ERR_STATE and "moptix_refit_accel" in str(e.value)
    ctx.refit_accel()
    sim = RefitSim(hs)
    sim.update(0, rows); sim.refit()
    want = radiancesim(sim._sim, rays, seeds=SEEDS)
    assert same_bits(ctx.query_radiance(rays, seeds=SEEDS), want)
    assert same_bits(want[:, 3], sim.query(rays)["t"])
    sim.close()
    fresh = M.Context(0)
    try:
        with pytest.raises(M.MoptixError) as e:
            fresh.query_radiance(rays, seeds=SEEDS)
        assert e.value.code == K.ERR_STATE
    finally:
        fresh.close()


@pytest.mark.timeout(300)
def test_a_radiance_query_leaves_the_context_as_it_was(ctx, coffee):
    hs, _ = coffee
    ctx.load(hs)
    seeds = M.launch_seeds(2)
    ctx.accum_clear(); ctx.render(seeds)
    ctx.aov_clear(); ctx.render_aovs(seeds[:1])
    dn = ctx.denoise(2)
    rays = coffee_rays(n=2048, seed=9)
    hits = ctx.query_rays(rays)
    accum, aovs = ctx.accum_read(), ctx.aov_read()
    launches, addr = ctx.kernel_time()[1], ctx.debug_buffer_addresses()
    fmt, variant = ctx.get_option("node_format_used"), ctx.get_option("kernel_variant_used")
    assert addr["query_overflow"] != 0 and launches > 0
    ctx.query_radiance(rays, seeds=SEEDS, clamp=True)
    assert same_bits(ctx.accum_read(), accum)
    after = ctx.aov_read()
    assert all(same_bits(after[k], aovs[k]) for k in aovs) and ctx.aov_samples() == 1
    out = np.empty_like(dn)
    ctx._chk(K.device_lib().moptix_denoise_read(ctx._h, out.ctypes.data_as(C.POINTER(C.c_float))))
    assert same_bits(out, dn)
    assert ctx.kernel_time()[1] == launches and ctx.debug_buffer_addresses() == addr
    assert ctx.get_option("node_format_used") == fmt and ctx.get_option("kernel_variant_used") == variant
    assert same_bits(ctx.query_rays(rays), hits)
