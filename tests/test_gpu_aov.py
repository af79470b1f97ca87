"""First-hit AOVs on the MI355X (aovkernel.hip): bit for bit the CPU mirror of the kernel's code (tests/hostsim/aovsim.cpp), the oracle's closest hits
on the camera rays, and no effect on anything else the context holds."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import M, REPO, oracle_scene, textured_scene
from aov_helpers import AOV_NAMES, aovsim_render, camera_rays

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same(gpu, cpu):
    for n in AOV_NAMES:
        assert np.array_equal(_bits(gpu[n]), _bits(cpu[n])), n


def _load(ctx, hs, leaf_size=4, node_format=0):
    ctx.set_option("leaf_size", leaf_size)
    ctx.set_option("node_format", node_format)
    ctx.load(hs)
    ctx.aov_clear()


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0); gpu_ctx.set_partition(0, 1)
    gpu_ctx.aov_bind(None)


CASES = [("spheres", 64, 36, 1, 4, 64), ("cornell_quads", 64, 36, 7, 4, 64), ("file:coffee", 64, 36, 1, 4, 64), ("file:coffee", 64, 36, 7, 1, 128),
         ("file:coffee", 61, 37, 7, 4, 128), ("file:coffee", 61, 37, 1, 1, 64), ("textured", 64, 36, 7, 4, 64), ("textured", 61, 37, 1, 1, 128),
         ("random_spheres", 61, 37, 7, 4, 64)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind,w,h,nseeds,leaf,fmt", CASES)
def test_gpu_aovs_are_the_cpu_mirrors_bits(ctx, tmp_path, kind, w, h, nseeds, leaf, fmt):
    hs = textured_scene(tmp_path, w, h) if kind == "textured" else M.HostScene(kind, w, h)
    seeds = M.launch_seeds(nseeds, 5)
    _load(ctx, hs, leaf, fmt)
    ctx.render_aovs(seeds)
    assert ctx.aov_samples() == nseeds
    _assert_same(ctx.aov_read(), aovsim_render(hs, seeds, leaf_size=leaf, node_format=fmt))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["spheres", "cornell_quads", "file:coffee", "textured"])
def test_gpu_aov_ids_and_depth_are_the_oracles_closest_hits(ctx, tmp_path, kind):
    hs = textured_scene(tmp_path, 64, 36) if kind == "textured" else M.HostScene(kind, 64, 36)
    seed = int(M.launch_seeds(1)[0])
    _load(ctx, hs)
    ctx.render_aovs([seed])
    g = ctx.aov_read()
    prim, t = oracle_scene(hs).closest_hits(camera_rays(hs, seed))
    assert np.array_equal(g["primId"].reshape(-1), prim)
    hit = prim >= 0
    assert np.array_equal(_bits(g["depth"].reshape(-1)[hit]), _bits(t[hit]))


@pytest.mark.timeout(900)
def test_gpu_aov_ids_on_the_benchmark_frame_are_the_oracles(ctx):
    """Coffee at 1920x1080, 4 seeds: the ids (first seed) of every pixel are the oracle's closest hits on the camera rays.  The only
    difference allowed is the documented tree-dependent grazing hit (include/moptix.h, rule D5's exception), and each one found must be
    proved the way test_gpu_parity.py::test_the_known_grazing_hit_is_tree_dependent_and_nothing_else proves it: (1) the CPU build of the
    kernel's code on the same tree gives the GPU's id, (2) on the other tree (the 128-byte nodes) the GPU gives the oracle's, (3) the
    oracle's brute-force mode agrees with its tree."""
    hs = M.HostScene("file:coffee", 1920, 1080)
    seeds = M.launch_seeds(4)
    _load(ctx, hs)
    ctx.render_aovs(seeds)
    g = ctx.aov_read()
    rays = camera_rays(hs, int(seeds[0]))
    prim, _t = oracle_scene(hs).closest_hits(rays)
    gp = g["primId"].reshape(-1)
    bad = np.where(gp != prim)[0]
    assert g["hits"].max() == 4 and (prim >= 0).mean() > 0.5
    assert len(bad) <= 2, bad[:10]
    if len(bad):
        mirror = aovsim_render(hs, seeds[:1], node_format=64)["primId"].reshape(-1)
        assert np.array_equal(mirror[bad], gp[bad])                                                      # leg 1
        _load(ctx, hs, 4, 128)
        ctx.render_aovs(seeds[:1])
        assert np.array_equal(ctx.aov_read()["primId"].reshape(-1)[bad], prim[bad])                      # leg 2
        pb, _ = oracle_scene(hs, brute_force_tris=True).closest_hits(rays[bad])
        assert np.array_equal(pb, prim[bad])                                                             # leg 3


@pytest.mark.timeout(300)
def test_aovs_change_nothing_else(ctx):
    hs = M.HostScene("file:coffee", 160, 90)
    seeds = M.launch_seeds(4)
    ctx.set_option("kernel_variant", 4)
    try:
        frames = {}
        for with_aovs in (False, True):
            ctx.load(hs)                         # new build: same depth history and node-format verdict for both runs
            ctx.accum_clear()
            ctx.kernel_time(reset=True)
            ctx.render(seeds)
            fmt, launches = ctx.get_option("node_format_used"), ctx.kernel_time()[1]
            if with_aovs:
                ctx.aov_clear()
                ctx.render_aovs(seeds)
                assert ctx.get_option("node_format_used") == fmt and ctx.kernel_time()[1] == launches
                assert ctx.aov_read()["hits"].any()
            st = ctx.render_counted(seeds)
            frames[with_aovs] = (ctx.accum_read(), st.as_dict(), ctx.kernel_time()[1], ctx.get_option("node_format_used"))
        a, b = frames[False], frames[True]
        assert np.array_equal(_bits(a[0]), _bits(b[0]))
        assert a[2] == b[2] and a[3] == b[3]
        for k in ("samples", "primaryRays", "bounceRays", "shadowRays", "closestHits"):
            assert a[1][k] == b[1][k], k
    finally:
        ctx.set_option("kernel_variant", -1)


@pytest.mark.timeout(300)
def test_a_partitioned_context_still_renders_whole_frame_aovs(ctx):
    hs = M.HostScene("file:coffee", 61, 37)
    seeds = M.launch_seeds(3)
    _load(ctx, hs)
    ctx.render_aovs(seeds)
    whole = ctx.aov_read()
    ctx.set_partition(1, 3)
    ctx.aov_clear()
    ctx.render_aovs(seeds)
    _assert_same(ctx.aov_read(), whole)
    assert whole["hits"].any()


@pytest.mark.timeout(300)
def test_two_calls_give_the_bits_of_one_and_bound_tensors_the_bits_of_read(ctx):
    import torch
    hs = M.HostScene("file:coffee", 61, 37)
    seeds = M.launch_seeds(5, 3)
    _load(ctx, hs)
    ctx.render_aovs(seeds)
    whole = ctx.aov_read()
    ctx.aov_clear()
    assert ctx.aov_samples() == 0
    ctx.render_aovs(seeds[:2]); ctx.render_aovs(seeds[2:])
    assert ctx.aov_samples() == 5
    _assert_same(ctx.aov_read(), whole)
    dev = torch.device("cuda", 0)
    t = {n: torch.full((37, 61, ctx.AOV_CHANNELS[n]), 7, dtype=torch.int32 if n in ("primId", "matId") else torch.float32, device=dev) for n in AOV_NAMES}
    torch.cuda.synchronize()                 # the fills are on torch's stream, the library works on its own
    ctx.aov_bind(t)
    ctx.aov_clear()
    ctx.render_aovs(seeds)
    torch.cuda.synchronize()
    _assert_same({n: t[n].cpu().numpy() for n in AOV_NAMES}, whole)
    _assert_same(ctx.aov_read(), whole)


@pytest.mark.timeout(300)
def test_a_resize_clears_the_aovs(ctx):
    hs = M.HostScene("file:coffee", 64, 36)
    _load(ctx, hs)
    ctx.render_aovs(M.launch_seeds(2))
    assert ctx.aov_samples() == 2
    p = hs.params
    p.width, p.height = 48, 30
    ctx.set_params(p)
    assert ctx.aov_samples() == 0
    a = ctx.aov_read()
    assert a["albedo"].shape == (30, 48, 3) and not a["albedo"].any() and not a["hits"].any() and (a["primId"] == -1).all()


def test_aov_kernel_resources_are_pinned():
    """The AOV kernels' numbers as shipped (tools/kernel_resources.py): 120 VGPRs -- four waves per SIMD, the four 256-thread workgroups per
    CU the launch plans for, with 32 KB of LDS stack each -- no vector spills, no scratch; the scalar spills go to vector lanes."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from kernel_resources import kernel_resources
    res = {k: v for k, v in kernel_resources(os.path.join(REPO, "minimaloptix_amd", "lib", "libmoptix.so")).items() if "pt_aovkernel" in k}
    assert len(res) == 2, sorted(res)
    for k, r in res.items():
        sgpr_spill = 72 if "pt_aovkernelILb1E" in k else 68          # 64-byte / 128-byte nodes
        assert (r["vgpr_count"], r["vgpr_spill_count"], r["sgpr_spill_count"], r["group_segment_fixed_size"], r["private_segment_fixed_size"]) == \
            (120, 0, sgpr_spill, 32768, 0), (k, r)


@pytest.mark.timeout(300)
def test_cli_aov_writes_the_means(ctx, tmp_path):
    exe = os.path.join(REPO, "minimaloptix_amd", "lib", "moptix_render")
    p = subprocess.run([exe, "--scene", "spheres", "--spp", "3", "--aov", "--width", "96", "--height", "54", "--scenes", M.scenes_dir(),
                        "--outdir", str(tmp_path), "--out", "f"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    hs = M.HostScene("spheres", 96, 54, farg=0.5)          # the CLI's spheres scene: lens aperture 0.5 (scene_desc.h)
    _load(ctx, hs)
    ctx.render_aovs(M.launch_seeds(3))
    m = ctx.aov_means()
    depth = np.where(np.isinf(m["depth"]), np.float32(0), m["depth"])
    for name, want in (("albedo", m["albedo"]), ("normal", m["normal"]), ("depth", np.repeat(depth, 3, axis=2))):
        with open(tmp_path / ("f_%s.pfm" % name), "rb") as f:
            assert f.readline() == b"PF\n" and f.readline() == b"96 54\n" and f.readline() == b"-1.0\n"
            got = np.frombuffer(f.read(), np.float32).reshape(54, 96, 3)
        assert np.array_equal(_bits(got), _bits(want)), name
