"""The material cases (tests/material_cases.py) on the MI355X: every Disney term away from its default, at 0 and at 1, twelve materials
side by side in a wave, a Disney GLASS pane, a Lambertian panel among Disney meshes -- through moptix_render (per-lane, queue and packet
kernels; the packet kernel's slim, lean and general builds), moptix_query_radiance, "fast_shading" and the AOV render.  The device must
give the CPU mirror's bits (tests/hostsim), the oracle's image to RMSE 2e-6 and its ray counts.  tests/test_material_cases_cpu.py checks the
mirror and the oracle against each other, without a GPU.

96 x 54 frames, four launch seeds.  The lines that start with "material_cases:" are the measurements profiles/r25_material_cases.txt
records (pytest -s shows them)."""
import numpy as np
import pytest

import material_cases as MC
from aov_helpers import aovsim_render
from common import HostsimHandle, M, hostsim_render, oracle_scene, rmse
from packet_helpers import DRAIN_DEFAULT, FEAT_ALL, OPTION_DEFAULTS, bits as _bits, render_after_other_seeds as _render
from query_helpers import box_rays, same_bits
from radiance_helpers import radiancesim, seed_states, shadow_rule

pytestmark = pytest.mark.gpu

W, H = 96, 54
SEEDS = M.launch_seeds(4)
RMSE_TIGHT = 2e-6
COUNTERS = ("primaryRays", "bounceRays", "shadowRays", "closestHits")
RADIANCE_SEEDS = [5, 0x9e3779b9, 77, 12345]


@pytest.fixture
def ctx(gpu_ctx):
    """The session's context; every option these tests touch goes back to its default afterwards."""
    yield gpu_ctx
    gpu_ctx.set_partition(0, 1)
    for name, value in OPTION_DEFAULTS + (("fast_shading", 0),):
        gpu_ctx.set_option(name, value)


_refs = {}


def reference(name):
    """Per case, made once and only read: the scene, its mirror handle, the mirror's frame (bit-identical between its state machines and
    node formats: test_material_cases_cpu.py) and the oracle's frame and counts."""
    if name not in _refs:
        hs = MC.case_scene(name, W, H)
        sim = HostsimHandle(hs)
        mirror, _ = hostsim_render(sim, SEEDS, node_format=64, packet=1)
        o, ost = oracle_scene(hs).render(SEEDS)
        assert np.isfinite(mirror).all() and np.isfinite(o).all()
        _refs[name] = dict(hs=hs, sim=sim, mirror=mirror, oracle=o, ost=ost)
    return _refs[name]


# ---- a. renders ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [0, 3, 4])
@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_render_is_the_mirrors_bits_and_the_oracles_image(ctx, name, variant):
    ref = reference(name)
    ctx.set_option("kernel_variant", variant)
    ctx.load(ref["hs"])
    ctx.accum_clear()
    st = ctx.render_counted(SEEDS)
    counted = ctx.accum_read()
    assert ctx.get_option("kernel_variant_used") == variant
    plain, used = _render(ctx, SEEDS)
    assert used[0] == variant
    assert np.isfinite(counted).all() and np.isfinite(plain).all() and counted.max() > 0
    assert np.array_equal(_bits(plain), _bits(counted))
    assert np.array_equal(_bits(counted), _bits(ref["mirror"]))
    e = rmse(counted / len(SEEDS), ref["oracle"] / len(SEEDS))
    print("material_cases: gpu render %s, variant %d: RMSE against the oracle %.3g, uncounted build (variant, features, slim) %s" % (name, variant, e, used))
    assert e <= RMSE_TIGHT
    for f in COUNTERS:
        assert getattr(st, f) == getattr(ref["ost"], f), f


# ---- b. the packet kernel's builds ----------------------------------------------------------------------------------------------------------

SLIM, LEAN, GENERAL = (4, 0, 1), (4, 0, 0), (4, FEAT_ALL, 0)


@pytest.mark.parametrize("name", ["all", MC.TWELVE, MC.GLASS])
def test_packet_builds_give_the_per_lane_kernels_bits(ctx, name):
    """Slim (lean, no borrowed slots), lean (128 of the 576 slots empty from the start, so that every path of depth >= 1 borrows one) and
    general ("specialize" 0), on both node formats, with the drain kernel and without.  On the glass case once more under "shadow_rule" 0,
    where the slim build has no glass code and the lean one runs instead."""
    ref = reference(name)
    ctx.load(ref["hs"])
    lane, used = _render(ctx, SEEDS, kernel_variant=0)
    assert used == (0, FEAT_ALL, 0), used
    assert np.array_equal(_bits(lane), _bits(ref["mirror"]))
    ctx.set_option("kernel_variant", 4)
    ran = []
    for node_format in (64, 128):
        for drain_below in (0, DRAIN_DEFAULT):
            for want, options in ((SLIM, dict(specialize=1, aux_depth=0, slots_in_use=-1)), (LEAN, dict(specialize=1, aux_depth=1, slots_in_use=448)),
                                  (GENERAL, dict(specialize=0, aux_depth=0, slots_in_use=-1))):
                g, used = _render(ctx, SEEDS, node_format=node_format, drain_below=drain_below, **options)
                assert ctx.get_option("node_format_used") == node_format
                assert used == want, (node_format, drain_below, used)
                assert np.array_equal(_bits(g), _bits(lane)), (node_format, drain_below, used)
                ran.append(used)
    if name == MC.GLASS:
        sim0 = HostsimHandle(ref["hs"])
        shadow_rule(sim0, 0)
        mirror0, _ = hostsim_render(sim0, SEEDS, node_format=64, packet=1)
        sim0.close()
        ctx.set_option("shadow_rule", 0); ctx.set_option("node_format", 0)
        ctx.load(ref["hs"])
        lane0, used = _render(ctx, SEEDS, kernel_variant=0, specialize=1, aux_depth=0, drain_below=DRAIN_DEFAULT)
        assert used == (0, FEAT_ALL, 0), used
        assert np.isfinite(mirror0).all() and np.array_equal(_bits(lane0), _bits(mirror0))
        g, used = _render(ctx, SEEDS, kernel_variant=4)
        assert used == LEAN, used
        assert np.array_equal(_bits(g), _bits(lane0))
        ran.append(used)
    print("material_cases: packet builds %s: slim %d, lean %d, general %d launches, all the per-lane kernel's bits" % (
        name, ran.count(SLIM), ran.count(LEAN), ran.count(GENERAL)))
    assert {SLIM, LEAN, GENERAL} <= set(ran)


@pytest.mark.parametrize("node_format", [64, 128])
def test_a_lambertian_panel_keeps_the_general_build_on_the_same_sweep(ctx, node_format):
    ref = reference(MC.LAMBERTIAN)
    ctx.load(ref["hs"])
    g, used = _render(ctx, SEEDS, kernel_variant=4, node_format=node_format, aux_depth=0)
    assert used == GENERAL and ctx.get_option("kernel_features_used") == 15, used
    assert np.array_equal(_bits(g), _bits(ref["mirror"]))
    lane, used = _render(ctx, SEEDS, kernel_variant=0)
    assert used[0] == 0 and np.array_equal(_bits(g), _bits(lane))
    flat = reference("all")["mirror"]
    assert not np.array_equal(_bits(g), _bits(flat))                                          # the panel is in the frame


# ---- c. radiance queries --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("name", MC.GRAZING_CASES + (MC.TWELVE, MC.GLASS, MC.LAMBERTIAN))
def test_radiance_queries_are_the_mirrors_bits(ctx, name, fmt):
    """2048 rays from inside the scene's box and the 5 x 512 grazing rays towards the floor, four samples each: seeds mode and states mode,
    clamped and not.  The mirror's values are finite before any are compared."""
    ref = reference(name)
    hs, sim = ref["hs"], ref["sim"]
    rays = np.ascontiguousarray(np.concatenate([box_rays(hs)] + list(MC.grazing_sets(hs).values())))
    ctx.set_option("node_format", fmt)
    ctx.load(hs)
    shadow_rule(sim, 1)
    base = 1000
    states = seed_states(len(rays), RADIANCE_SEEDS, base)
    for clamp in (False, True):
        want = radiancesim(sim, rays, states=states, clamp=clamp, node_format=fmt)
        assert np.isfinite(want).all() and want[:, :3].any()
        assert same_bits(ctx.query_radiance(rays, seeds=RADIANCE_SEEDS, index_base=base, clamp=clamp), want), ("seeds", clamp)
        assert same_bits(ctx.query_radiance(rays, states=states, clamp=clamp), want), ("states", clamp)
    print("material_cases: radiance query %s, %d-byte nodes: %d rays x %d samples, largest unclamped radiance %.3g, the mirror's bits" % (
        name, fmt, len(rays), len(RADIANCE_SEEDS), float(radiancesim(sim, rays, states=states, node_format=fmt)[:, :3].max())))


# ---- d. fast shading --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [3, 4])
@pytest.mark.parametrize("name", ["all", "rough0", "metal1"])
def test_fast_shading_keeps_the_paths(ctx, name, variant):
    """The hardware's rcp / sqrt / rsq inside disney_pdf and disney_eval only, on the queue and packet kernels (the per-lane kernel has no
    such build): the same rays (every ray counter is exact mode's), finite values, not the same bits.  How far the frame moves is printed
    and recorded (2.4e-8 at the most, on metal1) and held to the 1e-5 that tests/test_gpu_configs.py holds coffee to, which the measured
    values are well inside.  The traversal counters are not compared: the drain kernel takes a launch's last paths over when the
    packet kernel gets to them, and culls its shared frontier in the order the entries are popped."""
    ref = reference(name)
    ctx.set_option("kernel_variant", variant)
    ctx.load(ref["hs"])
    ctx.accum_clear()
    st0 = ctx.render_counted(SEEDS)
    exact = ctx.accum_read()
    assert np.array_equal(_bits(exact), _bits(ref["mirror"]))
    ctx.set_option("fast_shading", 1)
    ctx.accum_clear()
    st1 = ctx.render_counted(SEEDS)
    fast = ctx.accum_read()
    assert ctx.get_option("kernel_variant_used") == variant
    for f in COUNTERS + ("samples",):
        assert getattr(st0, f) == getattr(st1, f), f
    assert np.isfinite(fast).all() and fast.max() > 0
    assert not np.array_equal(_bits(fast), _bits(exact))                                      # the option reached the kernel
    print("material_cases: fast_shading %s, variant %d: RMSE fast against exact %.3g, largest difference %.3g, %d of %d values differ" % (
        name, variant, rmse(fast / len(SEEDS), exact / len(SEEDS)), float(np.abs(fast - exact).max() / len(SEEDS)),
        int((_bits(fast) != _bits(exact)).sum()), fast.size))
    assert rmse(fast / len(SEEDS), exact / len(SEEDS)) < 1e-5


# ---- e. AOVs -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["all", MC.TWELVE])
def test_albedo_and_material_id_are_the_mirrors(ctx, name):
    ref = reference(name)
    ctx.load(ref["hs"])
    ctx.aov_clear()
    ctx.render_aovs(SEEDS)
    got, want = ctx.aov_read(), aovsim_render(ref["sim"], SEEDS)
    assert np.isfinite(want["albedo"]).all() and want["albedo"].any()
    assert same_bits(got["albedo"], want["albedo"]) and same_bits(got["matId"], want["matId"])
    assert len(np.unique(want["matId"])) >= (12 if name == MC.TWELVE else 2)
