"""The adversarial-geometry cases of lbvh_cases.py on the MI355X: the device builder (csrc/lbvh.hip) gives the mirror's tree word for word
and a valid one by two checks that share no code with it; debug_trace and the ray queries find what a loop over all triangles finds, on
every ray; the three schedulers, both node formats and the drain kernel render the same bits; the AOV pass, the radiance queries and an
identity refit reproduce what they should.  tests/test_lbvh_cases_cpu.py proves on the mirror that each case is what it claims to be.

Not covered, on purpose: the kSahLevels = 40 cut-off (see tests/test_lbvh_cases_cpu.py: no finite input reaches it)."""
import numpy as np
import pytest

from common import HostsimHandle, M, hostsim_bvh, oracle_scene, rmse, tree_containment_errors, tree_containment_errors_exact
from aov_helpers import AOV_NAMES, aovsim_render
from lbvh_cases import BUILDERS, CASE_NAMES, LEAVES, RENDER_CASES, case_faces, case_rays, case_scene, tree_structure_errors
from query_helpers import querysim, same_bits
from radiance_helpers import camera_sum
from refit_helpers import same_words

pytestmark = pytest.mark.gpu

RMSE_TIGHT = 2e-6      # tests/test_gpu_parity.py: what the arithmetic contract delivers
DRAIN_DEFAULT = 64     # option drain_below as moptix_create leaves it
SEEDS = M.launch_seeds(2)

_hits = {}


def brute_force_hits(name):
    """(prim, t) of the oracle's loop over all triangles on the case's rays, computed once."""
    if name not in _hits:
        _hits[name] = oracle_scene(case_scene(name), brute_force_tris=True).closest_hits(case_rays(name))
    return _hits[name]


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    for name, v in (("leaf_size", 4), ("builder", 1), ("node_format", 0), ("kernel_variant", -1), ("drain_below", DRAIN_DEFAULT),
                    ("query_blocks_per_cu", 32)):
        gpu_ctx.set_option(name, v)


def _read(c):
    nodes, tris, prim = c.debug_read_accel()
    try:
        n64 = c.debug_read_nodes64()
    except M.MoptixError:                       # this tree has no 64-byte form
        n64 = None
    return nodes, tris, prim, n64


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_tree_is_the_mirrors_and_valid(gpu_ctx, name, leaf, builder):
    hs, n = case_scene(name), len(case_faces(name))
    gpu_ctx.set_option("leaf_size", leaf); gpu_ctx.set_option("builder", builder)
    try:
        gpu_ctx.load(hs)
        nodes, tris, prim, n64 = _read(gpu_ctx)
        info = gpu_ctx.accel_info()
    finally:
        gpu_ctx.set_option("builder", 1); gpu_ctx.set_option("leaf_size", 4)
    hn, ht, hp, root, depth, h64 = hostsim_bvh(hs, leaf, builder, want_nodes64=True)
    assert info.nNodes == len(hn) and info.treeDepth == depth
    assert np.array_equal(prim, hp)
    assert np.array_equal(tris[:, :11], ht[:, :11])
    assert np.array_equal(nodes[:, :29], hn[:, :29])
    if len(hn) == 0 or h64.any():
        assert n64 is not None and np.array_equal(n64, h64)
    else:
        assert n64 is None                      # debug_read_nodes64 raises exactly where the mirror has no 64-byte form
    errors, measured = tree_structure_errors(nodes, tris, prim, root, leaf, n)
    assert errors == 0 and measured == info.treeDepth
    assert tree_containment_errors(nodes, tris, root if len(nodes) else -1, n64) == 0
    assert tree_containment_errors_exact(nodes, tris, root if len(nodes) else -1, case_faces(name), n64) == 0      # no slack, the positions as handed in


def _assert_traversal(ctx, name, sim):
    rays = case_rays(name)
    op, ot = brute_force_hits(name)
    hit = op >= 0
    t, prim = ctx.debug_trace(rays)
    assert np.array_equal(prim, op) and same_bits(t[hit], ot[hit])
    h = ctx.query_rays(rays)
    assert np.array_equal(h["prim"], op) and same_bits(h["t"][hit], ot[hit])
    assert np.array_equal(ctx.query_rays(rays, "any"), hit.astype(np.int32))
    assert same_bits(h, querysim(sim, rays, "closest", node_format=64))      # 64: the 64-byte nodes where the tree has them, on both sides
    assert same_bits(ctx.query_rays(rays, "any"), querysim(sim, rays, "any", node_format=64))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_traversal_equals_brute_force(ctx, name):
    hs = case_scene(name)
    ctx.set_option("node_format", 64)           # the queries walk the 64-byte nodes where the tree has them, as querysim's default
    ctx.load(hs)
    sim = HostsimHandle(hs, 4, 1)
    _assert_traversal(ctx, name, sim)
    sim.close()


@pytest.mark.parametrize("name", ["geometric", "duplicates", "mixed"])
def test_traversal_equals_brute_force_at_leaf_1_on_a_capped_grid(ctx, name):
    hs = case_scene(name)
    ctx.set_option("leaf_size", 1); ctx.set_option("node_format", 64); ctx.set_option("query_blocks_per_cu", 1)
    ctx.load(hs)
    sim = HostsimHandle(hs, 1, 1)
    _assert_traversal(ctx, name, sim)
    sim.close()


@pytest.mark.parametrize("name", RENDER_CASES)
def test_render_across_schedulers(ctx, name):
    hs = case_scene(name, 96, 54)
    out = {}
    for variant, fmt, db in [(0, 0, DRAIN_DEFAULT), (3, 0, DRAIN_DEFAULT)] + [(4, f, d) for f in (64, 128) for d in (0, 64)]:
        ctx.set_option("kernel_variant", variant); ctx.set_option("node_format", fmt); ctx.set_option("drain_below", db)
        ctx.load(hs); ctx.accum_clear()
        st = ctx.render_counted(SEEDS)
        if ctx.get_option("kernel_variant_used") != variant:
            continue                            # a scene outside the packet kernel's limits: that leg is skipped, as test_drain_kernel_changes_nothing does
        out[(variant, fmt, db)] = (ctx.accum_read(), st)
    a0, s0 = out[(0, 0, DRAIN_DEFAULT)]
    assert (3, 0, DRAIN_DEFAULT) in out
    for key, (a, st) in out.items():
        assert np.array_equal(a.view(np.uint32), a0.view(np.uint32)), key
        assert (st.rays, st.closestHits) == (s0.rays, s0.closestHits), key
    o, ost = oracle_scene(hs).render(SEEDS)
    assert rmse(a0 / len(SEEDS), o / len(SEEDS)) <= RMSE_TIGHT
    assert s0.rays == ost.rays


@pytest.mark.parametrize("name", RENDER_CASES)
def test_aovs_are_the_mirrors_bits(ctx, name):
    hs = case_scene(name, 96, 54)
    ctx.set_option("node_format", 64)
    ctx.load(hs); ctx.aov_clear()
    ctx.render_aovs(SEEDS)
    g, want = ctx.aov_read(), aovsim_render(hs, SEEDS, node_format=64)
    for n in AOV_NAMES:
        assert same_bits(g[n], want[n]), n


def test_radiance_of_the_camera_rays_is_the_rendered_frame_on_geometric(ctx):
    hs = case_scene("geometric", 96, 54)
    ctx.load(hs)
    assert 3 * ctx.accel_info().treeDepth + 1 > 32      # deeper than the LDS part of the stack: the spill columns are in use
    ctx.accum_clear(); ctx.render(SEEDS)
    want = ctx.accum_read()
    got = camera_sum(lambda rays, states: ctx.query_radiance(rays, states=states, clamp=True), hs, SEEDS)
    assert want.any() and same_bits(got, want)


@pytest.mark.parametrize("name", RENDER_CASES)
def test_identity_refit_reproduces_the_built_tree(ctx, name):
    hs = case_scene(name)
    ctx.load(hs)
    built = _read(ctx)
    ctx.update_faces(0, case_faces(name))
    info = ctx.refit_accel()
    after = _read(ctx)
    for a, b in zip(built, after):
        assert (a is None) == (b is None) and (a is None or same_words(a, b))
    assert info["sahCost"] == info["sahCostBuilt"] > 0
