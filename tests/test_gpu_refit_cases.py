"""The adversarial deformations of refit_cases.py through moptix_update_faces* and moptix_refit_accel on the MI355X (refitkernel.hip,
api_refit.hip), and through every kernel that walks the refitted tree.  The device's arrays, verdict on the 64-byte form and cost are the
CPU mirror's (tests/hostsim/refitsim.cpp); apart from the mirror, the arrays the device hands back contain every moved vertex with no
slack at all, are a tree over exactly these triangles, and cost what include/moptix.h defines; debug_trace and the ray queries find what
the oracle's loop over all triangles of the moved scene finds, on every ray; the other query families give their mirrors' bits and the
bits of their definitions on a scene that knows no tree and no refit; the schedulers render the same bits, within the arithmetic
contract of the oracle.  tests/test_refit_cases_cpu.py proves on the mirror that each pair is what it claims to be and that the
reference side of every condition here holds.

The trees: levels of one or two nodes by the dozen (geometric), levels wider than a workgroup of k_refit_level and node counts that are
no multiple of 256 (counts_2049, mixed), a tree whose every box is the scene box or one point (shuffle, collapse_point), a root that is
a leaf (strip_3)."""
import numpy as np
import pytest

import lbvh_cases
from common import HostsimHandle, M, MovedScene, oracle_scene, rmse, tree_containment_errors_exact
from box_helpers import box_sets, boxbrute, boxbrute_list, boxsim, boxsim_list, csr
from frustum_helpers import frustum_sets, frustumbrute, frustumbrute_list, frustumsim, frustumsim_list
from multihit_helpers import multibrute, multisim
from obb_helpers import obb_sets, obbbrute, obbbrute_list, obbsim, obbsim_list
from point_helpers import Geometry, point_sets, pointbrute, pointsim, shortened, with_max
from pointmulti_helpers import pointmultibrute, pointmultisim
from query_helpers import same_bits
from refit_cases import (DEFORMATIONS, GPU_RUNS, OFFSET_DIR, STRIP, base_faces, base_scene, explode, leaf_interior_range, moved_faces, moved_scene, pair_rays,
                         sah_cost, shrink)
from refit_helpers import RefitSim, displace, same_words
from sign_helpers import mesh_scene as sign_mesh_scene, sign_info, signbrute, signsim
from sweep_helpers import base_sweeps, sweepbrute, sweepsim, with_tmax_variants
from winding_helpers import INF, box_points, mesh_scene, rows, uv_sphere, winding_table, windingbrute, windingsim

pytestmark = pytest.mark.gpu

RMSE_TIGHT = 2e-6      # tests/test_gpu_parity.py: what the arithmetic contract delivers
DRAIN_DEFAULT = 64     # option drain_below as moptix_create leaves it
SEEDS = M.launch_seeds(2)
ARRAYS = ("nodes", "nodes64", "tris")
CONSUMER_CASES = ("counts_257", "degenerate", "mixed")
CONSUMER_DEFORMATIONS = ("shuffle", "explode", "to_points", "outlier_wide")

_mirrors, _hits, _fresh = {}, {}, {}


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    for name, v in (("leaf_size", 4), ("builder", 1), ("node_format", 0), ("kernel_variant", -1), ("drain_below", DRAIN_DEFAULT),
                    ("query_blocks_per_cu", 32)):
        gpu_ctx.set_option(name, v)


def mirror(case, deformation, leaf=4, builder=1):
    """(the mirror's handle after update and refit, its arrays as built, its arrays after the refit), made once and only read."""
    key = (case, deformation, leaf, builder)
    if key not in _mirrors:
        sim = RefitSim(base_scene(case), leaf, builder)
        built = sim.read()
        sim.update(0, moved_faces(case, deformation))
        _mirrors[key] = (sim, built, sim.refit().read())
    return _mirrors[key]


def brute_force_hits(case, deformation):
    """(prim, t) of the oracle's loop over all triangles of the moved scene on the pair's rays, computed once."""
    key = (case, deformation)
    if key not in _hits:
        _hits[key] = oracle_scene(moved_scene(case, deformation), brute_force_tris=True).closest_hits(pair_rays(case, deformation))
    return _hits[key]


def fresh(case, deformation):
    """The moved scene built from scratch by the mirror's builder: what the *brute helpers loop over.  It knows no refit."""
    key = (case, deformation)
    if key not in _fresh:
        _fresh[key] = HostsimHandle(moved_scene(case, deformation), 4)
    return _fresh[key]


def _read(c):
    nodes, tris, prim = c.debug_read_accel()
    try:
        n64 = c.debug_read_nodes64()
    except M.MoptixError:                       # this tree has no 64-byte form
        n64 = None
    return dict(nodes=nodes, tris=tris, prim=prim, nodes64=n64 if len(nodes) else None)      # a root that is a leaf has neither form


def _same_tree(a, b):
    return all((a[k] is None) == (b[k] is None) and (a[k] is None or same_words(a[k], b[k])) for k in ARRAYS)


def _torch_rows(rows_):
    import torch
    return torch.from_numpy(np.array(rows_, np.float32)).to("cuda:0")            # a copy: the pairs' arrays are read-only


def _close(a, b):
    """Relative 1e-9, the bound of test_gpu_refit.py; a tree without nodes costs exactly 0."""
    return a == b if b == 0 else abs(a - b) <= 1e-9 * abs(b)


def _update(ctx, first, rows_, device):
    ctx.update_faces(first, _torch_rows(rows_) if device else np.ascontiguousarray(rows_))


def _assert_traversal(ctx, case, deformation, sim):
    rays = pair_rays(case, deformation)
    op, ot = brute_force_hits(case, deformation)
    hit = op >= 0
    for fmt in (64, 128):
        ctx.set_option("node_format", fmt)
        t, prim = ctx.debug_trace(rays)
        assert np.array_equal(prim, op), (fmt, np.nonzero(prim != op)[0][:8])
        assert same_bits(t[hit], ot[hit]), fmt
        h = ctx.query_rays(rays)
        assert np.array_equal(h["prim"], op) and same_bits(h["t"][hit], ot[hit]), fmt
        anyone = ctx.query_rays(rays, "any")
        assert np.array_equal(anyone, hit.astype(np.int32)), fmt
        assert same_bits(h, sim.query(rays, "closest", node_format=fmt)) and same_bits(anyone, sim.query(rays, "any", node_format=fmt)), fmt


@pytest.mark.parametrize("case,deformation,leaf,builder", GPU_RUNS)
def test_refitted_device_tree(ctx, case, deformation, leaf, builder):
    hs, fp = base_scene(case), moved_faces(case, deformation)
    n = len(fp)
    device = GPU_RUNS.index((case, deformation, leaf, builder)) % 2 == 1      # the two update entries, alternating by pair
    ctx.set_option("leaf_size", leaf); ctx.set_option("builder", builder); ctx.set_option("node_format", 64)
    ctx.load(hs)
    built = _read(ctx)
    depth = ctx.accel_info().treeDepth
    _update(ctx, 0, fp, device)
    info = ctx.refit_accel()
    got = _read(ctx)
    sim, mbuilt, want = mirror(case, deformation, leaf, builder)
    # the arrays and the info are the mirror's
    assert np.array_equal(built["nodes"][:, :29], mbuilt["nodes"][:, :29]) and np.array_equal(built["tris"][:, :11], mbuilt["tris"][:, :11])
    assert np.array_equal(got["nodes"][:, :29], want["nodes"][:, :29])
    assert np.array_equal(got["tris"][:, :11], want["tris"][:, :11])
    assert (got["nodes64"] is None) == (want["nodes64"] is None)
    assert got["nodes64"] is None or np.array_equal(got["nodes64"], want["nodes64"])
    assert info["has64"] == (1 if want["nodes64"] is not None and len(want["nodes"]) else 0)
    print("%s %s leaf %d builder %d: has64 %d, sahCost / sahCostBuilt %.6g" % (
        case, deformation, leaf, builder, info["has64"], info["sahCost"] / info["sahCostBuilt"] if info["sahCostBuilt"] else float("nan")))
    assert _close(info["sahCost"], want["sahCost"]) and _close(info["sahCostBuilt"], want["sahCostBuilt"])
    # the cost is the definition's, from the device's own nodes
    assert _close(info["sahCost"], sah_cost(got["nodes"])) and _close(info["sahCostBuilt"], sah_cost(built["nodes"]))
    # containment with no slack and the structure, from the device's arrays alone
    root = want["rootRef"]
    assert tree_containment_errors_exact(got["nodes"], got["tris"], root, fp, got["nodes64"]) == 0
    errors, measured = lbvh_cases.tree_structure_errors(got["nodes"], got["tris"], got["prim"], root, leaf, n)
    assert errors == 0 and measured == depth == ctx.accel_info().treeDepth
    assert np.array_equal(got["prim"], built["prim"])
    # the walks against the loop over all triangles
    _assert_traversal(ctx, case, deformation, sim)


def test_traversal_at_leaf_1_on_a_capped_grid(ctx):
    case, deformation = "counts_257", "shuffle"
    ctx.set_option("leaf_size", 1); ctx.set_option("query_blocks_per_cu", 1)
    ctx.load(base_scene(case))
    _update(ctx, 0, moved_faces(case, deformation), True)
    ctx.refit_accel()
    _assert_traversal(ctx, case, deformation, mirror(case, deformation, 1, 1)[0])


# ---- every other consumer of a refitted tree ----
_sets = {}


def query_sets(case, deformation):
    """The query sets of the moved faces, from each family's own helper; made once."""
    key = (case, deformation)
    if key not in _sets:
        hs = moved_scene(case, deformation)
        geo = Geometry(hs)
        lo, hi = geo.box()
        f = fresh(case, deformation)
        q = with_max(point_sets(geo, lo, hi)[0])
        near = pointbrute(f, q)
        base = base_sweeps(geo, lo, hi)[0]
        first = sweepbrute(f, base)
        _sets[key] = dict(points=q, short=shortened(q, near["dist"], near["prim"]), boxes=box_sets(geo, lo, hi)[0], obbs=obb_sets(geo, lo, hi)[0],
                          frusta=frustum_sets(hs, geo, lo, hi)[0], sweeps=with_tmax_variants(base, first["t"], first["prim"]))
    return _sets[key]


def _refit(ctx, case, deformation, device=False):
    ctx.set_option("node_format", 64)
    ctx.load(base_scene(case))
    _update(ctx, 0, moved_faces(case, deformation), device)
    ctx.refit_accel()
    return mirror(case, deformation)[0]._sim, fresh(case, deformation)


CONSUMERS = [(c, d) for c in CONSUMER_CASES for d in CONSUMER_DEFORMATIONS]


@pytest.mark.parametrize("case,deformation", CONSUMERS)
def test_multi_hit_queries_on_the_refitted_tree(ctx, case, deformation):
    sim, brute = _refit(ctx, case, deformation)
    rays = pair_rays(case, deformation)
    for k, count_all in ((4, False), (64, True)):
        h, c = ctx.query_rays_multi(rays, k, count_all)
        mh, mc = multisim(sim, rays, k, count_all)
        assert same_bits(c, mc) and same_bits(h, mh), (k, count_all)
        bh, bc = multibrute(brute, rays, k, count_all)
        assert same_bits(c, bc) and same_bits(h, bh), (k, count_all)
    assert (c > 0).sum() >= len(rays) // 8


@pytest.mark.parametrize("case,deformation", CONSUMERS)
def test_point_queries_on_the_refitted_tree(ctx, case, deformation):
    sim, brute = _refit(ctx, case, deformation, device=True)
    s = query_sets(case, deformation)
    for name in ("points", "short"):
        for mode in ("closest", "any"):
            got = ctx.query_points(s[name], mode)
            assert same_bits(got, pointsim(sim, s[name], mode)), (name, mode)
            assert same_bits(got, pointbrute(brute, s[name], mode)), (name, mode)
    for q, k, count_all in ((s["points"], 4, False), (s["short"], 8, True)):
        h, c = ctx.query_points_multi(q, k, count_all)
        mh, mc = pointmultisim(sim, q, k, count_all)
        assert same_bits(c, mc) and same_bits(h, mh), (k, count_all)
        bh, bc = pointmultibrute(brute, q, k, count_all)
        assert same_bits(c, bc) and same_bits(h, bh), (k, count_all)


REGIONS = dict(boxes=("query_boxes", boxsim, boxsim_list, boxbrute, boxbrute_list), obbs=("query_obbs", obbsim, obbsim_list, obbbrute, obbbrute_list),
               frusta=("query_frusta", frustumsim, frustumsim_list, frustumbrute, frustumbrute_list))


@pytest.mark.parametrize("family", tuple(REGIONS))
@pytest.mark.parametrize("case,deformation", CONSUMERS)
def test_region_queries_on_the_refitted_tree(ctx, case, deformation, family):
    sim, brute = _refit(ctx, case, deformation)
    entry, walk, walk_list, loop, loop_list = REGIONS[family]
    b = query_sets(case, deformation)[family]
    query = getattr(ctx, entry)
    counts = query(b, "count")
    assert same_bits(counts, walk(sim, b, "count")) and same_bits(counts, loop(brute, b, "count"))
    anyone = query(b, "any")
    assert same_bits(anyone, walk(sim, b, "any")) and same_bits(anyone, loop(brute, b, "any"))
    prims, offsets = query(b, "list")
    assert same_bits(offsets, csr(counts))
    assert same_bits(prims, walk_list(sim, b, offsets)[0]) and same_bits(prims, loop_list(brute, b, offsets)[0])
    assert (counts > 0).any() and (counts == 0).any()


@pytest.mark.parametrize("case,deformation", CONSUMERS)
def test_sweep_queries_on_the_refitted_tree(ctx, case, deformation):
    sim, brute = _refit(ctx, case, deformation, device=True)
    s = query_sets(case, deformation)["sweeps"]
    for mode in ("closest", "any"):
        got = ctx.query_sweeps(s, mode)
        assert same_bits(got, sweepsim(sim, s, mode)), mode
        assert same_bits(got, sweepbrute(brute, s, mode)), mode
    hits = ctx.query_sweeps(s)["prim"] >= 0
    assert hits.any() and not hits.all()


# ---- winding numbers and signed distances: closed surfaces, shared vertices, deformations that are functions of the position ----
def strong_wave(fp0):
    """refit_helpers.displace at 30 % of the extent and a wavelength of about the mesh: folds the surface over itself, keeps vertices shared."""
    p = np.asarray(fp0, np.float32).reshape(-1, 3)
    ext = float((p.max(axis=0) - p.min(axis=0)).max())
    return displace(p, 0.3 * ext, k=np.float32(3.0)).reshape(-1, 9)


def far_offset(fp0):
    """refit_cases.offset's translation, a sixteenth of the largest power of two at which the distinct corners of the mesh stay distinct
    as well (refit_cases.offset asks that of the areas alone, and merges vertices near the sphere's poles)."""
    v = np.asarray(fp0, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(np.unique(v, axis=0))
    for k in range(40, -60, -1):
        if len(np.unique((v + 2.0 ** k * OFFSET_DIR).astype(np.float32), axis=0)) == n:
            return np.ascontiguousarray((v + 2.0 ** (k - 4) * OFFSET_DIR).astype(np.float32).reshape(-1, 9))
    raise AssertionError("no translation keeps the corners apart")


POSITIONAL = dict(explode=explode, shrink=shrink, offset=far_offset, strong_wave=strong_wave)
_closed = {}


def closed_mesh(name):
    if name not in _closed:
        _closed[name] = mesh_scene(uv_sphere()) if name == "uv_sphere" else sign_mesh_scene(name)
    return _closed[name]


def _moved_closed(name, deformation):
    hs = closed_mesh(name)
    fp = POSITIONAL[deformation](hs.face_arrays()[0])
    return hs, fp, MovedScene(hs, fp)


@pytest.mark.parametrize("deformation", tuple(POSITIONAL))
def test_winding_numbers_on_the_refitted_tree(ctx, deformation):
    hs, fp, moved = _moved_closed("uv_sphere", deformation)
    lo, hi = Geometry(moved).box()
    pts = box_points(lo, hi, 1000, 21)
    ctx.set_option("node_format", 64)
    ctx.load(hs)
    builds = ctx.winding_info()["tableBuilds"]
    ctx.query_winding(rows(pts[:16], 2.0))
    assert ctx.winding_info()["tableBuilds"] == builds + 1
    rs, brute = RefitSim(hs, 4), HostsimHandle(moved, 4)
    try:
        for k, device in enumerate((False, True)):                             # the same refit twice: the table is rebuilt once per refit
            _update(ctx, 0, fp, device)
            ctx.refit_accel()
            assert ctx.winding_info()["stale"] == 1 and ctx.winding_info()["tableBuilds"] == builds + 1 + k
            rs.update(0, fp); rs.refit()
            for beta in (INF, 2.0):
                assert same_bits(ctx.query_winding(rows(pts, beta)), windingsim(rs._sim, rows(pts, beta))), beta
            assert ctx.winding_info()["tableBuilds"] == builds + 2 + k and ctx.winding_info()["stale"] == 0
            assert same_words(ctx.winding_table_read(), winding_table(rs._sim))
        # the definition on the freshly built moved mesh: the same binary32 terms in another order into a binary64 sum, so the words
        # differ by the final rounding at most (test_winding_cpu.py test_walk_is_the_definition_and_the_binary64_sum)
        w, b = ctx.query_winding(rows(pts, INF)), windingbrute(brute, pts)
        assert np.isfinite(w).all() and np.abs(w - b).max() <= np.spacing(np.abs(b).max().astype(np.float32)) + 1e-12
        assert ctx.winding_info()["tableBuilds"] == builds + 3
        assert (w > 0.5).sum() >= 16 and (w < 0.5).sum() >= 16      # points on both sides (the folded wave leaves little inside)
    finally:
        rs.close(); brute.close()


@pytest.mark.parametrize("deformation", tuple(POSITIONAL))
def test_signed_distances_on_the_refitted_tree(ctx, deformation):
    hs, fp, moved = _moved_closed("torus", deformation)
    # shared vertices stay shared, and distinct ones distinct: the topology a fresh build of the moved mesh finds is the built one's
    assert len(np.unique(fp.reshape(-1, 3), axis=0)) == len(np.unique(hs.face_arrays()[0].reshape(-1, 3), axis=0)) == 288
    geo = Geometry(moved)
    lo, hi = geo.box()
    q = with_max(point_sets(geo, lo, hi)[0])
    ctx.set_option("node_format", 64)
    ctx.load(hs)
    assert ctx.sign_info()["tableBuilds"] == 0 and ctx.sign_info()["closed"] == 1
    ctx.query_points(q[:16], "signed")
    assert ctx.sign_info()["tableBuilds"] == 1
    rs, brute = RefitSim(hs, 4), HostsimHandle(moved, 4)
    try:
        assert sign_info(rs._sim)["closed"] == 1                                # the mirror takes its topology here, before the move, as the upload does
        for k, device in enumerate((True, False)):
            _update(ctx, 0, fp, device)
            ctx.refit_accel()
            assert ctx.sign_info()["tableBuilds"] == 1 + k
            rs.update(0, fp); rs.refit()
            got = ctx.query_points(q, "signed")
            assert ctx.sign_info()["tableBuilds"] == 2 + k
            assert same_bits(got, signsim(rs._sim, q))
            assert same_bits(ctx.query_points(q, "signed"), got) and ctx.sign_info()["tableBuilds"] == 2 + k
        # the signed loop over the freshly built moved mesh, whose topology comes from the moved positions: the walk's bytes are the
        # loop's (test_sign_cpu.py)
        assert sign_info(brute)["closed"] == 1
        assert same_bits(got, signbrute(brute, q))
        assert (got["dist"] < 0).sum() > 50 and (got["dist"] > 0).sum() > 50
    finally:
        rs.close(); brute.close()


# ---- chains and partial ranges ----
CHAIN_CASES = ("counts_257", "geometric", "mixed", "counts_2049", STRIP)


@pytest.mark.parametrize("case", CHAIN_CASES)
def test_a_chain_comes_back_to_the_built_tree(ctx, case):
    hs, fp0 = base_scene(case), base_faces(case)
    ctx.load(hs)
    built = _read(ctx)
    sim = RefitSim(hs, 4, 1)
    try:
        for k, d in enumerate(("shuffle", "collapse_point", "explode")):
            _update(ctx, 0, moved_faces(case, d), k % 2 == 0)
            info = ctx.refit_accel()
            sim.update(0, moved_faces(case, d))
            want = sim.refit().read()
            got = _read(ctx)
            assert _same_tree(got, want) and info["has64"] == (1 if want["nodes64"] is not None and len(want["nodes"]) else 0), d
            assert tree_containment_errors_exact(got["nodes"], got["tris"], want["rootRef"], moved_faces(case, d), got["nodes64"]) == 0
        had64 = got["nodes64"] is not None
        _update(ctx, 0, fp0, True)
        info = ctx.refit_accel()
        back = _read(ctx)
        if had64 == (built["nodes64"] is not None):
            assert _same_tree(back, built)
        else:                                   # geometric: exploded it is wider than the 64-byte nodes' grid reaches
            assert case == "geometric" and back["nodes64"] is None
        assert same_words(back["nodes"], built["nodes"]) and same_words(back["tris"], built["tris"])
        assert info["sahCost"] == info["sahCostBuilt"]
    finally:
        sim.close()


@pytest.mark.parametrize("case", CHAIN_CASES)
def test_a_chain_through_a_node_too_wide_loses_the_64_byte_form_until_a_build(ctx, case):
    hs, fp0 = base_scene(case), base_faces(case)
    ctx.set_option("node_format", 64)
    ctx.load(hs)
    built = _read(ctx)
    for k, d in enumerate(("shuffle", "outlier_wide", "collapse_point", "explode")):
        _update(ctx, 0, moved_faces(case, d), k % 2 == 1)
        info = ctx.refit_accel()
        assert d == "shuffle" or (info["has64"] == 0 and _read(ctx)["nodes64"] is None)
    for _ in range(2):                          # the original positions, then an identity refit
        _update(ctx, 0, fp0, False)
        info = ctx.refit_accel()
        back = _read(ctx)
        assert info["has64"] == 0 and same_words(back["nodes"], built["nodes"]) and same_words(back["tris"], built["tris"])
        if len(built["nodes"]):
            with pytest.raises(M.MoptixError):
                ctx.debug_read_nodes64()
    # node_format 64 is served by the 128-byte nodes: the walks of the built tree on the original positions
    rays = lbvh_cases.case_rays(case) if case != STRIP else pair_rays(case, "shuffle")
    op, ot = oracle_scene(hs, brute_force_tris=True).closest_hits(rays)
    hit = op >= 0
    t, prim = ctx.debug_trace(rays)
    assert np.array_equal(prim, op) and same_bits(t[hit], ot[hit])
    h = ctx.query_rays(rays)
    assert np.array_equal(h["prim"], op) and same_bits(h["t"][hit], ot[hit]) and hit.sum() >= 100
    assert np.array_equal(ctx.query_rays(rays, "any"), hit.astype(np.int32))
    ctx.build_accel(hs.accel)                   # a build brings the form back
    assert _same_tree(_read(ctx), built)
    assert ctx.refit_accel()["has64"] == (1 if built["nodes64"] is not None and len(built["nodes"]) else 0)


@pytest.mark.parametrize("deformation", ["shuffle", "explode", "outlier_wide"])
@pytest.mark.parametrize("case", ["counts_9", "counts_257", "geometric", "mixed", STRIP])
def test_an_update_of_a_range_is_the_update_of_the_whole_array(ctx, case, deformation):
    hs, fp0, fp = base_scene(case), base_faces(case), moved_faces(case, deformation)
    n = len(fp0)
    ctx.load(hs)
    built = _read(ctx)
    ranges = [[(0, 1)], [(n - 1, n)], [(0, 1), (n - 1, n)]]
    if len(built["nodes"]):
        a, b = leaf_interior_range(built, n)
        ranges += [[(a, b)], [(1, a), (b, n - 1)]]
    for k, parts in enumerate(ranges):
        whole = fp0.copy()
        ctx.load(hs)
        for a, b in parts:
            whole[a:b] = fp[a:b]
            _update(ctx, a, fp[a:b], k % 2 == 0)
        part_info = ctx.refit_accel()
        part = _read(ctx)
        ctx.load(hs)
        _update(ctx, 0, whole, k % 2 == 1)
        info = ctx.refit_accel()
        assert _same_tree(part, _read(ctx)), parts
        assert part_info["sahCost"] == info["sahCost"] and part_info["sahCostBuilt"] == info["sahCostBuilt"] and part_info["has64"] == info["has64"]
        sim = RefitSim(hs, 4, 1)
        sim.update(0, whole)
        assert _same_tree(part, sim.refit().read()), parts
        sim.close()


# ---- renders ----
@pytest.mark.parametrize("deformation", ["shuffle", "to_slivers"])
@pytest.mark.parametrize("name", lbvh_cases.RENDER_CASES)
def test_render_on_the_refitted_tree_across_schedulers(ctx, name, deformation):
    hs = lbvh_cases.case_scene(name, 96, 54)
    fp = DEFORMATIONS[deformation](lbvh_cases.case_faces(name))
    out = {}
    for k, (variant, fmt, db) in enumerate([(0, 0, DRAIN_DEFAULT), (3, 0, DRAIN_DEFAULT)] + [(4, f, d) for f in (64, 128) for d in (0, 64)]):
        ctx.set_option("kernel_variant", variant); ctx.set_option("node_format", fmt); ctx.set_option("drain_below", db)
        ctx.load(hs)
        _update(ctx, 0, fp, k % 2 == 1)
        ctx.refit_accel()
        ctx.accum_clear()
        st = ctx.render_counted(SEEDS)
        if ctx.get_option("kernel_variant_used") != variant:
            continue                            # a scene outside the packet kernel's limits: that leg is skipped, as test_render_across_schedulers does
        out[(variant, fmt, db)] = (ctx.accum_read(), st)
    a0, s0 = out[(0, 0, DRAIN_DEFAULT)]
    assert (3, 0, DRAIN_DEFAULT) in out
    for key, (a, st) in out.items():
        assert np.array_equal(a.view(np.uint32), a0.view(np.uint32)), key
        assert (st.rays, st.closestHits) == (s0.rays, s0.closestHits), key
    o, ost = oracle_scene(MovedScene(hs, fp)).render(SEEDS)
    assert rmse(a0 / len(SEEDS), o / len(SEEDS)) <= RMSE_TIGHT
    assert s0.rays == ost.rays
