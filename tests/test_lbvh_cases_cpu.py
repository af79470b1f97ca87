"""The adversarial-geometry cases of lbvh_cases.py on the CPU mirror of the device's builder (tests/hostsim): every tree is a valid tree over
exactly its triangles, every box contains what lies below it, the mirror's walk finds what a loop over all triangles finds on every ray,
and every case is what it claims to be (the branch of the builder it is there for is taken).  tests/test_gpu_lbvh_cases.py asserts the
same of the device's trees and kernels, and that they are the mirror's word for word.

Not covered, on purpose: the kSahLevels = 40 cut-off after which the SAH builder splits in the middle.  A binned sweep takes about four
binades of a geometric progression off a node per level, so a 41st level needs a scene that spans about 2^160, where box areas overflow
float32: no finite input reaches it."""
import numpy as np
import pytest

from common import HostsimHandle, M, hostsim_bvh, hostsim_sah_levels, oracle_scene, tree_containment_errors, tree_containment_errors_exact
from aov_helpers import aovsim_render
from lbvh_cases import (BIG_FIRST, CASE_NAMES, LEAVES, BUILDERS, PLANE_AXIS, RENDER_CASES, case_faces, case_rays, case_scene, middle_split_levels,
                        tree_structure_errors)
from query_helpers import querysim

K_WIDE_TASKS, K_WIDE_COUNT = 1024, 2048        # csrc/lbvh.hip kWideTasks, kWideCount: a level takes the per-triangle form when nodes <= 1024 and largest > 2048
LDS_STACK = 32                                 # entries of a traversal stack that the kernels keep in LDS; deeper ones go to the spill columns


def mirror_tree(name, leaf, builder):
    """dict(nodes, tris, prim, root, depth, nodes64 or None) of the mirror's tree; nodes64 is None where the tree has no 64-byte form."""
    nodes, tris, prim, root, depth, n64 = hostsim_bvh(case_scene(name), leaf, builder, want_nodes64=True)
    return dict(nodes=nodes, tris=tris, prim=prim, root=root, depth=depth, nodes64=n64 if len(nodes) == 0 or n64.any() else None)


@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_mirror_tree_is_a_valid_tree(name, leaf, builder):
    t = mirror_tree(name, leaf, builder)
    n = len(case_faces(name))
    errors, depth = tree_structure_errors(t["nodes"], t["tris"], t["prim"], t["root"], leaf, n)
    assert errors == 0
    assert depth == t["depth"]
    assert (len(t["nodes"]) == 0) == (n <= leaf)
    assert tree_containment_errors(t["nodes"], t["tris"], t["root"] if len(t["nodes"]) else -1, t["nodes64"]) == 0
    # and with no slack at all, from the positions as the builder was handed them: the slack above is wider than all of `geometric`
    assert tree_containment_errors_exact(t["nodes"], t["tris"], t["root"] if len(t["nodes"]) else -1, case_faces(name), t["nodes64"]) == 0


@pytest.mark.parametrize("name", CASE_NAMES)
def test_mirror_walk_equals_brute_force(name):
    hs, rays = case_scene(name), case_rays(name)
    assert rays.shape == (2048, 8) and np.isfinite(rays).all()
    op, ot = oracle_scene(hs, brute_force_tris=True).closest_hits(rays)
    n_tri_hits = int((op >= hs.sizes.nSpheres + hs.sizes.nQuads).sum())
    print("%s: %d of %d rays hit a triangle" % (name, n_tri_hits, len(rays)))
    assert n_tri_hits >= 100 or name == "counts_1"
    sim = HostsimHandle(hs, 4, 1)
    for fmt in (64, 128):
        h = querysim(sim, rays, "closest", node_format=fmt)
        assert np.array_equal(h["prim"], op)
        assert np.array_equal(h["t"][op >= 0].view(np.uint32), ot[op >= 0].view(np.uint32))
        assert np.array_equal(querysim(sim, rays, "any", node_format=fmt), (op >= 0).astype(np.int32))
    if name == "duplicates":                                        # rule D5: a tie of all 100 goes to face 0
        first = hs.sizes.nSpheres + hs.sizes.nQuads
        assert set(op[op >= first].tolist()) == {first}
    if name in PLANE_AXIS:                                          # some rays lie in the plane, exactly
        a = PLANE_AXIS[name]
        assert ((rays[:, 3 + a] == 0) & (rays[:, a] == np.float32(0.0625))).sum() >= 50


def test_mixed_meets_a_large_node_in_the_workgroup_per_node_form():
    lv = hostsim_sah_levels(case_scene("mixed"))
    late = [i for i, (nodes, largest) in enumerate(lv) if nodes > K_WIDE_TASKS and largest > K_WIDE_COUNT]
    assert late
    assert any(nodes <= K_WIDE_TASKS and largest > K_WIDE_COUNT for nodes, largest in lv[:late[0]])
    assert len(case_faces("mixed")) < 7000


def test_geometric_is_deeper_than_the_lds_stack():
    for leaf, builder in ((1, 1), (4, 1)):
        assert 3 * mirror_tree("geometric", leaf, builder)["depth"] + 1 > LDS_STACK


def test_geometric_wide_has_no_64_byte_form():
    for leaf in LEAVES:
        for builder in BUILDERS:
            assert mirror_tree("geometric_wide", leaf, builder)["nodes64"] is None
            assert mirror_tree("geometric", leaf, builder)["nodes64"] is not None


@pytest.mark.parametrize("name", ["duplicates", "concentric"])
def test_coinciding_centroids_split_in_the_middle(name):
    n = len(case_faces(name))
    for leaf in LEAVES:
        lv = hostsim_sah_levels(case_scene(name), leaf, 1)
        assert lv[:, 0].tolist() == middle_split_levels(n)
    assert len(hostsim_sah_levels(case_scene(name), 4, 0)) == 0     # the table is the SAH builder's


@pytest.mark.parametrize("b,s", BIG_FIRST)
def test_big_first_forces_the_root_split(b, s):
    """pt_lbvh.h big_key_count, read off the order the triangles end in: the large triangles (faces 0 .. b-1) in front of all others."""
    n = b + s
    for leaf in LEAVES:
        for builder in BUILDERS:
            prim = mirror_tree("big_first_%d_%d" % (b, s), leaf, builder)["prim"]
            big = prim < b
            k = int(np.argmin(big)) if not big.all() else n         # length of the leading run of large triangles
            assert not big[k:].any()
            assert (k if 0 < k < n else 0) == (b if s and b else 0)
    if b and s:                                                     # the root's range is cut there
        lv = hostsim_sah_levels(case_scene("big_first_%d_%d" % (b, s)), 4, 1)
        assert lv[1, 1] == max(b, s)


@pytest.mark.parametrize("name", RENDER_CASES)
def test_rendered_cases_fill_a_quarter_of_the_coffee_view(name):
    hs = case_scene(name, 96, 54)
    a = aovsim_render(hs, M.launch_seeds(1))
    assert (a["primId"] >= hs.sizes.nSpheres + hs.sizes.nQuads).mean() >= 0.25
