"""The adversarial deformations of refit_cases.py on the CPU mirror of the refit (tests/hostsim/refitsim.cpp: pt_refit.h compiled for the host):
every pair is what it claims to be and its ray set meets triangles; the refitted tree keeps the built topology, contains every moved vertex
with no slack at all in both node forms, and its walk finds what a loop over all triangles finds; the cost is the one include/moptix.h
defines; chains of deformations come back to the built tree word for word; an update of a face range is the update of the whole array.
tests/test_gpu_refit_cases.py asserts the same of the device's arrays and kernels, and that they are the mirror's word for word."""
import numpy as np
import pytest

from common import oracle_scene, tree_containment_errors, tree_containment_errors_exact
from refit_cases import (BASE_CASES, CPU_PAIRS, DEFORMATION_NAMES, HIT_SHARE, N_RAYS, SLAB_REACH, STRIP, areas, base_faces, base_scene,
                         leaf_interior_range, moved_faces, moved_scene, offset_magnitude, pair_rays, sah_cost, shrink_factor)
from refit_helpers import RefitSim, same_words

ARRAYS = ("nodes", "nodes64", "tris")
RUNS = [(c, d, 4) for c, d in CPU_PAIRS] + [("counts_257", d, leaf) for d in DEFORMATION_NAMES for leaf in (1, 8)]
# The pairs whose ray set may hit fewer than one ray in HIT_SHARE, with the triangle hits of the loop over all triangles: the deformation
# leaves every triangle with zero area, and nothing else excuses a pair.  (collapse_point by construction.  The triangles of the two
# geometric chains have p0 and p1 apart on x only and p2 on their bisector: flatten_x joins p0 and p1, flatten_y puts the three on a line.)
ZERO_AREA_PAIRS = tuple([((c, "collapse_point"), 0) for c in BASE_CASES] +
                        [((c, d), 0) for c in ("geometric", "geometric_wide") for d in ("flatten_x", "flatten_y")])

_refitted, _hits = {}, {}


def refitted(case, deformation, leaf):
    """(the mirror's handle after update and refit, its arrays as built, its arrays after the refit), made once and only read."""
    key = (case, deformation, leaf)
    if key not in _refitted:
        sim = RefitSim(base_scene(case), leaf, 1)
        built = sim.read()
        sim.update(0, moved_faces(case, deformation))
        _refitted[key] = (sim, built, sim.refit().read())
    return _refitted[key]


def brute_force_hits(case, deformation):
    """(prim, t) of the oracle's loop over all triangles of the moved scene, which knows no tree and no refit; computed once."""
    key = (case, deformation)
    if key not in _hits:
        _hits[key] = oracle_scene(moved_scene(case, deformation), brute_force_tris=True).closest_hits(pair_rays(case, deformation))
    return _hits[key]


def triangle_hits(case, deformation):
    hs = base_scene(case)
    return int((brute_force_hits(case, deformation)[0] >= hs.sizes.nSpheres + hs.sizes.nQuads).sum())


def _ratio(t):
    return t["sahCost"] / t["sahCostBuilt"]


def _explode_bound(got, fp0, fp):
    """How far sahCost / sahCostBuilt may be from 1 after a scaling by s about a point, from the number formats alone.  A bound of a
    refitted box is pad(binary32(c + (p - c) s)) against s x pad(p) + const before: the rounding of the position moves it by 2^-24 |v'|
    at most, and the relative part of the padding (pt_lbvh.h pad_lo: 1e-6 |v|) depends on where the origin is, by 1e-6 (|v'| + s |v|) at
    most; the absolute part scales with the scene, up to a rounding that the 2^-24 below covers twice over.  With P the largest
    |coordinate| on either side, every bound is within d = 2.2e-6 P of its scaled place and every extent within 2 d, so a half area
    exey + eyez + ezex moves by at most 4 d (ex + ey + ez) + 12 d^2.  The cost is a weighted sum of half areas over the root's: its
    relative change is at most that of the sum plus that of the root's, to first order; the factor 1.01 pays for the second."""
    s = 1e6
    P = max(float(np.abs(fp).max()), s * float(np.abs(fp0).max()))
    d = (2.0 ** -23 + 2e-6) * P
    nodes = got["nodes"]
    box = nodes.view(np.float32)[:, 0:24].reshape(-1, 6, 4).astype(np.float64)
    refs = nodes[:, 24:28].view(np.int32).astype(np.int64)
    used = refs != 0x7ffffffe
    e = np.moveaxis(box[:, 3:6] - box[:, 0:3], 1, 2)                               # [m, child, axis]
    area = e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0]
    w = np.where(refs < 0, ((~refs) & 7) + 1, 1).astype(np.float64)
    moved = 4.0 * d * e.sum(axis=2) + 12.0 * d * d
    lo = np.moveaxis(box[0, 0:3], 0, 1)[used[0]].min(axis=0); hi = np.moveaxis(box[0, 3:6], 0, 1)[used[0]].max(axis=0)
    re = hi - lo
    root = re[0] * re[1] + re[1] * re[2] + re[2] * re[0]
    return 1.01 * (float((moved * w)[used].sum()) / float((area * w)[used].sum()) + (4.0 * d * re.sum() + 12.0 * d * d) / root)


@pytest.mark.parametrize("case,deformation", CPU_PAIRS)
def test_each_pair_is_what_it_claims(case, deformation):
    fp0, fp = base_faces(case), moved_faces(case, deformation)
    _, built, got = refitted(case, deformation, 4)
    has_tree = len(built["nodes"]) > 0
    assert has_tree == (case != STRIP)
    if deformation == "outlier_wide":
        assert got["nodes64"] is None                                          # also where the built tree had the form
    elif deformation == "outlier":
        assert (got["nodes64"] is None) == (built["nodes64"] is None)          # 1e9 is within the grid's reach: what was there survives
        assert case == "geometric_wide" or not has_tree or got["nodes64"] is not None
    elif deformation == "collapse_point":
        assert not areas(fp).any() and len(np.unique(fp)) <= 3
    elif deformation in ("shuffle", "reverse", "swap_halves"):
        assert same_words(np.sort(fp.view(np.uint32), axis=0), np.sort(fp0.view(np.uint32), axis=0))      # the same faces in another order
        if case == "duplicates":                                               # one triangle 100 times: any order is the same positions
            assert same_words(fp, fp0) and got["sahCost"] == got["sahCostBuilt"]
        elif has_tree:
            assert _ratio(got) > 1.0
    elif deformation == "explode":
        if has_tree:
            bound = _explode_bound(got, fp0, fp)
            print("%s: sahCost / sahCostBuilt - 1 = %.3g, bound %.3g" % (case, _ratio(got) - 1.0, bound))
            assert bound < 0.05 and abs(_ratio(got) - 1.0) <= bound
    elif deformation == "shrink":
        assert shrink_factor(fp0) == (1e-5 if case == "mixed" else 1e-6)
    elif deformation in ("to_points", "to_slivers"):
        third = np.arange(len(fp)) % 3 == 0
        assert not areas(fp)[third].any() and same_words(fp[~third], fp0[~third])
        assert same_words(fp[third, 3:6], fp[third, 6:9]) and same_words(fp[third, 0:3], fp[third, 3:6]) == (deformation == "to_points")
    elif deformation.startswith("flatten"):
        axis = "xyz".index(deformation[-1])
        assert len(np.unique(fp.reshape(-1, 3)[:, axis])) == 1
    elif deformation == "offset":
        m = offset_magnitude(fp0)
        assert (areas(fp) > 0).sum() == (areas(fp0) > 0).sum() and not same_words(fp, fp0)
        smallest = np.sqrt(areas(fp0)[areas(fp0) > 0].min())                   # far from the origin for the size of its smallest triangle
        assert m >= 1000.0 * smallest
    if not has_tree:
        assert got["sahCost"] == 0.0 and got["sahCostBuilt"] == 0.0
    # beyond the reach of the slab test for axis-parallel rays (refit_cases.rays_of): this pair and no other
    assert (float(np.abs(fp).max()) >= SLAB_REACH) == ((case, deformation) == ("geometric_wide", "explode"))


@pytest.mark.parametrize("case,deformation", CPU_PAIRS)
def test_the_ray_set_meets_triangles(case, deformation):
    rays = pair_rays(case, deformation)
    assert rays.shape == (N_RAYS, 8) and np.isfinite(rays).all()
    if float(np.abs(moved_faces(case, deformation)).max()) < SLAB_REACH:
        assert ((rays[:, 3:6] == 0).sum(axis=1) == 2).sum() == 3 * N_RAYS // 16      # exact zeros in the direction
    n = triangle_hits(case, deformation)
    print("%s %s: %d of %d rays hit a triangle" % (case, deformation, n, N_RAYS))
    exempt = dict(ZERO_AREA_PAIRS)
    if (case, deformation) in exempt:
        assert not areas(moved_faces(case, deformation)).any() and n == exempt[(case, deformation)]
    else:
        assert HIT_SHARE * n >= N_RAYS


def test_the_exempt_pairs_are_pairs():
    assert len(dict(ZERO_AREA_PAIRS)) == len(ZERO_AREA_PAIRS) and set(dict(ZERO_AREA_PAIRS)) <= set(CPU_PAIRS)


@pytest.mark.parametrize("case,deformation,leaf", RUNS)
def test_the_refitted_tree_is_sound(case, deformation, leaf):
    fp = moved_faces(case, deformation)
    sim, built, got = refitted(case, deformation, leaf)
    # the moved vertices are inside every box above them, in both forms, with no slack
    assert tree_containment_errors_exact(got["nodes"], got["tris"], got["rootRef"], fp, got["nodes64"]) == 0
    assert tree_containment_errors_exact(got["nodes"], got["tris"], got["rootRef"], fp) == 0
    # the topology and the order of the records are the built tree's
    assert got["rootRef"] == built["rootRef"] and len(got["nodes"]) == len(built["nodes"])
    assert same_words(got["nodes"][:, 24:29], built["nodes"][:, 24:29])
    assert same_words(got["tris"][:, [3, 7, 11]], built["tris"][:, [3, 7, 11]])
    if got["nodes64"] is not None:
        assert same_words(got["nodes64"][:, 12:16], built["nodes64"][:, 12:16])
    # the walk finds what the loop over all triangles finds
    rays = pair_rays(case, deformation)
    op, ot = brute_force_hits(case, deformation)
    hit = op >= 0
    for fmt in (64, 128):
        h = sim.query(rays, "closest", node_format=fmt)
        assert np.array_equal(h["prim"], op), (fmt, np.nonzero(h["prim"] != op)[0][:8])
        assert np.array_equal(h["t"][hit].view(np.uint32), ot[hit].view(np.uint32)), fmt
        assert np.array_equal(sim.query(rays, "any", node_format=fmt), hit.astype(np.int32)), fmt


@pytest.mark.parametrize("case,deformation,leaf", RUNS)
def test_the_cost_is_the_definitions(case, deformation, leaf):
    _, built, got = refitted(case, deformation, leaf)
    for tree, value in ((got, got["sahCost"]), (built, got["sahCostBuilt"]), (built, built["sahCost"])):
        want = sah_cost(tree["nodes"])
        assert abs(value - want) <= 1e-9 * abs(want), (value, want)
        assert np.isfinite(value) and (value > 0) == (len(tree["nodes"]) > 0)


def test_the_exact_check_sees_what_the_slack_hides():
    """One bound of one leaf box of `geometric` pulled one unit in the last place inside its triangles (1e-15 of a 1e-8 triangle):
    tree_containment_errors allows 1e-6 and sees nothing, the exact check counts the child; the 64-byte form, left alone, stays sound."""
    fp = base_faces("geometric")
    _, built, _ = refitted("geometric", "shuffle", 4)
    nodes = built["nodes"].copy()
    prim = built["tris"][:, 7].view(np.int32)
    slot = int(np.nonzero(prim == 0)[0][0])                                    # the smallest triangle
    refs = nodes[:, 24:28].view(np.int32)
    n, k = next((n, k) for n in range(len(nodes)) for k in range(4)
                if refs[n, k] < 0 and refs[n, k] != 0x7ffffffe and (~refs[n, k]) >> 3 <= slot <= ((~refs[n, k]) >> 3) + ((~refs[n, k]) & 7))
    first, cnt = (~int(refs[n, k])) >> 3, ((~int(refs[n, k])) & 7) + 1
    top = fp[prim[first:first + cnt]].reshape(-1, 3)[:, 0].max()
    assert tree_containment_errors_exact(nodes, built["tris"], built["rootRef"], fp, built["nodes64"]) == 0
    nodes.view(np.float32)[n, 12 + k] = np.nextafter(top, np.float32(-np.inf))      # hix of child k
    assert tree_containment_errors(nodes, built["tris"], built["rootRef"], built["nodes64"]) == 0
    assert tree_containment_errors_exact(nodes, built["tris"], built["rootRef"], fp, built["nodes64"]) == 1
    n64 = built["nodes64"].copy()
    n64[n, 9] = 0                                                              # the four hix bytes of the 64-byte node: the planes at the corner
    assert tree_containment_errors_exact(built["nodes"], built["tris"], built["rootRef"], fp, n64) >= 1


def _same_tree(a, b):
    return all((a[k] is None) == (b[k] is None) and (a[k] is None or same_words(a[k], b[k])) for k in ARRAYS)


def _step(sim, fp):
    sim.update(0, fp)
    return sim.refit().read()


@pytest.mark.parametrize("case", BASE_CASES)
def test_a_chain_comes_back_to_the_built_tree(case):
    fp0 = base_faces(case)
    sim = RefitSim(base_scene(case), 4, 1)
    built = sim.read()
    for d in ("shuffle", "collapse_point", "explode"):
        got = _step(sim, moved_faces(case, d))
        assert tree_containment_errors_exact(got["nodes"], got["tris"], got["rootRef"], moved_faces(case, d), got["nodes64"]) == 0
    had64 = got["nodes64"] is not None
    back = _step(sim, fp0)
    if had64 == (built["nodes64"] is not None):
        assert _same_tree(back, built)
    else:                                                                      # geometric: exploded it is wider than the 64-byte nodes' grid reaches
        assert case == "geometric" and back["nodes64"] is None
    assert same_words(back["nodes"], built["nodes"]) and same_words(back["tris"], built["tris"]) and same_words(back["shade"], built["shade"])
    assert back["sahCost"] == back["sahCostBuilt"] == built["sahCost"]
    sim.close()


@pytest.mark.parametrize("case", BASE_CASES)
def test_a_chain_through_a_node_too_wide_loses_the_64_byte_form_for_good(case):
    fp0 = base_faces(case)
    sim = RefitSim(base_scene(case), 4, 1)
    built = sim.read()
    for d in ("shuffle", "outlier_wide", "collapse_point", "explode"):
        got = _step(sim, moved_faces(case, d))
        assert d == "shuffle" or got["nodes64"] is None
    for _ in range(2):                                                         # the original positions, then an identity refit
        back = _step(sim, fp0)
        assert back["nodes64"] is None and same_words(back["nodes"], built["nodes"]) and same_words(back["tris"], built["tris"])
        assert back["sahCost"] == back["sahCostBuilt"] == built["sahCost"]
    sim.close()


@pytest.mark.parametrize("deformation", ["shuffle", "explode", "outlier_wide"])
@pytest.mark.parametrize("case", ["counts_9", "counts_257", "geometric", "mixed", STRIP])
def test_an_update_of_a_range_is_the_update_of_the_whole_array(case, deformation):
    hs, fp0, fp = base_scene(case), base_faces(case), moved_faces(case, deformation)
    n = len(fp0)
    built = RefitSim(hs, 4, 1).read()
    ranges = [[(0, 1)], [(n - 1, n)], [(0, 1), (n - 1, n)]]
    if len(built["nodes"]):
        a, b = leaf_interior_range(built, n)
        ranges += [[(a, b)], [(1, a), (b, n - 1)]]
    for parts in ranges:
        whole = fp0.copy()
        part = RefitSim(hs, 4, 1)
        for a, b in parts:
            whole[a:b] = fp[a:b]
            part.update(a, fp[a:b])
        one = RefitSim(hs, 4, 1)
        want = _step(one, whole)
        got = part.refit().read()
        assert _same_tree(got, want) and same_words(got["shade"], want["shade"]), parts
        assert got["sahCost"] == want["sahCost"] and got["sahCostBuilt"] == want["sahCostBuilt"]
        assert tree_containment_errors_exact(got["nodes"], got["tris"], got["rootRef"], whole, got["nodes64"]) == 0
        part.close(); one.close()
