"""The mesh refit without a GPU: the CPU mirror (tests/hostsim/refitsim.cpp: pt_refit.h compiled for the host, on the host mirror of the builder's tree)
against fresh builds of the same positions -- the refitted tree is a valid tree, its triangle records are a fresh build's, and what a
render or a query computes on it does not depend on which of the two trees it walks (rule D5)."""
import numpy as np
import pytest

from common import M, MovedScene, hostsim_bvh, hostsim_render, tree_containment_errors
from query_helpers import coffee_rays, querysim, same_bits
from refit_helpers import RefitSim, displace, extent, moved_faces, new_normals, same_words, wide_strip

K = M._capi
TREES = [(1, 0), (1, 1), (4, 0), (4, 1), (8, 0), (8, 1)]                      # (leaf size, builder)
# (amplitude as a share of the scene's extent, first face, faces or None = to the end)
MOVES = [(0.01, 0, None), (0.10, 0, None), (0.01, 5000, 60000), (0.10, 5000, 60000)]
SEEDS = M.launch_seeds(2)


@pytest.fixture(scope="module")
def coffee():
    return M.HostScene("file:coffee", 64, 36)


@pytest.fixture(scope="module")
def fresh_renders(coffee):
    """hostsim_render of the scene freshly built from each move's positions, once per (move, leaf size)."""
    cache = {}

    def get(move, leaf):
        if (move, leaf) not in cache:
            cache[(move, leaf)] = hostsim_render(MovedScene(coffee, moved_faces(coffee, *move)[0]), SEEDS, leaf_size=leaf)
        return cache[(move, leaf)]
    return get


def test_package_exports_the_refit():
    names = {"moptix_update_faces", "moptix_update_faces_device", "moptix_refit_accel", "moptix_get_refit_info"}
    assert names <= set(K.DEVICE_SYMBOLS)
    lib = K.device_lib()
    for n in names:
        assert hasattr(lib, n), n
    assert {"update_faces", "refit_accel", "refit_info"} <= set(dir(M.Context))
    assert [f[0] for f in K.RefitInfo._fields_] == ["refitMs", "sahCost", "sahCostBuilt", "has64"]


def test_the_displacement_keeps_shared_vertices_shared(coffee):
    p = coffee.flat()["positions"]
    a = np.float32(0.1 * extent(coffee))
    d = displace(p, a)
    assert d.dtype == np.float32 and np.abs(d - p).max() <= a * 1.000001 and np.abs(d - p).max() > 0.5 * a
    fp = coffee.face_arrays()[0]
    assert same_words(displace(fp.reshape(-1, 3), a), d[coffee.flat()["vIdx"].reshape(-1)])


@pytest.mark.parametrize("leaf,builder", TREES)
def test_identity_refit_reproduces_the_built_tree(coffee, leaf, builder):
    nodes, tris, prim, root, depth, n64 = hostsim_bvh(coffee, leaf, builder, want_nodes64=True)
    sim = RefitSim(coffee, leaf, builder)
    built = sim.read()
    assert same_words(built["nodes"], nodes) and same_words(built["tris"], tris) and same_words(built["nodes64"], n64)
    got = sim.refit().read()
    assert same_words(got["nodes"], nodes) and same_words(got["tris"], tris) and same_words(got["nodes64"], n64)
    assert same_words(got["shade"], built["shade"]) and got["rootRef"] == root
    assert got["sahCost"] == got["sahCostBuilt"] > 1.0
    again = sim.refit().read()
    assert all(same_words(again[k], got[k]) for k in ("nodes", "nodes64", "tris", "shade")) and again["sahCost"] == got["sahCost"]


@pytest.mark.parametrize("move", MOVES, ids=["1pc-all", "10pc-all", "1pc-range", "10pc-range"])
@pytest.mark.parametrize("leaf,builder", TREES)
def test_displaced_refit(coffee, fresh_renders, leaf, builder, move):
    face_pos, rows = moved_faces(coffee, *move)
    first = move[1]
    assert first == 0 or first > 0 and len(rows) < len(face_pos)
    sim = RefitSim(coffee, leaf, builder)
    sim.update(first, rows)
    got = sim.refit().read()
    # a valid tree: every child box, in either node form, contains the triangles below it
    assert got["nodes64"] is not None
    assert tree_containment_errors(got["nodes"], got["tris"], got["rootRef"], got["nodes64"]) == 0
    # every triangle record is the one a fresh build writes for that face (the two trees order them differently)
    moved = MovedScene(coffee, face_pos)
    fnodes, ftris, fprim, froot, fdepth = hostsim_bvh(moved, leaf, builder)
    prim = got["tris"][:, 7].view(np.int32)
    assert np.array_equal(np.sort(prim), np.arange(len(prim)))
    by_face = np.empty_like(ftris); by_face[fprim] = ftris
    assert same_words(got["tris"], by_face[prim])
    # rule D5: the image, the ray count and the closest-hit count do not depend on the tree
    want, wc = fresh_renders(move, leaf)
    img, c = sim.render(SEEDS)
    assert same_words(img, want)
    assert c["closestHits"] == wc["closestHits"]
    assert c["primaryRays"] + c["bounceRays"] + c["shadowRays"] == wc["primaryRays"] + wc["bounceRays"] + wc["shadowRays"]
    img64, c64 = sim.render(SEEDS, node_format=64)
    assert same_words(img64, want) and c64["closestHits"] == wc["closestHits"]
    # the cost signal
    if move[0] >= 0.1:
        assert got["sahCost"] / got["sahCostBuilt"] > 1.0
    assert got["sahCostBuilt"] == RefitSim(coffee, leaf, builder).read()["sahCost"]
    rebuilt = RefitSim(moved, leaf, builder).refit().read()
    assert rebuilt["sahCost"] == rebuilt["sahCostBuilt"]                      # after a fresh build of the same positions the ratio is 1


def test_queries_on_the_refitted_tree_are_the_fresh_trees(coffee):
    face_pos, rows = moved_faces(coffee, 0.10)
    sim = RefitSim(coffee, 4, 1)
    sim.update(0, rows)
    sim.refit()
    moved = MovedScene(coffee, face_pos)
    rays = coffee_rays()
    for mode in ("closest", "any"):
        for fmt in (64, 128):
            assert same_bits(sim.query(rays, mode, node_format=fmt), querysim(moved, rays, mode, node_format=fmt)), (mode, fmt)
    assert (sim.query(rays)["prim"] >= 0).sum() > 1000


def test_two_moves_in_a_row_are_one_move(coffee):
    fp1, _ = moved_faces(coffee, 0.05)
    fp2, _ = moved_faces(coffee, 0.10)
    a = RefitSim(coffee, 4, 0)
    a.update(0, fp1); a.refit(); a.update(0, fp2)
    one = a.refit().read()
    b = RefitSim(coffee, 4, 0)
    b.update(0, fp2)
    two = b.refit().read()
    assert all(same_words(one[k], two[k]) for k in ("nodes", "nodes64", "tris", "shade")) and one["sahCost"] == two["sahCost"]


def test_normals_are_written_only_where_the_face_has_them(coffee):
    fp, fn, has, fm = coffee.face_arrays()
    sim = RefitSim(coffee, 4, 1)
    before = sim.read()
    new = np.full_like(fn, 0.25)
    sim.update(0, fp, new)
    got = sim.refit().read()
    prim = got["tris"][:, 7].view(np.int32)
    sh = got["shade"].view(np.float32)
    flags = got["shade"][:, 3].view(np.int32)
    assert np.array_equal(flags, has[prim]) and same_words(got["tris"], before["tris"]) and same_words(got["nodes"], before["nodes"])
    with_n = flags == 1
    assert (sh[with_n][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] == np.float32(0.25)).all()
    assert not got["shade"][~with_n].any()


def test_normals_on_a_range_that_mixes_faces_with_and_without(coffee):
    """Positions and normals of faces 5000 .. 65000 of coffee with every third run of 7 faces stripped of its normals: the shading records
    and the render are a fresh build's of the scene that has those positions and normals."""
    fp0, _, _, _ = coffee.face_arrays()
    base = MovedScene(coffee, fp0, drop_normals=(np.arange(len(fp0)) // 7) % 3 == 0)
    fp, fn, has, _ = base.face_arrays()
    first, count = 5000, 60000
    assert 0 < has[first:first + count].sum() < count
    fp_moved, rows = moved_faces(base, 0.01, first, count)
    nrm = new_normals(base, first, count)
    assert (np.abs(nrm).max(axis=1) > 0.5).all()                               # also where the face has no normals: to be ignored
    fn_new = fn.copy(); fn_new[first:first + count] = np.where(has[first:first + count, None] != 0, nrm, 0)
    sim = RefitSim(base, 4, 1)
    sim.update(first, rows, nrm)
    got = sim.refit().read()
    want_scene = MovedScene(base, fp_moved, face_nrm=fn_new)
    wfp, wfn, whas, _ = want_scene.face_arrays()
    assert same_words(wfp, fp_moved) and same_words(wfn, fn_new) and np.array_equal(whas, has)
    fresh = RefitSim(want_scene, 4, 1).read()
    by_face = np.empty_like(fresh["shade"]); by_face[fresh["tris"][:, 7].view(np.int32)] = fresh["shade"]
    prim = got["tris"][:, 7].view(np.int32)
    assert same_words(got["shade"], by_face[prim])
    assert not got["shade"][has[prim] == 0].any()                              # flat faces stay flat
    want, wc = hostsim_render(want_scene, SEEDS)
    img, c = sim.render(SEEDS)
    assert same_words(img, want) and c["closestHits"] == wc["closestHits"]
    plain = RefitSim(base, 4, 1); plain.update(first, rows); plain.refit()
    assert not same_words(plain.render(SEEDS)[0], want)                        # the render does see the normals


def test_a_node_too_wide_drops_the_64_byte_form():
    hs, fp = wide_strip()
    for leaf, builder in ((1, 0), (1, 1), (2, 1)):
        sim = RefitSim(hs, leaf, builder)
        built = sim.read()
        assert built["nodes64"] is not None
        sim.update(0, fp)
        got = sim.refit().read()
        assert got["nodes64"] is None
        assert tree_containment_errors(got["nodes"], got["tris"], got["rootRef"]) == 0
        fresh = RefitSim(MovedScene(hs, fp, new_faces=True), leaf, builder).read()
        assert fresh["nodes64"] is None                                        # as at build
        want, wc = hostsim_render(MovedScene(hs, fp, new_faces=True), SEEDS, leaf_size=leaf)
        img, c = sim.render(SEEDS)
        assert same_words(img, want) and c["closestHits"] == wc["closestHits"]
        sim.update(0, hs.face_arrays()[0])                                     # back where it was: the form does not come back
        back = sim.refit().read()
        assert back["nodes64"] is None and same_words(back["nodes"], built["nodes"]) and same_words(back["tris"], built["tris"])


def test_tiny_trees():
    """7 triangles in a strip at leaf sizes 1 and 2 (nodes with 2, 3 and 4 children), and 3 triangles at leaf size 4 (the root is a leaf)."""
    from refit_helpers import strip_scene
    hs7 = strip_scene(7)
    for builder in (0, 1):
        seen = set()
        for leaf in (1, 2):
            sim = RefitSim(hs7, leaf, builder)
            built = sim.read()
            seen |= set(int(c) for c in built["nodes"][:, 28].view(np.int32))
            ident = sim.refit().read()
            assert all(same_words(ident[k], built[k]) for k in ("nodes", "nodes64", "tris", "shade"))
            fp = hs7.face_arrays()[0]
            moved = displace(fp.reshape(-1, 3), 0.3).reshape(-1, 9)
            sim.update(0, moved)
            got = sim.refit().read()
            assert tree_containment_errors(got["nodes"], got["tris"], got["rootRef"], got["nodes64"]) == 0
            assert not same_words(got["nodes"], built["nodes"])
        assert seen == {2, 3, 4}
    hs3 = strip_scene(3)
    sim = RefitSim(hs3, 4, 1)
    built = sim.read()
    assert len(built["nodes"]) == 0 and built["rootRef"] < 0
    moved = displace(hs3.face_arrays()[0].reshape(-1, 3), 0.3).reshape(-1, 9)
    sim.update(1, moved[1:])
    got = sim.refit().read()
    assert same_words(got["tris"][:, [3, 7, 11]], built["tris"][:, [3, 7, 11]]) and got["sahCost"] == 0.0
    p0 = got["tris"].view(np.float32)[:, 0:3]
    prim = got["tris"][:, 7].view(np.int32)
    want = np.where((prim >= 1)[:, None], moved[prim, 0:3], hs3.face_arrays()[0][prim, 0:3])
    assert same_words(p0, want)
