"""Mesh updates and the in-place refit on the MI355X (refitkernel.hip): the refitted arrays are the CPU mirror's (tests/hostsim/refitsim.cpp) byte for
byte, an identity refit reproduces the built tree, and what renders, AOVs and queries compute on a refitted tree is what a context that
loaded the moved scene from scratch computes."""
import ctypes as C

import numpy as np
import pytest

from common import M, MovedScene, oracle_scene
from query_helpers import HIT_DTYPE, coffee_rays, same_bits
from refit_helpers import RefitSim, displace, moved_faces, new_normals, same_words, strip_scene, wide_strip

pytestmark = pytest.mark.gpu
K = M._capi
TREES = [(1, 0), (1, 1), (4, 0), (4, 1), (8, 0), (8, 1)]                      # (leaf size, builder)
MOVE = (0.10, 0, None)                                                          # the whole scene by 10 % of its extent
PART = (0.01, 5000, 60000)                                                      # a face range with first > 0 by 1 %
SEEDS = M.launch_seeds(2)
ARRAYS = ("nodes", "nodes64", "tris")


def _defaults(ctx):
    ctx.set_option("leaf_size", 4); ctx.set_option("builder", 1); ctx.set_option("node_format", 0); ctx.set_option("kernel_variant", -1)


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    _defaults(gpu_ctx)


@pytest.fixture(scope="module")
def other():
    """A second context: the one that loads the moved scene from scratch."""
    c = M.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def coffee():
    return M.HostScene("file:coffee", 64, 36)


@pytest.fixture(scope="module")
def moves(coffee):
    """Per move: the scene's face positions after it, the moved rows, the moved scene."""
    out = {}
    for mv in (MOVE, PART):
        fp, rows = moved_faces(coffee, *mv)
        out[mv] = (fp, rows, MovedScene(coffee, fp))
    return out


@pytest.fixture(scope="module")
def mirrors(coffee, moves):
    """The mirror's refitted tree per (leaf size, builder, move), made once."""
    cache = {}

    def get(leaf, builder, mv):
        if (leaf, builder, mv) not in cache:
            sim = RefitSim(coffee, leaf, builder)
            sim.update(mv[1], moves[mv][1])
            sim.refit()
            cache[(leaf, builder, mv)] = (sim, sim.read())
        return cache[(leaf, builder, mv)]
    return get


@pytest.fixture(scope="module")
def oracle_hits(moves):
    rays = coffee_rays()
    prim, t = oracle_scene(moves[MOVE][2]).closest_hits(rays)
    return rays, prim, t


def _setup(c, leaf=4, builder=1, fmt=0, variant=-1):
    c.set_option("leaf_size", leaf); c.set_option("builder", builder); c.set_option("node_format", fmt); c.set_option("kernel_variant", variant)


def _read(c):
    nodes, tris, prim = c.debug_read_accel()
    try:
        n64 = c.debug_read_nodes64()
    except M.MoptixError:                                                       # this tree has no 64-byte form
        n64 = None
    return dict(nodes=nodes, tris=tris, nodes64=n64)


def _same_tree(a, b):
    return all((a[k] is None) == (b[k] is None) and (a[k] is None or same_words(a[k], b[k])) for k in ARRAYS)


def _torch_rows(rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows, np.float32)).to("cuda:0")


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.timeout(300)
def test_tiny_meshes(ctx):
    L = K.device_lib()
    hs7 = strip_scene(7)
    fp = hs7.face_arrays()[0]
    moved = displace(fp.reshape(-1, 3), 0.3).reshape(-1, 9)
    for leaf in (1, 2):
        for builder in (0, 1):
            _setup(ctx, leaf, builder)
            ctx.load(hs7)
            built = _read(ctx)
            if leaf == 1:
                assert set(int(x) for x in built["nodes"][:, 28].view(np.int32)) == {2, 3, 4}
            info = ctx.refit_accel()
            assert _same_tree(_read(ctx), built) and info["sahCost"] == info["sahCostBuilt"] > 0
            sim = RefitSim(hs7, leaf, builder)
            sim.update(0, moved)
            want = sim.refit().read()
            ctx.update_faces(0, moved)
            info = ctx.refit_accel()
            assert _same_tree(_read(ctx), want) and _rel(info["sahCost"], want["sahCost"]) <= 1e-9
    # the root is a leaf: the records only
    hs3 = strip_scene(3)
    _setup(ctx, 4, 1)
    ctx.load(hs3)
    assert ctx.accel_info().nNodes == 0
    m3 = displace(hs3.face_arrays()[0].reshape(-1, 3), 0.3).reshape(-1, 9)
    sim = RefitSim(hs3, 4, 1)
    sim.update(1, m3[1:])
    ctx.update_faces(1, m3[1:])
    info = ctx.refit_accel()
    assert same_words(ctx.debug_read_accel()[1], sim.refit().read()["tris"]) and info["sahCost"] == 0.0 and info["has64"] == 0
    rays = np.array([[*m3[2, 0:3] * 0.25 + m3[2, 3:6] * 0.25 + m3[2, 6:9] * 0.5 + np.float32([0, 0, 1]), 0, 0, -1, 1e-3, 1e27]], np.float32)
    assert same_bits(ctx.query_rays(rays), sim.query(rays)) and ctx.query_rays(rays)["prim"][0] >= 0
    # no triangles at all
    hs = M.HostScene("spheres", 64, 36)
    ctx.load(hs)
    assert L.moptix_refit_accel(ctx._h) == K.MOPTIX_OK
    assert L.moptix_update_faces(ctx._h, 0, 0, None, None) == K.MOPTIX_OK
    assert L.moptix_update_faces(ctx._h, 0, 1, np.zeros(9, np.float32).ctypes.data_as(C.POINTER(C.c_float)), None) == K.ERR_INVALID
    ctx.render(SEEDS)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("leaf,builder", TREES)
def test_refitted_arrays_are_the_mirrors(ctx, coffee, moves, mirrors, leaf, builder):
    _setup(ctx, leaf, builder)
    ctx.load(coffee)
    built = _read(ctx)
    assert built["nodes64"] is not None
    info = ctx.refit_accel()
    assert _same_tree(_read(ctx), built)                                        # the anchor: nothing moved, nothing changes
    assert info["sahCost"] == info["sahCostBuilt"] and info["has64"] == 1 and info["refitMs"] > 0
    for mv, device in ((MOVE, False), (PART, True), (MOVE, True), (PART, False)):
        ctx.load(coffee)
        sim, want = mirrors(leaf, builder, mv)
        ctx.update_faces(mv[1], _torch_rows(moves[mv][1]) if device else moves[mv][1])
        info = ctx.refit_accel()
        got = _read(ctx)
        assert _same_tree(got, want), (mv, device)
        assert _rel(info["sahCost"], want["sahCost"]) <= 1e-9 and _rel(info["sahCostBuilt"], want["sahCostBuilt"]) <= 1e-9
        if mv is MOVE:
            assert info["sahCost"] / info["sahCostBuilt"] > 1.0
        ctx.update_faces(mv[1], moves[mv][1])                                   # the same update again: the same bytes
        ctx.refit_accel()
        assert _same_tree(_read(ctx), got)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("variant", [0, 3, 4])
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("leaf,builder", TREES)
def test_traces_on_the_refitted_tree_are_a_fresh_contexts(ctx, other, coffee, moves, mirrors, oracle_hits, leaf, builder, fmt, variant):
    fp, rows, moved = moves[MOVE]
    rays, op, ot = oracle_hits
    try:
        _setup(other, leaf, builder, fmt, variant)
        other.load(moved)
        other.accum_clear()
        wst = other.render_counted(SEEDS)
        want = other.accum_read()
        other.aov_clear(); other.render_aovs(SEEDS[:1])
        want_aov = other.aov_read()
    finally:
        _defaults(other)
    sim, _ = mirrors(leaf, builder, MOVE)
    hit = op >= 0
    assert hit.sum() > 1000
    for device in (False, True):
        _setup(ctx, leaf, builder, fmt, variant)
        ctx.load(coffee)
        ctx.update_faces(0, _torch_rows(rows) if device else rows)
        ctx.refit_accel()
        ctx.accum_clear()
        st = ctx.render_counted(SEEDS)
        assert same_words(ctx.accum_read(), want), device
        assert st.rays == wst.rays and st.closestHits == wst.closestHits
        ctx.aov_clear(); ctx.render_aovs(SEEDS[:1])
        got_aov = ctx.aov_read()
        assert all(same_words(got_aov[k], want_aov[k]) for k in want_aov)
        for mode in ("closest", "any"):
            assert same_bits(ctx.query_rays(rays, mode), sim.query(rays, mode, node_format=fmt)), (mode, device)
        h = ctx.query_rays(rays)
        assert np.array_equal(h["prim"], op) and np.array_equal(h["t"][hit], ot[hit])


def _raises_state(fn):
    with pytest.raises(M.MoptixError) as e:
        fn()
    assert e.value.code == K.ERR_STATE
    return str(e.value)


@pytest.mark.timeout(300)
def test_state(ctx, other, coffee, moves):
    import torch
    L, h = K.device_lib(), ctx._h
    fp, rows, moved = moves[MOVE]
    f32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ctx.load(coffee)
    rays = coffee_rays(n=64)
    ctx.update_faces(0, rows)
    msg = _raises_state(lambda: ctx.render(SEEDS))
    assert "moptix_refit_accel" in msg and "moptix_build_accel" in msg
    _raises_state(lambda: ctx.render_aovs(SEEDS[:1]))
    _raises_state(lambda: ctx.render_adaptive(SEEDS))
    _raises_state(lambda: ctx.query_rays(rays))
    _raises_state(lambda: ctx.query_rays(torch.from_numpy(rays).to("cuda:0")))
    ctx.refit_accel()
    ctx.render(SEEDS); ctx.query_rays(rays)
    ctx.update_faces(0, fp)
    _raises_state(lambda: ctx.render(SEEDS))
    ctx.build_accel("Trbvh")
    ctx.render(SEEDS)
    host_built = _read(ctx)
    # a device-side update, then a rebuild: the tree of a context that loaded the moved positions
    ctx.load(coffee)
    ctx.update_faces(0, _torch_rows(rows))
    ctx.build_accel("Trbvh")
    other.load(moved)
    want = _read(other)
    assert _same_tree(_read(ctx), want) and _same_tree(host_built, want)
    # bad arguments
    n = len(fp)
    pos = np.ascontiguousarray(rows[:4])
    assert L.moptix_update_faces(h, -1, 4, f32p(pos), None) == K.ERR_INVALID
    assert L.moptix_update_faces(h, n - 3, 4, f32p(pos), None) == K.ERR_INVALID
    assert L.moptix_update_faces(h, 0, -1, f32p(pos), None) == K.ERR_INVALID
    assert L.moptix_update_faces(h, 0, 4, None, None) == K.ERR_INVALID
    assert L.moptix_update_faces(None, 0, 4, f32p(pos), None) == K.ERR_INVALID
    bad = pos.copy(); bad[2, 5] = np.nan
    assert L.moptix_update_faces(h, 0, 4, f32p(bad), None) == K.ERR_INVALID
    bad[2, 5] = np.inf
    assert L.moptix_update_faces(h, 0, 4, f32p(pos), f32p(bad)) == K.ERR_INVALID
    dev = _torch_rows(np.concatenate([pos.reshape(-1), np.zeros(1, np.float32)]))
    assert L.moptix_update_faces_device(h, 0, 4, None, None) == K.ERR_INVALID
    assert L.moptix_update_faces_device(h, n - 3, 4, C.c_void_p(dev.data_ptr()), None) == K.ERR_INVALID
    assert L.moptix_update_faces_device(h, 0, 4, C.c_void_p(dev.data_ptr() + 2), None) == K.ERR_INVALID
    assert L.moptix_update_faces_device(h, 0, 4, C.c_void_p(dev.data_ptr()), C.c_void_p(dev.data_ptr() + 1)) == K.ERR_INVALID
    assert L.moptix_get_refit_info(h, None) == K.ERR_INVALID and L.moptix_refit_accel(None) == K.ERR_INVALID
    ctx.render(SEEDS)                                                            # none of the refused calls left the faces dirty
    for wrong in (dev.cpu(), dev[:36].double(), dev[:35], dev[:36].reshape(6, 6).t()):
        with pytest.raises(ValueError):
            ctx.update_faces(0, wrong)
    # a refit needs a tree; before the build an update edits the staging only
    fresh = M.Context(0)
    try:
        assert L.moptix_refit_accel(fresh._h) == K.ERR_STATE
        ctx.set_option("leaf_size", 8)                                            # invalidates the tree
        assert L.moptix_refit_accel(h) == K.ERR_STATE
        ctx.update_faces(0, coffee.face_arrays()[0])                              # staging: the host entry puts the original positions back,
        ctx.update_faces(0, _torch_rows(fp))                                      # then the device entry the moved ones on top
        ctx.build_accel("Trbvh")
        other.set_option("leaf_size", 8); other.load(moved)
        assert _same_tree(_read(ctx), _read(other))
    finally:
        fresh.close(); other.set_option("leaf_size", 4)


@pytest.mark.timeout(300)
def test_what_a_refit_keeps(ctx, coffee, moves):
    import torch
    fp, rows, moved = moves[MOVE]
    _setup(ctx, 4, 1, 0, 4)
    ctx.load(coffee)
    ctx.accum_clear(); ctx.render(SEEDS)                                         # decides the node format
    fmt = ctx.get_option("node_format_used")
    ctx.aov_clear(); ctx.render_aovs(SEEDS); ctx.denoise_temporal(2); ctx.denoise_temporal(2)
    assert ctx.aov_samples() == 2 and ctx.temporal_info()["frames"] == 2
    rt = torch.from_numpy(coffee_rays()).to("cuda:0")
    dev_rows = _torch_rows(rows)
    ctx.query_rays(rt)
    ctx.update_faces(0, dev_rows); ctx.refit_accel()                              # the first refit makes its plan
    depth = ctx.accel_info().treeDepth
    kept = ctx.debug_buffer_addresses()
    assert kept["query_overflow"] != 0 and all(kept["refit_plan"])
    ctx.update_faces(0, dev_rows); info = ctx.refit_accel()
    ctx.query_rays(rt)
    assert ctx.debug_buffer_addresses() == kept                                  # the refit kept its plan, the query after it its overflow area
    assert ctx.get_option("node_format_used") == fmt and info["has64"] == 1 and ctx.accel_info().treeDepth == depth
    assert ctx.aov_samples() == 2 and ctx.temporal_info()["frames"] == 2
    a = _read(ctx)
    ctx.update_faces(0, rows); ctx.refit_accel()
    assert _same_tree(_read(ctx), a)
    ctx.render(SEEDS)
    assert ctx.get_option("node_format_used") == fmt
    ctx.load(coffee)                                                             # whereas a rebuild drops the overflow area and the plan
    gone = ctx.debug_buffer_addresses()
    assert gone["query_overflow"] == 0 and not any(gone["refit_plan"])


@pytest.mark.timeout(300)
def test_normals_through_both_entries(ctx, other, coffee):
    """Positions and normals of faces 5000 .. 65000 of coffee with every third run of 7 faces stripped of its normals, as numpy arrays and
    as torch tensors: renders and AOVs are those of a context that loaded the scene with those positions and normals; the faces without
    normals ignore what they are handed and shade flat."""
    fp0 = coffee.face_arrays()[0]
    base = MovedScene(coffee, fp0, drop_normals=(np.arange(len(fp0)) // 7) % 3 == 0)
    fp, fn, has, _ = base.face_arrays()
    first, count = 5000, 60000
    assert 0 < has[first:first + count].sum() < count
    fp_moved, rows = moved_faces(base, 0.01, first, count)
    nrm = new_normals(base, first, count)                                        # non-zero for every face, flat ones included
    fn_new = fn.copy(); fn_new[first:first + count] = np.where(has[first:first + count, None] != 0, nrm, 0)
    _setup(other); _setup(ctx)
    other.load(MovedScene(base, fp_moved, face_nrm=fn_new))
    other.accum_clear()
    wst = other.render_counted(SEEDS)
    want = other.accum_read()
    other.aov_clear(); other.render_aovs(SEEDS[:1])
    want_aov = other.aov_read()
    for device in (False, True):
        ctx.load(base)
        if device:
            ctx.update_faces(first, _torch_rows(rows), _torch_rows(nrm))
        else:
            ctx.update_faces(first, rows, nrm)
        ctx.refit_accel()
        ctx.accum_clear()
        st = ctx.render_counted(SEEDS)
        assert same_words(ctx.accum_read(), want), device
        assert st.rays == wst.rays and st.closestHits == wst.closestHits
        ctx.aov_clear(); ctx.render_aovs(SEEDS[:1])
        got_aov = ctx.aov_read()
        assert all(same_words(got_aov[k], want_aov[k]) for k in want_aov), device
        ctx.update_faces(first, _torch_rows(rows) if device else rows)           # positions alone: the normals stay
        ctx.refit_accel()
        ctx.aov_clear(); ctx.render_aovs(SEEDS[:1])
        assert all(same_words(ctx.aov_read()[k], want_aov[k]) for k in want_aov), device
    # the normal AOV sees the update, and a face without normals shows its geometric normal whatever it was handed
    ctx.load(base)
    ctx.update_faces(first, rows); ctx.refit_accel()
    ctx.aov_clear(); ctx.render_aovs(SEEDS[:1])
    assert not same_words(ctx.aov_read()["normal"], want_aov["normal"])
    face = want_aov["primId"][..., 0] - (base.sizes.nSpheres + base.sizes.nQuads)
    tri = (want_aov["hits"][..., 0] > 0) & (face >= first) & (face < first + count)
    flat = tri & (has[np.clip(face, 0, len(has) - 1)] == 0)
    assert flat.sum() > 20 and (tri & ~flat).sum() > 20
    p = fp_moved[face[flat]].astype(np.float64)
    ng = np.cross(p[:, 0:3] - p[:, 6:9], p[:, 3:6] - p[:, 0:3])
    ng /= np.linalg.norm(ng, axis=1, keepdims=True)
    # (binary32 edges: the angle between the two normals is about 2^-23 / sin(the triangle's corner angle), far below the 4.5e-3 this allows)
    assert np.abs(np.abs((want_aov["normal"][flat].astype(np.float64) * ng).sum(axis=1)) - 1.0).max() < 1e-5


@pytest.mark.timeout(300)
def test_a_node_too_wide_drops_the_64_byte_form(ctx, other):
    hs, fp = wide_strip()
    rays = coffee_rays(n=256)
    for leaf, builder in ((1, 0), (2, 1)):
        _setup(ctx, leaf, builder); _setup(other, leaf, builder)
        try:
            other.load(MovedScene(hs, fp, new_faces=True))
            assert _read(other)["nodes64"] is None                               # as at build
            other.accum_clear()
            wst = other.render_counted(SEEDS)
            want = other.accum_read()
            want_hits = {mode: other.query_rays(rays, mode) for mode in ("closest", "any")}
        finally:
            _defaults(other)
        for device in (False, True):
            ctx.load(hs)
            built = _read(ctx)
            assert built["nodes64"] is not None
            ctx.accum_clear(); ctx.render(SEEDS)
            ctx.update_faces(0, _torch_rows(fp) if device else fp)
            info = ctx.refit_accel()
            sim = RefitSim(hs, leaf, builder)
            sim.update(0, fp)
            mirror = sim.refit().read()
            assert info["has64"] == 0 and mirror["nodes64"] is None and _same_tree(_read(ctx), mirror)
            with pytest.raises(M.MoptixError):
                ctx.debug_read_nodes64()
            ctx.accum_clear()
            st = ctx.render_counted(SEEDS)
            assert same_words(ctx.accum_read(), want) and st.rays == wst.rays and st.closestHits == wst.closestHits
            assert ctx.get_option("node_format_used") == 128
            for mode in ("closest", "any"):
                assert same_bits(ctx.query_rays(rays, mode), sim.query(rays, mode, node_format=128)) and same_bits(ctx.query_rays(rays, mode), want_hits[mode])
            ctx.update_faces(0, hs.face_arrays()[0])                             # back where it was: the form does not come back
            info = ctx.refit_accel()
            back = _read(ctx)
            assert info["has64"] == 0 and back["nodes64"] is None and same_words(back["nodes"], built["nodes"]) and same_words(back["tris"], built["tris"])
            ctx.render(SEEDS)


@pytest.mark.timeout(300)
def test_faces_added_after_a_device_side_update_survive_the_fetch(ctx, other, coffee):
    """The device copy covers the faces of the last build.  A mesh added after a device-side update exists in the staging only: the fetch
    that precedes the next build must bring back the updated faces and leave the added ones alone -- also when the device buffers are
    still large from an earlier scene."""
    L = K.device_lib()
    _setup(ctx); _setup(other)
    ctx.load(coffee)                                                             # large device buffers, which are kept
    hs7, hs10 = strip_scene(7), strip_scene(10)
    fp7, fp10 = hs7.face_arrays()[0], hs10.face_arrays()[0]
    assert same_words(fp10[:7], fp7)
    moved = displace(fp7.reshape(-1, 3), 0.3).reshape(-1, 9)
    ctx.load(hs7)
    ctx.update_faces(0, _torch_rows(moved))
    pos = np.ascontiguousarray(fp10[7:].reshape(-1, 3)); vi = np.arange(9, dtype=np.int32)
    ctx._chk(L.moptix_add_mesh(ctx._h, pos.ctypes.data_as(C.POINTER(C.c_float)), 9, None, 0, None, 0,
                               vi.ctypes.data_as(C.POINTER(C.c_int32)), None, None, 3, 0))
    ctx.build_accel("Trbvh")
    other.load(MovedScene(hs10, np.concatenate([moved, fp10[7:]]), new_faces=True))
    assert ctx.accel_info().nTriangles == 10 and _same_tree(_read(ctx), _read(other))
    ctx.render(SEEDS)


@pytest.mark.timeout(300)
def test_two_successive_displacements(ctx, coffee):
    fp1, _ = moved_faces(coffee, 0.05)
    fp2, _ = moved_faces(coffee, 0.10)
    _setup(ctx, 4, 0)
    ctx.load(coffee)
    ctx.update_faces(0, fp1); ctx.refit_accel()
    ctx.update_faces(0, _torch_rows(fp2)); i2 = ctx.refit_accel()
    two = _read(ctx)
    ctx.load(coffee)
    ctx.update_faces(0, fp2); i1 = ctx.refit_accel()
    assert _same_tree(_read(ctx), two) and i1["sahCost"] == i2["sahCost"] and i1["sahCostBuilt"] == i2["sahCostBuilt"]
