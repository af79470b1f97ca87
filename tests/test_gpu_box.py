"""Box overlap queries on the MI355X (boxkernel.hip pt_boxquery): bit for bit the CPU mirror of the kernel's code (tests/boxsim/boxsim.cpp),
whole buffers -- any, count, the CSR list and the fixed-capacity list -- on the host path and the tensor path."""
import ctypes as C

import numpy as np
import pytest

from box_helpers import box_sets, boxsim, boxsim_list, csr, same_bits
from common import M, MovedScene
from point_helpers import point_case
from query_helpers import SCENES, coffee_rays
from refit_helpers import RefitSim, moved_faces
from sign_helpers import mesh_scene

pytestmark = pytest.mark.gpu
K = M._capi
COFFEE = "file:coffee"
LDS_ENTRIES = 16                       # boxkernel.hip kLdsStack: the stack entries a lane keeps in LDS


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0)
    gpu_ctx.set_option("query_blocks_per_cu", 32)


def _load(ctx, hs, node_format=0):
    ctx.set_option("node_format", node_format)
    ctx.load(hs)


_sets = {}


def _boxes(name):
    """The scene's box set (box_helpers.box_sets); on coffee without most of the 18,184 triangle specials: every 16th of them."""
    if name not in _sets:
        pc = point_case(name)
        b, parts = box_sets(pc.geo, pc.lo, pc.hi)
        if name == COFFEE:
            sp = parts["special"]
            b = np.concatenate([b[:sp.start], b[sp.start:sp.stop - 4:16], b[-4:]])
        _sets[name] = np.ascontiguousarray(b)
    return _sets[name]


def _np(t):
    return t.cpu().numpy()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("kind,iarg", SCENES, ids=[s[0].replace("file:", "") for s in SCENES])
def test_device_is_the_cpu_mirrors_bits(ctx, kind, iarg, fmt):
    import torch
    pc = point_case(kind)
    _load(ctx, pc.hs, fmt)
    b = _boxes(kind)
    n = len(b)
    want_any, want_c = boxsim(pc.sim, b, "any", fmt), boxsim(pc.sim, b, "count", fmt)
    want_p = boxsim_list(pc.sim, b, csr(want_c), fmt)[0]
    cap = 8 if kind == COFFEE else 2                            # a capacity that some of the scene's boxes overflow and some do not fill
    fixed = np.arange(n + 1, dtype=np.int64) * cap
    want_fp, want_fc = boxsim_list(pc.sim, b, fixed, fmt)
    assert (want_c > cap).any() and ((want_c > 0) & (want_c < cap)).sum() > 20 and (want_c == 0).sum() > 20
    tb = torch.from_numpy(b).to("cuda:0")
    # any / count: host path, the (n, 2, 3) form, tensor path
    for mode, want in (("any", want_any), ("count", want_c)):
        got = ctx.query_boxes(b, mode)
        assert got.dtype == np.int32 and got.shape == (n,) and same_bits(got, want), (mode, np.where(got != want)[0][:8])
        assert same_bits(ctx.query_boxes(b.reshape(n, 2, 3), mode), want), mode
        t = ctx.query_boxes(tb, mode)
        assert t.is_cuda and t.dtype == torch.int32 and same_bits(_np(t), want), mode
    # the CSR pair
    prims, offsets = ctx.query_boxes(b, "list")
    assert prims.dtype == np.int32 and offsets.dtype == np.int64 and same_bits(offsets, csr(want_c)) and same_bits(prims, want_p)
    tp, to = ctx.query_boxes(tb, "list")
    assert tp.is_cuda and tp.dtype == torch.int32 and to.dtype == torch.int64
    assert same_bits(_np(to), csr(want_c)) and same_bits(_np(tp), want_p)
    # the fixed-capacity form: truncated slices are -1 throughout, the counts the true ones
    fp, fc = ctx.query_boxes(b, "list", max_prims=cap)
    assert fp.shape == (n, cap) and same_bits(fc, want_c) and same_bits(fc, want_fc) and same_bits(fp.reshape(-1), want_fp)
    assert (fp[want_c > cap] == -1).all()
    tfp, tfc = ctx.query_boxes(tb, "list", max_prims=cap)
    assert tuple(tfp.shape) == (n, cap) and same_bits(_np(tfc), want_c) and same_bits(_np(tfp).reshape(-1), want_fp)
    zp, zc = ctx.query_boxes(b, "list", max_prims=0)
    assert zp.shape == (n, 0) and same_bits(zc, want_c)


@pytest.mark.timeout(300)
def test_capped_grid_walks_several_boxes_per_lane(ctx):
    """One workgroup per CU and more boxes than that grid has lanes, with a partial last block: lanes walk a second box through the same
    stack columns, on a tree deeper than the LDS part of the stack, so the overflow columns of the capped grid are in use.  The mirror's
    bits, and the bits at the default grid."""
    pc = point_case(COFFEE)
    _load(ctx, pc.hs)
    assert 3 * ctx.accel_info().treeDepth + 1 > LDS_ENTRIES
    cus = ctx.get_option("num_cus")
    n = 256 * cus + 257
    rng = np.random.default_rng(35)
    diag = float(np.linalg.norm(pc.hi - pc.lo))
    c = rng.uniform(pc.lo, pc.hi, (n, 3))
    h = diag * 10.0 ** rng.uniform(-3.0, -1.5, (n, 3))
    bl = np.ascontiguousarray(np.concatenate([c - h, c + h], axis=1), np.float32)
    b = bl.copy()
    b[-1] = _boxes(COFFEE)[-4]                                 # any / count: the whole scene, the deepest walk, in the partial last block
    want_c, want_lc = boxsim(pc.sim, b, "count"), boxsim(pc.sim, bl, "count")
    want_p = boxsim_list(pc.sim, bl, csr(want_lc))[0]
    assert (want_c > 64).sum() > 100 and (want_c == 0).sum() > 1000 and want_c[-1] > 100000
    default = (ctx.query_boxes(b, "any"), ctx.query_boxes(b, "count"), ctx.query_boxes(bl, "list"))
    ctx.set_option("query_blocks_per_cu", 1)
    capped = (ctx.query_boxes(b, "any"), ctx.query_boxes(b, "count"), ctx.query_boxes(bl, "list"))
    for anyone, counts, (prims, offsets) in (capped, default):
        assert same_bits(counts, want_c) and same_bits(anyone, (want_c > 0).astype(np.int32))
        assert same_bits(offsets, csr(want_lc)) and same_bits(prims, want_p)


@pytest.mark.timeout(300)
def test_after_update_faces_and_refit(ctx):
    pc = point_case(COFFEE)
    _load(ctx, pc.hs)
    b = _boxes(COFFEE)[1024:]
    before = ctx.query_boxes(b, "count")
    assert same_bits(before, boxsim(pc.sim, b, "count"))
    fp, rows = moved_faces(pc.hs, 0.02)
    ctx.update_faces(0, rows)
    for kw in (dict(mode="any"), dict(mode="count"), dict(mode="list"), dict(mode="list", max_prims=4)):
        with pytest.raises(M.MoptixError) as e:
            ctx.query_boxes(b, **kw)
        assert e.value.code == K.ERR_STATE
    ctx.refit_accel()
    rs = RefitSim(pc.hs, 4)
    try:
        rs.update(0, fp); rs.refit()
        want_c = boxsim(rs._sim, b, "count")
        assert same_bits(ctx.query_boxes(b, "count"), want_c) and same_bits(ctx.query_boxes(b, "any"), boxsim(rs._sim, b, "any"))
        prims, offsets = ctx.query_boxes(b, "list")
        assert same_bits(offsets, csr(want_c)) and same_bits(prims, boxsim_list(rs._sim, b, csr(want_c))[0])
        assert not same_bits(want_c, before)                    # the move changed the answer
    finally:
        rs.close()


@pytest.mark.timeout(300)
def test_query_sees_updated_spheres(ctx):
    hs = M.HostScene("random_spheres", 64, 36, iarg=60)
    _load(ctx, hs)
    n = hs.sizes.nSpheres
    sph = (K.SphereParams * n)()
    for i in range(n):
        sph[i] = hs.flat()["spheres"][i]
    b = _boxes("random_spheres")
    before = ctx.query_boxes(b, "count")
    assert same_bits(before, boxsim(hs, b, "count"))
    for i in range(0, n, 3):
        sph[i].center.y += 0.75
    ctx.update_spheres(0, sph, n)
    moved = MovedScene(hs, spheres=sph)
    want_c = boxsim(moved, b, "count")
    assert not same_bits(want_c, before)
    assert same_bits(ctx.query_boxes(b, "count"), want_c)
    prims, offsets = ctx.query_boxes(b, "list")
    assert same_bits(offsets, csr(want_c)) and same_bits(prims, boxsim_list(moved, b, csr(want_c))[0])


@pytest.mark.timeout(300)
def test_leaves_the_context_alone(ctx):
    pc = point_case(COFFEE)
    _load(ctx, pc.hs)
    b = _boxes(COFFEE)[::4]
    q = np.ascontiguousarray(np.concatenate([pc.pts[::16], np.full((len(pc.pts[::16]), 1), np.inf, np.float32)], axis=1))
    rays = coffee_rays()
    seeds = M.launch_seeds(1)
    ctx.accum_clear(); ctx.render(seeds)
    accum = ctx.accum_read()
    closest, anyone = ctx.query_points(q), ctx.query_points(q, "any")
    hits = ctx.query_rays(rays)
    addr = ctx.debug_buffer_addresses()
    assert addr["query_overflow"] != 0
    counts = ctx.query_boxes(b, "count")
    ctx.query_boxes(b, "any"); ctx.query_boxes(b, "list"); ctx.query_boxes(b, "list", max_prims=4)
    assert ctx.debug_buffer_addresses() == addr
    assert same_bits(ctx.accum_read(), accum)
    assert same_bits(ctx.query_points(q), closest) and same_bits(ctx.query_points(q, "any"), anyone)
    assert same_bits(ctx.query_rays(rays), hits)
    assert same_bits(ctx.query_boxes(b, "count"), counts)
    ctx.refit_accel()                                           # keeps the box queries' overflow area with the others
    assert ctx.debug_buffer_addresses()["query_overflow"] == addr["query_overflow"] and same_bits(ctx.query_boxes(b, "count"), counts)


@pytest.mark.timeout(300)
def test_occupancy_grid_of_the_torus(ctx):
    hs = mesh_scene("torus")
    _load(ctx, hs)
    lo, hi = (-1.5, -1.5, -0.5), (1.5, 1.5, 0.5)
    occ = ctx.occupancy(lo, hi, (16, 16, 16))
    assert occ.shape == (16, 16, 16) and occ.dtype == np.bool_
    want = boxsim(hs, M.occupancy_boxes(lo, hi, (16, 16, 16)), "any").reshape(16, 16, 16) != 0
    assert np.array_equal(occ, want)
    assert 200 < occ.sum() < 2000 and not occ[6:10, 6:10].any() and not occ[0, 0].any()      # a shell: the hole and the corners are empty


@pytest.mark.timeout(300)
def test_argument_errors(ctx):
    import torch
    hs = M.HostScene("spheres", 64, 36)
    _load(ctx, hs)
    L, h = K.device_lib(), ctx._h
    b = np.ascontiguousarray(np.tile(np.array([-1, -1, -1, 1, 1, 1], np.float32), (4, 1)))
    out, prims, off = np.zeros(4, np.int32), np.zeros(16, np.int32), np.arange(5, dtype=np.int64) * 4
    bp, op, pp = b.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_int32)), prims.ctypes.data_as(C.POINTER(C.c_int32))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.moptix_query_boxes(h, bp, 4, K.BOX_ANY, op) == K.MOPTIX_OK
    assert L.moptix_query_boxes(h, bp, 4, K.BOX_COUNT, op) == K.MOPTIX_OK
    for mode in (2, -1, 7):
        assert L.moptix_query_boxes(h, bp, 4, mode, op) == K.ERR_INVALID                      # an unknown mode
    assert L.moptix_query_boxes(h, bp, -1, K.BOX_ANY, op) == K.ERR_INVALID
    assert L.moptix_query_boxes(h, None, 4, K.BOX_ANY, op) == K.ERR_INVALID
    assert L.moptix_query_boxes(h, bp, 4, K.BOX_ANY, None) == K.ERR_INVALID
    assert L.moptix_query_boxes(None, bp, 4, K.BOX_ANY, op) == K.ERR_INVALID
    assert L.moptix_query_boxes(h, None, 0, K.BOX_ANY, None) == K.MOPTIX_OK
    assert L.moptix_query_boxes_device(h, None, 0, K.BOX_COUNT, None) == K.MOPTIX_OK
    assert L.moptix_query_boxes_list(h, bp, 4, fp(off), pp, op) == K.MOPTIX_OK
    assert L.moptix_query_boxes_list(h, bp, -1, fp(off), pp, op) == K.ERR_INVALID
    assert L.moptix_query_boxes_list(h, None, 4, fp(off), pp, op) == K.ERR_INVALID
    assert L.moptix_query_boxes_list(h, bp, 4, None, pp, op) == K.ERR_INVALID
    assert L.moptix_query_boxes_list(h, bp, 4, fp(off), None, op) == K.ERR_INVALID
    assert L.moptix_query_boxes_list(h, bp, 4, fp(off), pp, None) == K.ERR_INVALID
    assert L.moptix_query_boxes_list(None, bp, 4, fp(off), pp, op) == K.ERR_INVALID
    assert L.moptix_query_boxes_list(h, None, 0, None, None, None) == K.MOPTIX_OK
    assert L.moptix_query_boxes_list_device(h, None, 0, None, None, None) == K.MOPTIX_OK
    falling = np.array([0, 4, 3, 8, 12], np.int64)
    assert L.moptix_query_boxes_list(h, bp, 4, fp(falling), pp, op) == K.ERR_INVALID        # offsets decrease
    negative = np.array([-4, 0, 4, 8, 12], np.int64)
    assert L.moptix_query_boxes_list(h, bp, 4, fp(negative), pp, op) == K.ERR_INVALID       # offsets[0] < 0
    dev = torch.device("cuda", 0)
    db = torch.from_numpy(np.concatenate([b, b[:1]])).to(dev)
    do = torch.zeros(8, dtype=torch.int32, device=dev)
    dp = torch.zeros(24, dtype=torch.int32, device=dev)
    doff = torch.from_numpy(np.concatenate([off, off[-1:]])).to(dev)
    vp = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    assert L.moptix_query_boxes_device(h, vp(db), 4, K.BOX_COUNT, vp(do)) == K.MOPTIX_OK
    assert L.moptix_query_boxes_list_device(h, vp(db), 4, vp(doff), vp(dp), vp(do)) == K.MOPTIX_OK
    ctx.sync()
    assert L.moptix_query_boxes_device(h, vp(db, 8), 4, K.BOX_COUNT, vp(do)) == K.MOPTIX_OK            # boxes need 8-byte alignment only
    ctx.sync()
    assert L.moptix_query_boxes_device(h, vp(db, 4), 4, K.BOX_COUNT, vp(do)) == K.ERR_INVALID          # misaligned boxes
    assert L.moptix_query_boxes_device(h, vp(db), 4, K.BOX_COUNT, vp(do, 2)) == K.ERR_INVALID          # misaligned results
    assert L.moptix_query_boxes_device(h, vp(db), 4, 2, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_boxes_device(h, vp(db), -1, K.BOX_ANY, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_boxes_device(h, None, 4, K.BOX_ANY, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_boxes_device(h, vp(db), 4, K.BOX_ANY, None) == K.ERR_INVALID
    assert L.moptix_query_boxes_list_device(h, vp(db, 4), 4, vp(doff), vp(dp), vp(do)) == K.ERR_INVALID
    assert L.moptix_query_boxes_list_device(h, vp(db), 4, vp(doff, 4), vp(dp), vp(do)) == K.ERR_INVALID      # misaligned offsets
    assert L.moptix_query_boxes_list_device(h, vp(db), 4, vp(doff), vp(dp, 2), vp(do)) == K.ERR_INVALID
    assert L.moptix_query_boxes_list_device(h, vp(db), 4, vp(doff), vp(dp), vp(do, 1)) == K.ERR_INVALID
    assert L.moptix_query_boxes_list_device(h, vp(db), 4, None, vp(dp), vp(do)) == K.ERR_INVALID
    assert L.moptix_query_boxes_list_device(h, vp(db), 4, vp(doff), None, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_boxes_list_device(h, vp(db), 4, vp(doff), vp(dp), None) == K.ERR_INVALID
    assert L.moptix_query_boxes_list_device(h, vp(db), -1, vp(doff), vp(dp), vp(do)) == K.ERR_INVALID
    db = db[:4].contiguous()
    for bad in (db[:, :5], db.cpu(), db.double(), db.reshape(-1), db.reshape(2, 12), db.reshape(4, 2, 3)):
        with pytest.raises(ValueError):
            ctx.query_boxes(bad, "count")
    for bad in (b.reshape(-1), b[:, :5], np.zeros((4, 3, 2), np.float32)):
        with pytest.raises(ValueError):
            ctx.query_boxes(bad, "count")
    for kw in (dict(mode="closest"), dict(mode="count", max_prims=4), dict(mode="list", max_prims=-1)):
        with pytest.raises(ValueError):
            ctx.query_boxes(b, **kw)
        with pytest.raises(ValueError):
            ctx.query_boxes(db, **kw)
    assert len(ctx.query_boxes(np.zeros((0, 6), np.float32), "count")) == 0
    ep, eo = ctx.query_boxes(np.zeros((0, 6), np.float32), "list")
    assert len(ep) == 0 and same_bits(eo, np.zeros(1, np.int64))
    fresh = M.Context(0)
    try:
        assert L.moptix_query_boxes(fresh._h, bp, 4, K.BOX_ANY, op) == K.ERR_STATE      # no params, no tree
        assert L.moptix_query_boxes_device(fresh._h, vp(db), 4, K.BOX_ANY, vp(do)) == K.ERR_STATE
        assert L.moptix_query_boxes_list(fresh._h, bp, 4, fp(off), pp, op) == K.ERR_STATE
        assert L.moptix_query_boxes_list_device(fresh._h, vp(db), 4, vp(doff), vp(dp), vp(do)) == K.ERR_STATE
    finally:
        fresh.close()
