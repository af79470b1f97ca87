"""K-nearest point queries on the MI355X (pointkernel.hip pt_pointquery_multi): bit for bit the CPU mirror of the kernel's code
(tests/pointmultisim/pointmultisim.cpp), whole buffers -- records, miss records behind them, counts -- on the host path and the tensor path."""
import ctypes as C

import numpy as np
import pytest

from common import M
from point_helpers import INF, POINT_DTYPE, point_case, with_max
from pointmulti_helpers import duplicates_scene, gpu_point_set, is_miss_record, pointmultisim, same_bits
from query_helpers import SCENES, coffee_rays
from refit_helpers import RefitSim, moved_faces
from sign_helpers import mesh_scene

pytestmark = pytest.mark.gpu
K = M._capi
COFFEE = "file:coffee"


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0)
    gpu_ctx.set_option("query_blocks_per_cu", 32)


def _load(ctx, hs, node_format=0):
    ctx.set_option("node_format", node_format)
    ctx.load(hs)


def _records(t):
    """A tensor path's hits as the host path's array."""
    r = t["records"]
    return r.cpu().numpy().view(POINT_DTYPE).reshape(r.shape[0], r.shape[1])


def _same(got, want):
    return same_bits(got[1], want[1]) and same_bits(got[0], want[0])


def _coffee_queries(pc):
    """The near and special slices and 512 uniform points of coffee's set, with the shortened maxDist (0.5 x / 2 x the nearest distance)."""
    return np.ascontiguousarray(dict(pc.sets(walked=True))["shortened"][gpu_point_set(pc)])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("kind,iarg", SCENES, ids=[s[0].replace("file:", "") for s in SCENES])
def test_device_is_the_cpu_mirrors_bits(ctx, kind, iarg, fmt):
    """The near and special slices plus 512 uniform points, maxDist = inf and the shortened values; K in 1, 4, 64 with and without COUNT_ALL.
    On coffee, COUNT_ALL without a limit is a loop over all 168,196 primitives per point -- a minute of the mirror on the CPU -- and runs
    on every 97th of the points."""
    import torch
    pc = point_case(kind)
    _load(ctx, pc.hs, fmt)
    sel = gpu_point_set(pc)
    some = 0
    for set_name, full in pc.sets(walked=True)[:2]:
        for k in (1, 4, 64):
            for count_all in (False, True):
                q = np.ascontiguousarray(full[sel[::97]] if kind == COFFEE and set_name == "inf" and count_all else full[sel])
                want_h, want_c = pointmultisim(pc.sim, q, k, count_all, node_format=fmt)
                h, c = ctx.query_points_multi(q, k, count_all)
                assert h.shape == (len(q), k) and h.dtype == POINT_DTYPE and c.dtype == np.int32
                assert same_bits(c, want_c), (set_name, k, count_all, np.where(c != want_c)[0][:8])
                assert same_bits(h, want_h), (set_name, k, count_all)
                th, tc = ctx.query_points_multi(torch.from_numpy(q).to("cuda:0"), k, count_all)
                assert th["records"].shape == (len(q), k, 8) and th["records"].is_cuda and tc.dtype == torch.int32
                assert same_bits(tc.cpu().numpy(), want_c) and same_bits(_records(th), want_h), (set_name, k, count_all)
                assert np.array_equal(th["prim"].cpu().numpy(), want_h["prim"]) and same_bits(th["p"].cpu().numpy(), want_h["p"])
                some += int((want_c > 0).sum())
    assert some > 1000
    # the host path's (n, 3) form
    q = np.ascontiguousarray(pc.pts[sel][:256])
    assert _same(ctx.query_points_multi(q, 4, max_dist=0.5), ctx.query_points_multi(with_max(q, np.float32(0.5)), 4))


@pytest.mark.timeout(300)
def test_capped_grid_walks_several_points_per_lane(ctx):
    """One workgroup per CU and more points than that grid has lanes, with a partial last block: lanes walk a second point through the same
    stack columns and list slices of their own.  The mirror's bits, and the bits at the default grid."""
    hs = mesh_scene("torus")
    cus = ctx.get_option("num_cus")
    n = 256 * cus + 257
    rng = np.random.default_rng(33)
    pts = rng.uniform((-2.0, -2.0, -0.8), (2.0, 2.0, 0.8), (n, 3)).astype(np.float32)
    q = with_max(pts, np.where(np.arange(n) % 2 == 0, np.float32(0.15), INF).astype(np.float32))
    _load(ctx, hs)
    default = ctx.query_points_multi(q, 3)
    ctx.set_option("query_blocks_per_cu", 1)
    capped = ctx.query_points_multi(q, 3)
    want = pointmultisim(hs, q, 3)
    assert (want[1] == 3).sum() > 500 and (want[1] == 0).sum() > 500 and ((want[1] > 0) & (want[1] < 3)).sum() > 300
    for got in (capped, default):
        assert _same(got, want)
    # coffee's tree is deeper than the LDS part of the stack: the overflow columns of the capped grid, every lane walking many points
    pc = point_case(COFFEE)
    _load(ctx, pc.hs)
    assert 3 * ctx.accel_info().treeDepth + 1 > 16
    diag = float(np.linalg.norm(pc.hi - pc.lo))
    cpts = rng.uniform(pc.lo, pc.hi, (n, 3)).astype(np.float32)
    for k, count_all, md in ((4, False, INF), (4, True, np.float32(0.02 * diag))):
        cq = with_max(cpts, md)
        assert _same(ctx.query_points_multi(cq, k, count_all), pointmultisim(pc.sim, cq, k, count_all)), (k, count_all)


@pytest.mark.timeout(300)
def test_pure_in_range_count(ctx):
    import torch
    pc = point_case(COFFEE)
    _load(ctx, pc.hs)
    q = _coffee_queries(pc)
    h4, c4 = ctx.query_points_multi(q, 4, True)
    h0, c0 = ctx.query_points_multi(q, 0, True)
    assert h0.shape == (len(q), 0) and same_bits(c0, c4) and c4.max() > 4
    assert same_bits(c4, pointmultisim(pc.sim, q, 0, True)[1])
    counts = np.full(len(q), -7, np.int32)
    rc = K.device_lib().moptix_query_points_multi(ctx._h, q.ctypes.data_as(C.POINTER(C.c_float)), len(q), 0, K.POINT_MULTI_COUNT_ALL, None,
                                                  counts.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == K.MOPTIX_OK and same_bits(counts, c4)
    th, tc = ctx.query_points_multi(torch.from_numpy(q).to("cuda:0"), 0, True)
    assert th["records"].shape == (len(q), 0, 8) and same_bits(tc.cpu().numpy(), c4)


@pytest.mark.timeout(300)
def test_coincident_triangles_on_the_device(ctx):
    """One triangle 100 times (prim = face id): 64 records of one distance with prims 0 .. 63 in order, 100 counted, K = 1 the lowest id."""
    hs = duplicates_scene()
    q = with_max(point_case("case:duplicates").pts)
    for fmt in (64, 128):
        _load(ctx, hs, fmt)
        h, c = ctx.query_points_multi(q, 64, True)
        assert (c == 100).all() and (h["prim"] == np.arange(64)[None, :]).all()
        assert (h["dist"].view(np.uint32) == h["dist"].view(np.uint32)[:, :1]).all()
        assert _same((h, c), pointmultisim(hs, q, 64, True, node_format=fmt))
        h1, c1 = ctx.query_points_multi(q, 1)
        assert (c1 == 1).all() and (h1["prim"] == 0).all() and same_bits(h1, np.ascontiguousarray(h[:, :1]))
        assert (ctx.query_points_multi(q, 64)[1] == 64).all()


@pytest.mark.timeout(300)
def test_leaves_the_context_alone(ctx):
    pc = point_case(COFFEE)
    _load(ctx, pc.hs)
    q = _coffee_queries(pc)[::4]
    rays = coffee_rays()
    seeds = M.launch_seeds(1)
    ctx.accum_clear(); ctx.render(seeds)
    accum = ctx.accum_read()
    closest, anyone = ctx.query_points(q), ctx.query_points(q, "any")
    hits = ctx.query_rays(rays)
    addr = ctx.debug_buffer_addresses()
    assert addr["query_overflow"] != 0
    h, c = ctx.query_points_multi(q, 8, True)
    assert ctx.debug_buffer_addresses() == addr
    assert same_bits(ctx.accum_read(), accum)
    assert same_bits(ctx.query_points(q), closest) and same_bits(np.ascontiguousarray(h[:, 0]), closest)
    assert same_bits(ctx.query_rays(rays), hits)
    assert np.array_equal(c > 0, anyone == 1) and same_bits(ctx.query_points(q, "any"), anyone)
    assert is_miss_record(h, q[:, 3])[np.arange(8)[None, :] >= c[:, None]].all()


@pytest.mark.timeout(300)
def test_after_update_faces(ctx):
    pc = point_case(COFFEE)
    _load(ctx, pc.hs)
    q = with_max(pc.pts[::8], np.float32(0.05))
    fp, rows = moved_faces(pc.hs, 0.02)
    ctx.update_faces(0, rows)
    with pytest.raises(M.MoptixError) as e:
        ctx.query_points_multi(q, 4)
    assert e.value.code == K.ERR_STATE
    ctx.refit_accel()
    rs = RefitSim(pc.hs, 4)
    try:
        rs.update(0, fp); rs.refit()
        for count_all in (False, True):
            want = pointmultisim(rs._sim, q, 4, count_all)
            assert _same(ctx.query_points_multi(q, 4, count_all), want), count_all
        assert not same_bits(want[0], pointmultisim(pc.sim, q, 4, True)[0])      # the move changed the answer
    finally:
        rs.close()


@pytest.mark.timeout(300)
def test_argument_errors(ctx):
    import torch
    hs = M.HostScene("spheres", 64, 36)
    _load(ctx, hs)
    L, h = K.device_lib(), ctx._h
    q = with_max(np.zeros((4, 3), np.float32))
    hits, counts = np.zeros((4, 65), POINT_DTYPE), np.zeros(4, np.int32)
    qp, hp, cp = q.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(hits.ctypes.data), counts.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.moptix_query_points_multi(h, qp, 4, 4, 0, hp, cp) == K.MOPTIX_OK
    assert L.moptix_query_points_multi(h, qp, 4, 0, 0, hp, cp) == K.ERR_INVALID              # maxNear 0 without the flag
    assert L.moptix_query_points_multi(h, qp, 4, 0, K.POINT_MULTI_COUNT_ALL, None, cp) == K.MOPTIX_OK
    assert L.moptix_query_points_multi(h, qp, 4, 65, 0, hp, cp) == K.ERR_INVALID
    assert L.moptix_query_points_multi(h, qp, 4, 65, K.POINT_MULTI_COUNT_ALL, hp, cp) == K.ERR_INVALID
    assert L.moptix_query_points_multi(h, qp, 4, -1, K.POINT_MULTI_COUNT_ALL, hp, cp) == K.ERR_INVALID
    assert L.moptix_query_points_multi(h, qp, 4, 4, 2, hp, cp) == K.ERR_INVALID              # an unknown flag
    assert L.moptix_query_points_multi(h, qp, 4, 4, 0x80000001, hp, cp) == K.ERR_INVALID
    assert L.moptix_query_points_multi(h, qp, -1, 4, 0, hp, cp) == K.ERR_INVALID
    assert L.moptix_query_points_multi(h, None, 4, 4, 0, hp, cp) == K.ERR_INVALID
    assert L.moptix_query_points_multi(h, qp, 4, 4, 0, None, cp) == K.ERR_INVALID
    assert L.moptix_query_points_multi(h, qp, 4, 4, 0, hp, None) == K.ERR_INVALID
    assert L.moptix_query_points_multi(None, qp, 4, 4, 0, hp, cp) == K.ERR_INVALID
    assert L.moptix_query_points_multi(h, None, 0, 4, 0, None, None) == K.MOPTIX_OK
    assert L.moptix_query_points_multi_device(h, None, 0, 4, 0, None, None) == K.MOPTIX_OK
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(np.concatenate([q, q[:1]])).to(dev)
    dh = torch.zeros((4 * 4 * 8 + 8,), dtype=torch.float32, device=dev)
    dc = torch.zeros(8, dtype=torch.int32, device=dev)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    assert L.moptix_query_points_multi_device(h, vp(dq), 4, 4, 0, vp(dh), vp(dc)) == K.MOPTIX_OK
    ctx.sync()
    assert L.moptix_query_points_multi_device(h, vp(dq), 4, 4, 0, vp(dh, 4), vp(dc)) == K.ERR_INVALID      # misaligned records
    assert L.moptix_query_points_multi_device(h, vp(dq), 4, 4, 0, vp(dh), vp(dc, 2)) == K.ERR_INVALID      # misaligned counts
    assert L.moptix_query_points_multi_device(h, vp(dq, 4), 4, 4, 0, vp(dh), vp(dc)) == K.ERR_INVALID      # misaligned points
    assert L.moptix_query_points_multi_device(h, vp(dq), 4, 4, 0, None, vp(dc)) == K.ERR_INVALID
    assert L.moptix_query_points_multi_device(h, vp(dq), 4, 4, 0, vp(dh), None) == K.ERR_INVALID
    assert L.moptix_query_points_multi_device(h, None, 4, 4, 0, vp(dh), vp(dc)) == K.ERR_INVALID
    assert L.moptix_query_points_multi_device(h, vp(dq), -1, 4, 0, vp(dh), vp(dc)) == K.ERR_INVALID
    assert L.moptix_query_points_multi_device(h, vp(dq), 4, 0, 0, vp(dh), vp(dc)) == K.ERR_INVALID
    assert L.moptix_query_points_multi_device(h, vp(dq), 4, 65, 0, vp(dh), vp(dc)) == K.ERR_INVALID
    assert L.moptix_query_points_multi_device(h, vp(dq), 4, 4, 4, vp(dh), vp(dc)) == K.ERR_INVALID
    assert L.moptix_query_points_multi_device(h, vp(dq), 4, 0, K.POINT_MULTI_COUNT_ALL, None, vp(dc)) == K.MOPTIX_OK
    ctx.sync()
    dq = dq[:4].contiguous()
    for bad in (dq[:, :3], dq.cpu(), dq.double(), dq.reshape(-1), dq.reshape(2, 8)):
        with pytest.raises(ValueError):
            ctx.query_points_multi(bad, 4)
    for bad in (q.reshape(-1), q[:, :2], np.zeros((4, 5), np.float32)):
        with pytest.raises(ValueError):
            ctx.query_points_multi(bad, 4)
    with pytest.raises(ValueError):
        ctx.query_points_multi(q[:, :3], 4, max_dist=np.ones(3, np.float32))
    for k, count_all in ((0, False), (65, False), (65, True), (-1, True)):
        with pytest.raises(ValueError):
            ctx.query_points_multi(dq, k, count_all)
        with pytest.raises(ValueError):
            ctx.query_points_multi(q, k, count_all)
    fresh = M.Context(0)
    try:
        assert L.moptix_query_points_multi(fresh._h, qp, 4, 4, 0, hp, cp) == K.ERR_STATE      # no params, no tree
        assert L.moptix_query_points_multi_device(fresh._h, vp(dq), 4, 4, 0, vp(dh), vp(dc)) == K.ERR_STATE
    finally:
        fresh.close()
