"""Point queries on the MI355X (pointkernel.hip): bit for bit the CPU mirror of the kernel's code (tests/hostsim/pointsim.cpp), whatever the grid, the
node format and the path the points take; moving geometry; and nothing else in the context touched."""
import ctypes as C

import numpy as np
import pytest

from common import M
from point_helpers import INF, POINT_DTYPE, point_case, pointsim, same_bits, with_max
from query_helpers import SCENES, coffee_rays
from refit_helpers import RefitSim, moved_faces

pytestmark = pytest.mark.gpu
K = M._capi
CASES = ("duplicates", "degenerate", "geometric", "offset", "mixed", "counts_9")


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0)
    gpu_ctx.set_option("query_blocks_per_cu", 32)


def _load(ctx, hs, node_format=0):
    ctx.set_option("node_format", node_format)
    ctx.load(hs)


def _coffee(ctx, node_format=0):
    pc = point_case("file:coffee")
    _load(ctx, pc.hs, node_format)
    return pc


def _both_modes(ctx, pc, fmt, mirror_fmt):
    for set_name, q in pc.sets(walked=True):
        for mode in ("closest", "any"):
            assert same_bits(ctx.query_points(q, mode), pointsim(pc.sim, q, mode, node_format=mirror_fmt)), (set_name, mode)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("kind,iarg", SCENES, ids=[s[0].replace("file:", "") for s in SCENES])
def test_gpu_points_are_the_cpu_mirrors_bits(ctx, kind, iarg, fmt):
    pc = point_case(kind)
    _load(ctx, pc.hs, fmt)
    _both_modes(ctx, pc, fmt, fmt)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", CASES)
def test_gpu_points_on_adversarial_meshes(ctx, name):
    pc = point_case("case:" + name)
    _load(ctx, pc.hs)                                      # the default options: the 64-byte nodes where the tree has them
    _both_modes(ctx, pc, 0, 64)


@pytest.mark.timeout(300)
def test_grid_size_does_not_change_a_bit(ctx):
    pc = _coffee(ctx)
    q = dict(pc.sets(walked=True))["shortened"]
    want = {m: pointsim(pc.sim, q, m) for m in ("closest", "any")}
    for bpc in (1, 4, 64):
        ctx.set_option("query_blocks_per_cu", bpc)
        for m in ("closest", "any"):
            assert same_bits(ctx.query_points(q, m), want[m]), (bpc, m)


@pytest.mark.timeout(300)
def test_a_capped_grid_and_a_deep_stack(ctx):
    """2^18 points on coffee through a grid of one workgroup per CU: every lane walks several points one after the other, and the tree's
    stack bound is deeper than the 16 entries a lane keeps in LDS, so the overflow columns are in use.  A 1-in-64 stride against the
    mirror, and the whole "any" output against the whole "closest" one."""
    pc = _coffee(ctx)
    ctx.set_option("query_blocks_per_cu", 1)
    assert 3 * ctx.accel_info().treeDepth + 1 > 16                      # the stack bound of this tree: deeper than the LDS part
    rng = np.random.default_rng(17)
    lo, hi = pc.lo, pc.hi
    diag = float(np.linalg.norm(hi - lo))
    q = with_max(rng.uniform(lo, hi, (1 << 18, 3)).astype(np.float32), np.float32(0.02 * diag))
    h, a = ctx.query_points(q), ctx.query_points(q, "any")
    assert np.array_equal(a, (h["prim"] >= 0).astype(np.int32))
    assert (a == 1).sum() > len(a) // 10 and (a == 0).sum() > len(a) // 10
    sub = q[::64]
    assert same_bits(h[::64], pointsim(pc.sim, sub)) and same_bits(a[::64], pointsim(pc.sim, sub, "any"))
    miss = h[h["prim"] < 0]
    assert (miss["dist"] == q[0, 3]).all() and (miss["mat"] == -1).all() and not miss["p"].any()
    far = with_max(q[::16, :3])                                         # no limit: the walks that go deepest
    assert same_bits(ctx.query_points(far)[::16], pointsim(pc.sim, far[::16]))


@pytest.mark.timeout(300)
def test_torch_device_path_returns_the_host_paths_bits(ctx):
    import torch
    pc = _coffee(ctx)
    q = dict(pc.sets(walked=True))["shortened"][:4096]
    want, want_any = ctx.query_points(q), ctx.query_points(q, "any")
    assert same_bits(want, pointsim(pc.sim, q))
    # the host path's three input forms
    assert same_bits(ctx.query_points(q[:, :3], max_dist=q[:, 3]), want)
    assert same_bits(ctx.query_points(q[:, :3], max_dist=0.05), ctx.query_points(with_max(q[:, :3], np.float32(0.05))))
    assert same_bits(ctx.query_points(q[:, :3]), ctx.query_points(with_max(q[:, :3])))
    dev = torch.device("cuda", 0)
    qt = torch.from_numpy(q).to(dev)
    got = ctx.query_points(qt)
    assert got["records"].shape == (len(q), 8) and got["records"].is_cuda
    assert same_bits(got["records"].cpu().numpy().view(POINT_DTYPE).reshape(-1), want)
    assert got["dist"].dtype == torch.float32 and got["prim"].dtype == torch.int32 and got["mat"].dtype == torch.int32
    assert got["u"].dtype == torch.float32 and got["v"].dtype == torch.float32 and got["p"].dtype == torch.float32 and got["p"].shape == (len(q), 3)
    assert np.array_equal(got["prim"].cpu().numpy(), want["prim"]) and np.array_equal(got["mat"].cpu().numpy(), want["mat"])
    assert same_bits(got["dist"].cpu().numpy(), want["dist"]) and same_bits(got["p"].cpu().numpy(), want["p"])
    assert same_bits(got["u"].cpu().numpy(), want["u"]) and same_bits(got["v"].cpu().numpy(), want["v"])
    ga = ctx.query_points(qt, "any")
    assert ga.dtype == torch.int32 and same_bits(ga.cpu().numpy(), want_any)
    # a slice of a wider tensor, made contiguous
    wide = torch.zeros((len(q), 6), dtype=torch.float32, device=dev)
    wide[:, 1:5] = qt
    sl = wide[:, 1:5]
    assert same_bits(ctx.query_points(sl.contiguous())["records"].cpu().numpy().view(POINT_DTYPE).reshape(-1), want)
    for bad in (sl, qt.cpu(), qt.double(), qt.to(torch.float16), qt.reshape(4, -1), qt.reshape(-1), qt[:, :3].contiguous()):
        with pytest.raises(ValueError):
            ctx.query_points(bad)
    for bad in (q.reshape(-1), q[:, :2], np.zeros((4, 5), np.float32)):
        with pytest.raises(ValueError):
            ctx.query_points(bad)
    with pytest.raises(ValueError):
        ctx.query_points(q[:, :3], max_dist=np.ones(3, np.float32))
    with pytest.raises(ValueError):
        ctx.query_points(qt, "nearest")
    with pytest.raises(ValueError):
        ctx.query_points(q, "nearest")


@pytest.mark.timeout(300)
def test_odd_sizes(ctx):
    import torch
    pc = _coffee(ctx)
    q = dict(pc.sets(walked=True))["shortened"][:1000]
    want, want_any = pointsim(pc.sim, q), pointsim(pc.sim, q, "any")
    for n in (1000, 65, 63, 1, 0):
        h, a = ctx.query_points(q[:n]), ctx.query_points(q[:n], "any")
        assert len(h) == n and len(a) == n
        assert same_bits(h, want[:n]) and same_bits(a, want_any[:n])
        qt = torch.from_numpy(q[:n].copy()).to("cuda:0")
        assert same_bits(ctx.query_points(qt)["records"].cpu().numpy().view(POINT_DTYPE).reshape(-1), want[:n])
        assert same_bits(ctx.query_points(qt, "any").cpu().numpy(), want_any[:n])


@pytest.mark.timeout(300)
def test_query_sees_updated_spheres(ctx):
    hs = M.HostScene("random_spheres", 64, 36, iarg=60)
    _load(ctx, hs)
    n = hs.sizes.nSpheres
    sph = (K.SphereParams * n)()
    for i in range(n):
        sph[i] = hs.flat()["spheres"][i]
    c = np.array([[s.center.x, s.center.y, s.center.z] for s in sph], np.float32)
    r = np.array([s.radius for s in sph], np.float32)
    pts = c.copy(); pts[:, 1] += r + np.float32(0.5)                    # half a unit above each sphere
    before = ctx.query_points(pts)
    own = np.where((before["prim"] == np.arange(n)) & (np.abs(before["dist"] - 0.5) < 1e-3))[0]
    assert len(own) > 0
    i = int(own[0])
    one = (K.SphereParams * 1)(sph[i])
    one[0].center.y += 0.125                                            # towards the point
    ctx.update_spheres(i, one, 1)
    after = ctx.query_points(pts[i:i + 1])
    assert after["prim"][0] == i and abs(float(after["dist"][0]) - 0.375) < 1e-3
    assert ctx.query_points(pts[i:i + 1], "any", max_dist=0.4)[0] == 1 and ctx.query_points(pts[i:i + 1], "any", max_dist=0.3)[0] == 0


@pytest.mark.timeout(300)
@pytest.mark.parametrize("device_rows", [False, True], ids=["host", "device"])
def test_refitted_mesh(ctx, device_rows):
    """update_faces + refit_accel: the GPU equals the refitted mirror; between the update and the refit the call is a state error."""
    import torch
    pc = _coffee(ctx)
    fp, rows = moved_faces(pc.hs, 0.02)
    q = with_max(pc.pts[::8], np.float32(0.05))
    rs = RefitSim(pc.hs, 4)
    try:
        ctx.query_points(q)                                             # the overflow area exists before the refit
        ctx.update_faces(0, torch.from_numpy(rows).to("cuda:0") if device_rows else rows)
        L, out = K.device_lib(), np.zeros(len(q), POINT_DTYPE)
        assert L.moptix_query_points(ctx._h, q.ctypes.data_as(C.POINTER(C.c_float)), len(q), 0, C.c_void_p(out.ctypes.data)) == K.ERR_STATE
        with pytest.raises(M.MoptixError) as e:
            ctx.query_points(torch.from_numpy(q).to("cuda:0"))
        assert e.value.code == K.ERR_STATE
        ctx.refit_accel()
        rs.update(0, fp); rs.refit()
        for mode in ("closest", "any"):
            assert same_bits(ctx.query_points(q, mode), pointsim(rs._sim, q, mode)), mode
        assert len(np.nonzero(ctx.query_points(q)["dist"] != pointsim(pc.sim, q)["dist"])[0]) > len(q) // 4      # the mesh did move
    finally:
        rs.close()


@pytest.mark.timeout(300)
def test_a_point_query_changes_nothing_else(ctx):
    """After a ray query and a refit, a point query leaves moptix_debug_buffer_addresses' eight slots and a ray query's bytes as they were.
    (That a second point query allocates nothing is not shown here: the point overflow area's address is not among those eight slots, and
    reporting it would change the C ABI.)"""
    pc = _coffee(ctx)
    rays = coffee_rays()
    fp, rows = moved_faces(pc.hs, 0.01)
    hits = ctx.query_rays(rays)
    ctx.update_faces(0, rows); ctx.refit_accel()
    hits = ctx.query_rays(rays); occl = ctx.query_rays(rays, "any")
    kept = ctx.debug_buffer_addresses()
    assert kept["query_overflow"] != 0 and all(kept["refit_plan"])
    q = with_max(pc.pts[::8])
    first = ctx.query_points(q)
    assert ctx.debug_buffer_addresses() == kept
    assert same_bits(ctx.query_rays(rays), hits) and same_bits(ctx.query_rays(rays, "any"), occl)
    ctx.update_faces(0, rows); ctx.refit_accel()                        # a refit keeps the point queries' area as it keeps the rays'
    assert same_bits(ctx.query_points(q), first) and same_bits(ctx.query_points(q, "any"), (first["prim"] >= 0).astype(np.int32))
    assert ctx.debug_buffer_addresses() == kept
    assert same_bits(ctx.query_rays(rays), hits)


@pytest.mark.timeout(300)
def test_bad_arguments(ctx):
    import torch
    hs = M.HostScene("spheres", 64, 36)
    _load(ctx, hs)
    L, h = K.device_lib(), ctx._h
    q = with_max(np.zeros((4, 3), np.float32))
    out = np.zeros(4, POINT_DTYPE)
    qp, op = q.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(out.ctypes.data)
    assert L.moptix_query_points(h, qp, -1, 0, op) == K.ERR_INVALID
    assert L.moptix_query_points(h, qp, 4, 2, op) == K.ERR_INVALID
    assert L.moptix_query_points(h, qp, 4, -1, op) == K.ERR_INVALID
    assert L.moptix_query_points(h, None, 4, 0, op) == K.ERR_INVALID
    assert L.moptix_query_points(h, qp, 4, 0, None) == K.ERR_INVALID
    assert L.moptix_query_points(h, None, 0, 0, None) == K.MOPTIX_OK
    assert L.moptix_query_points_device(h, None, 0, 1, None) == K.MOPTIX_OK
    assert L.moptix_query_points_device(h, None, 4, 0, None) == K.ERR_INVALID
    assert L.moptix_query_points(None, qp, 4, 0, op) == K.ERR_INVALID
    dq = torch.zeros(4 * 4 + 4, dtype=torch.float32, device="cuda:0"); do = torch.zeros(4 * 8 + 4, dtype=torch.float32, device="cuda:0")
    vp = C.c_void_p
    assert L.moptix_query_points_device(h, vp(dq.data_ptr()), 4, 0, vp(do.data_ptr())) == K.MOPTIX_OK
    ctx.sync()
    assert L.moptix_query_points_device(h, vp(dq.data_ptr() + 4), 4, 0, vp(do.data_ptr())) == K.ERR_INVALID
    assert L.moptix_query_points_device(h, vp(dq.data_ptr()), 4, 0, vp(do.data_ptr() + 4)) == K.ERR_INVALID
    assert L.moptix_query_points_device(h, vp(dq.data_ptr()), 4, 1, vp(do.data_ptr() + 2)) == K.ERR_INVALID
    assert L.moptix_query_points_device(h, vp(dq.data_ptr()), 4, 1, vp(do.data_ptr() + 4)) == K.MOPTIX_OK      # "any" writes int32: 4 bytes do
    ctx.sync()
    fresh = M.Context(0)
    try:
        assert L.moptix_query_points(fresh._h, qp, 4, 0, op) == K.ERR_STATE          # no params, no tree
        assert L.moptix_query_points_device(fresh._h, vp(dq.data_ptr()), 4, 0, vp(do.data_ptr())) == K.ERR_STATE
    finally:
        fresh.close()
