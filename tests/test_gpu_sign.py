"""Signed point queries on the MI355X (signkernel.hip, pointkernel.hip): the device's table of pseudonormals and the signed records are bit for bit the
CPU mirror's (tests/hostsim/signsim.cpp), whatever the node format, the entry point and the grid; the table follows a refit; and the
closest and any modes are not disturbed."""
import ctypes as C

import numpy as np
import pytest

from common import M, HostsimHandle
from point_helpers import invalid_queries, point_case, pointsim, shortened
from refit_helpers import RefitSim, displace
from sign_helpers import (INF, MESHES, POINT_DTYPE, mesh_points, same_bits, sign_case, sign_info, sign_table, signsim, spheres_and_cube,
                          with_max)

pytestmark = pytest.mark.gpu
K = M._capi


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0)
    gpu_ctx.set_option("query_blocks_per_cu", 32)


def _load(ctx, hs, node_format=0):
    ctx.set_option("node_format", node_format)
    ctx.load(hs)


def _sets(sc):
    ref = signsim(sc.sim, sc.q)
    return [("inf", sc.q), ("shortened", shortened(sc.q, np.abs(ref["dist"]), ref["prim"])), ("invalid", invalid_queries(np.append(sc.pts[0], INF)))]


def _moved(sc, amplitude=0.05):
    return displace(sc.face_pos.reshape(-1, 3), amplitude, k=np.float32(2.0)).reshape(-1, 9)


@pytest.mark.parametrize("name", tuple(MESHES))
def test_signed_records_and_info_are_the_mirrors(ctx, name):
    sc = sign_case(name)
    _load(ctx, sc.hs)
    want_info = sign_info(sc.sim)
    assert ctx.sign_info() == want_info                                         # before any signed query: tableBuilds 0
    for set_name, q in _sets(sc):
        assert same_bits(ctx.query_points(q, "signed"), signsim(sc.sim, q)), set_name
    assert same_bits(ctx.sign_table_read(), sign_table(sc.sim))
    assert ctx.sign_info() == dict(want_info, tableBuilds=1)


@pytest.mark.parametrize("name", ["torus", "spike"])
def test_table_before_and_after_a_refit(ctx, name):
    sc = sign_case(name)
    _load(ctx, sc.hs)
    rs = RefitSim(sc.hs, 4)
    try:
        before = ctx.sign_table_read()
        assert same_bits(before, sign_table(rs._sim)) and before.shape == (len(sc.f), 24)
        fp = _moved(sc)
        ctx.update_faces(0, fp); ctx.refit_accel()
        rs.update(0, fp); rs.refit()
        after = ctx.sign_table_read()
        assert same_bits(after, sign_table(rs._sim)) and not same_bits(after, before)
        assert same_bits(ctx.query_points(sc.q, "signed"), signsim(rs._sim, sc.q))
        ctx.update_faces(0, fp); ctx.refit_accel()                              # over unchanged positions: the same words
        assert same_bits(ctx.sign_table_read(), after)
    finally:
        rs.close()


@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("name", ["torus", "spike"])
def test_node_formats_entry_points_and_grids(ctx, name, fmt):
    import torch
    sc = sign_case(name)
    _load(ctx, sc.hs, fmt)
    q = sc.q[:4096]
    want = signsim(sc.sim, q, fmt)
    assert same_bits(signsim(sc.sim, q, 192 - fmt), want)                       # the other node format gives the same bytes
    for bpc in (1, 32):
        ctx.set_option("query_blocks_per_cu", bpc)
        assert same_bits(ctx.query_points(q, "signed"), want), bpc
        got = ctx.query_points(torch.from_numpy(q).to("cuda:0"), "signed")
        assert got["records"].shape == (len(q), 8)
        assert same_bits(got["records"].cpu().numpy().view(POINT_DTYPE).reshape(-1), want), bpc
        assert same_bits(got["dist"].cpu().numpy(), want["dist"])
    for n in (1000, 65, 1, 0):
        assert same_bits(ctx.query_points(q[:n], "signed"), want[:n])


def test_a_capped_grid(ctx):
    """300,000 points on the torus through a grid of one workgroup per CU: every lane walks several points one after the other."""
    sc = sign_case("torus")
    _load(ctx, sc.hs)
    ctx.set_option("query_blocks_per_cu", 1)
    rng = np.random.default_rng(29)
    lo, hi = sc.pts.min(axis=0), sc.pts.max(axis=0)
    q = with_max(rng.uniform(lo, hi, (300000, 3)).astype(np.float32), np.float32(0.25))
    got = ctx.query_points(q, "signed")
    assert same_bits(got, signsim(sc.sim, q))
    hit = got["prim"] >= 0
    assert (got["dist"][hit] < 0).sum() > 10000 and (got["dist"][hit] > 0).sum() > 10000 and (~hit).sum() > 10000
    assert (got["dist"][~hit] == np.float32(0.25)).all()


def test_spheres_quads_and_a_mesh(ctx):
    hs, c, r, v, f = spheres_and_cube()
    sim = HostsimHandle(hs, 4)
    _load(ctx, hs)
    d = np.random.default_rng(5).normal(size=(len(c), 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = np.concatenate([c, c + 0.5 * r[:, None] * d, c + 1.5 * r[:, None] * d, mesh_points(v, f)[0]]).astype(np.float32)
    q = with_max(pts)
    got = ctx.query_points(q, "signed")
    assert same_bits(got, signsim(sim, q))
    assert (got["dist"] < 0).sum() > 20 and (got["prim"] < hs.sizes.nSpheres).sum() >= 3
    pc = point_case("cornell_quads")
    _load(ctx, pc.hs)
    q = with_max(pc.pts)
    got = ctx.query_points(q, "signed")
    assert same_bits(got, signsim(pc.sim, q)) and same_bits(got, pointsim(pc.sim, q)) and not np.signbit(got["dist"]).any()
    assert ctx.sign_info() == dict(sign_info(pc.sim), tableBuilds=0)            # no faces: nothing to build


def test_the_other_modes_are_not_disturbed(ctx):
    sc = sign_case("torus")
    _load(ctx, sc.hs)
    q = shortened(sc.q, np.abs(signsim(sc.sim, sc.q)["dist"]), signsim(sc.sim, sc.q)["prim"])
    closest, anyhit = ctx.query_points(q), ctx.query_points(q, "any")
    assert same_bits(closest, pointsim(sc.sim, q)) and same_bits(anyhit, pointsim(sc.sim, q, "any"))
    kept = ctx.debug_buffer_addresses()
    signed = ctx.query_points(q, "signed")
    assert same_bits(signed, signsim(sc.sim, q))
    assert same_bits(ctx.query_points(q), closest) and same_bits(ctx.query_points(q, "any"), anyhit)
    assert ctx.debug_buffer_addresses() == kept
    a, b = signed.copy(), closest.copy()
    a["dist"] = np.abs(a["dist"]); b["dist"] = np.abs(b["dist"])
    assert same_bits(a, b)                                                      # only the sign bit of dist differs


def test_table_builds(ctx):
    sc = sign_case("torus")
    _load(ctx, sc.hs)
    assert ctx.sign_info()["tableBuilds"] == 0
    ctx.query_points(sc.q, "signed"); ctx.query_points(sc.q, "signed")
    assert ctx.sign_info()["tableBuilds"] == 1
    ctx.query_points(sc.q); ctx.query_points(sc.q, "any")
    assert ctx.sign_info()["tableBuilds"] == 1
    ctx.update_faces(0, _moved(sc)); ctx.refit_accel()
    ctx.query_points(sc.q)
    assert ctx.sign_info()["tableBuilds"] == 1
    ctx.query_points(sc.q, "signed")
    assert ctx.sign_info()["tableBuilds"] == 2


def test_state_and_argument_errors(ctx):
    import torch
    sc = sign_case("cube")
    _load(ctx, sc.hs)
    L, h = K.device_lib(), ctx._h
    q = np.ascontiguousarray(sc.q[:4])
    out = np.zeros(4, POINT_DTYPE)
    qp, op = q.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(out.ctypes.data)
    assert L.moptix_query_points(h, qp, 4, 3, op) == K.ERR_INVALID
    assert L.moptix_query_points(h, qp, 4, 2, op) == K.ERR_INVALID              # the host entry keeps its two modes ...
    assert L.moptix_query_points_signed(h, qp, 4, op) == K.MOPTIX_OK            # ... the signed host form is its own entry
    assert same_bits(out, signsim(sc.sim, q))
    assert L.moptix_query_points_signed(h, qp, 4, None) == K.ERR_INVALID and L.moptix_query_points_signed(h, qp, -1, op) == K.ERR_INVALID
    assert L.moptix_query_points_signed(h, None, 0, None) == K.MOPTIX_OK
    assert L.moptix_query_points_device(h, None, 0, 2, None) == K.MOPTIX_OK
    dq = torch.from_numpy(q).to("cuda:0"); do = torch.zeros(4 * 8 + 4, dtype=torch.float32, device="cuda:0")
    assert L.moptix_query_points_device(h, C.c_void_p(dq.data_ptr()), 4, 3, C.c_void_p(do.data_ptr())) == K.ERR_INVALID
    assert L.moptix_query_points_device(h, C.c_void_p(dq.data_ptr()), 4, 2, C.c_void_p(do.data_ptr() + 4)) == K.ERR_INVALID
    assert L.moptix_get_sign_info(h, None) == K.ERR_INVALID and L.moptix_debug_read_sign_table(h, None) == K.ERR_INVALID
    with pytest.raises(ValueError):
        ctx.query_points(q, "nearest")
    ctx.update_faces(0, sc.face_pos)                                            # faces dirty: a state error like every other query
    assert L.moptix_query_points_signed(h, qp, 4, op) == K.ERR_STATE
    with pytest.raises(M.MoptixError) as e:
        ctx.query_points(dq, "signed")
    assert e.value.code == K.ERR_STATE
    assert ctx.sign_info()["closed"] == 1                                       # the report needs no fitted tree
    ctx.refit_accel()
    assert same_bits(ctx.query_points(q, "signed"), signsim(sc.sim, q))
    assert L.moptix_clear_scene(h) == K.MOPTIX_OK                               # the topology goes with the faces
    assert ctx.sign_info() == dict(weldedVerts=0, edges=0, boundaryEdges=0, nonManifoldEdges=0, flippedEdges=0, degenerateFaces=0, closed=0,
                                   tableBuilds=0, signedVolume=0.0)
    fresh = M.Context(0)
    try:
        assert L.moptix_query_points_signed(fresh._h, qp, 4, op) == K.ERR_STATE # no params, no tree
    finally:
        fresh.close()
