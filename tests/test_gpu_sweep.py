"""Sphere sweep queries on the MI355X (sweepkernel.hip pt_sweepquery): bit for bit the CPU mirror of the kernel's code
(tests/sweepsim/sweepsim.cpp), whole buffers -- closest and any -- on the host path and the tensor path."""
import ctypes as C

import numpy as np
import pytest

from common import M
from query_helpers import SCENES
from refit_helpers import RefitSim, moved_faces
from sweep_helpers import (SWEEP_DTYPE, exact_mesh_cases, exact_mesh_scene, exact_sphere_case, exact_sphere_scene, invalid_sweeps, make_sweeps,
                           same_bits, sweep_case, sweep_stack_depth, sweepsim)

pytestmark = pytest.mark.gpu
K = M._capi
COFFEE = "file:coffee"
LDS_ENTRIES = 16                       # sweepkernel.hip kLdsStack: the stack entries a lane keeps in LDS


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0)
    gpu_ctx.set_option("query_blocks_per_cu", 32)


def _load(ctx, hs, node_format=0):
    ctx.set_option("node_format", node_format)
    ctx.load(hs)


def _np(t):
    return t.cpu().numpy()


def _records(t):
    """The tensor path's (n, 8) float32 records as a SWEEP_DTYPE array."""
    return np.ascontiguousarray(_np(t["records"])).view(SWEEP_DTYPE).reshape(-1)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("kind,iarg", SCENES, ids=[s[0].replace("file:", "") for s in SCENES])
def test_device_is_the_cpu_mirrors_bits(ctx, kind, iarg, fmt):
    import torch
    c = sweep_case(kind)
    _load(ctx, c.pc.hs, fmt)
    s = c.sweeps
    n = len(s)
    want, want_any = sweepsim(c.pc.sim, s, "closest", fmt), sweepsim(c.pc.sim, s, "any", fmt)
    assert same_bits(want_any, (want["prim"] >= 0).astype(np.int32)) and (want["prim"] >= 0).sum() > 100 and (want["prim"] < 0).sum() > 100
    got = ctx.query_sweeps(s)
    assert got.dtype == SWEEP_DTYPE and got.shape == (n,)
    assert same_bits(got, want), np.where((got["t"] != want["t"]) | (got["prim"] != want["prim"]))[0][:8]
    anyone = ctx.query_sweeps(s, "any")
    assert anyone.dtype == np.int32 and anyone.shape == (n,) and same_bits(anyone, want_any)
    ts = torch.from_numpy(s).to("cuda:0")
    t = ctx.query_sweeps(ts)
    assert t["records"].is_cuda and t["records"].dtype == torch.float32 and tuple(t["records"].shape) == (n, 8)
    assert same_bits(_records(t), want)
    assert same_bits(_np(t["t"]), want["t"]) and same_bits(_np(t["prim"]), want["prim"]) and same_bits(_np(t["p"]), want["p"])
    ta = ctx.query_sweeps(ts, "any")
    assert ta.is_cuda and ta.dtype == torch.int32 and same_bits(_np(ta), want_any)


@pytest.mark.timeout(300)
def test_capped_grid_walks_several_sweeps_per_lane(ctx):
    """One workgroup per CU and more sweeps than that grid has lanes, with a partial last block: lanes walk a second sweep through the
    same stack columns, on walks deeper than the LDS part of the stack, so the overflow columns of the capped grid are in use.  The
    mirror's bits, and the bits at the default grid."""
    c = sweep_case(COFFEE)
    _load(ctx, c.pc.hs)
    cus = ctx.get_option("num_cus")
    n = 256 * cus + 257
    rng = np.random.default_rng(37)
    lo, hi = np.asarray(c.pc.lo, np.float64), np.asarray(c.pc.hi, np.float64)
    diag = float(np.linalg.norm(hi - lo))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    v = 2.0 ** rng.uniform(-2.0, 2.0, (n, 1))
    s = make_sweeps(rng.uniform(lo, hi, (n, 3)), d * v, diag * 10.0 ** rng.uniform(-3.0, -1.5, n), 2.0 * diag / v)
    s[-300:] = c.sweeps[np.linspace(0, len(c.sweeps) - 1, 300).astype(np.int64)]      # the set's own sweeps, in the partial last block too
    assert sweep_stack_depth(c.pc.sim, s[::16]) > LDS_ENTRIES
    want = sweepsim(c.pc.sim, s)
    assert (want["prim"] >= 0).sum() > 1000 and (want["prim"] < 0).sum() > 100
    default = (ctx.query_sweeps(s), ctx.query_sweeps(s, "any"))
    ctx.set_option("query_blocks_per_cu", 1)
    capped = (ctx.query_sweeps(s), ctx.query_sweeps(s, "any"))
    for hits, anyone in (capped, default):
        assert same_bits(hits, want) and same_bits(anyone, (want["prim"] >= 0).astype(np.int32))


@pytest.mark.timeout(300)
def test_after_update_faces_and_refit(ctx):
    c = sweep_case(COFFEE)
    _load(ctx, c.pc.hs)
    s = c.sweeps
    before = ctx.query_sweeps(s)
    assert same_bits(before, c.hits)
    fp, rows = moved_faces(c.pc.hs, 0.02)
    ctx.update_faces(0, rows)
    for mode in ("closest", "any"):
        with pytest.raises(M.MoptixError) as e:
            ctx.query_sweeps(s, mode)
        assert e.value.code == K.ERR_STATE
    ctx.refit_accel()
    rs = RefitSim(c.pc.hs, 4)
    try:
        rs.update(0, fp); rs.refit()
        want = sweepsim(rs._sim, s)
        assert same_bits(ctx.query_sweeps(s), want) and same_bits(ctx.query_sweeps(s, "any"), sweepsim(rs._sim, s, "any"))
        assert not same_bits(want, before)                      # the move changed the answer
    finally:
        rs.close()


@pytest.mark.timeout(300)
def test_invalid_sweeps_and_exact_cases(ctx):
    hs = exact_mesh_scene()
    hs.upload(ctx)
    names, s, want = exact_mesh_cases()
    got = ctx.query_sweeps(s)
    for k, nm in enumerate(names):
        assert same_bits(got[k:k + 1], want[k:k + 1]), (nm, got[k], want[k])
    assert same_bits(ctx.query_sweeps(s, "any"), (want["prim"] >= 0).astype(np.int32))
    bad = invalid_sweeps(s[0])
    got = ctx.query_sweeps(bad)
    assert (got["prim"] == -1).all() and (got["mat"] == -1).all() and same_bits(got["t"], bad[:, 7])
    assert not got["u"].any() and not got["v"].any() and not got["p"].any()
    assert not ctx.query_sweeps(bad, "any").any()
    sph, _ = exact_sphere_scene()
    sph.upload(ctx)
    s, want = exact_sphere_case(sph)
    got = ctx.query_sweeps(s)
    assert same_bits(got, want), (got, want)


@pytest.mark.timeout(300)
def test_argument_errors(ctx):
    import torch
    hs = M.HostScene("spheres", 64, 36)
    _load(ctx, hs)
    L, h = K.device_lib(), ctx._h
    s = np.ascontiguousarray(np.tile(np.array([0, 5, 0, 0, -1, 0, 0.5, 10], np.float32), (4, 1)))
    out = np.zeros(4, SWEEP_DTYPE)
    sp, op = s.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(out.ctypes.data)
    assert L.moptix_query_sweeps(h, sp, 4, K.SWEEP_CLOSEST, op) == K.MOPTIX_OK
    assert L.moptix_query_sweeps(h, sp, 4, K.SWEEP_ANY, op) == K.MOPTIX_OK
    for mode in (2, -1, 7):
        assert L.moptix_query_sweeps(h, sp, 4, mode, op) == K.ERR_INVALID                     # an unknown mode
    assert L.moptix_query_sweeps(h, sp, -1, K.SWEEP_CLOSEST, op) == K.ERR_INVALID
    assert L.moptix_query_sweeps(h, None, 4, K.SWEEP_CLOSEST, op) == K.ERR_INVALID
    assert L.moptix_query_sweeps(h, sp, 4, K.SWEEP_CLOSEST, None) == K.ERR_INVALID
    assert L.moptix_query_sweeps(None, sp, 4, K.SWEEP_CLOSEST, op) == K.ERR_INVALID
    assert L.moptix_query_sweeps(h, None, 0, K.SWEEP_CLOSEST, None) == K.MOPTIX_OK
    assert L.moptix_query_sweeps_device(h, None, 0, K.SWEEP_ANY, None) == K.MOPTIX_OK
    dev = torch.device("cuda", 0)
    ds = torch.from_numpy(np.concatenate([s, s[:1]])).to(dev)
    do = torch.zeros((8, 8), dtype=torch.float32, device=dev)
    vp = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    assert L.moptix_query_sweeps_device(h, vp(ds), 4, K.SWEEP_CLOSEST, vp(do)) == K.MOPTIX_OK
    assert L.moptix_query_sweeps_device(h, vp(ds), 4, K.SWEEP_ANY, vp(do, 4)) == K.MOPTIX_OK          # int32 results need 4-byte alignment only
    ctx.sync()
    assert L.moptix_query_sweeps_device(h, vp(ds, 8), 4, K.SWEEP_CLOSEST, vp(do)) == K.ERR_INVALID     # misaligned sweeps
    assert L.moptix_query_sweeps_device(h, vp(ds), 4, K.SWEEP_CLOSEST, vp(do, 8)) == K.ERR_INVALID     # misaligned records
    assert L.moptix_query_sweeps_device(h, vp(ds), 4, K.SWEEP_ANY, vp(do, 2)) == K.ERR_INVALID
    assert L.moptix_query_sweeps_device(h, vp(ds), 4, 2, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_sweeps_device(h, vp(ds), -1, K.SWEEP_ANY, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_sweeps_device(h, None, 4, K.SWEEP_ANY, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_sweeps_device(h, vp(ds), 4, K.SWEEP_ANY, None) == K.ERR_INVALID
    ds = ds[:4].contiguous()
    for bad in (ds[:, :7], ds.cpu(), ds.double(), ds.reshape(-1), ds.reshape(2, 16), ds.reshape(4, 2, 4)):
        with pytest.raises(ValueError):
            ctx.query_sweeps(bad)
    for bad in (s.reshape(-1), s[:, :7], np.zeros((4, 2, 4), np.float32)):
        with pytest.raises(ValueError):
            ctx.query_sweeps(bad)
    for mode in ("count", "signed", 0):
        with pytest.raises(ValueError):
            ctx.query_sweeps(s, mode)
        with pytest.raises(ValueError):
            ctx.query_sweeps(ds, mode)
    assert len(ctx.query_sweeps(np.zeros((0, 8), np.float32))) == 0 and len(ctx.query_sweeps(np.zeros((0, 8), np.float32), "any")) == 0
    empty = ctx.query_sweeps(torch.zeros((0, 8), dtype=torch.float32, device=dev))
    assert tuple(empty["records"].shape) == (0, 8)
    fresh = M.Context(0)
    try:
        assert L.moptix_query_sweeps(fresh._h, sp, 4, K.SWEEP_CLOSEST, op) == K.ERR_STATE      # no params, no tree
        assert L.moptix_query_sweeps_device(fresh._h, vp(ds), 4, K.SWEEP_CLOSEST, vp(do)) == K.ERR_STATE
    finally:
        fresh.close()


@pytest.mark.timeout(300)
def test_leaves_the_context_alone(ctx):
    from point_helpers import with_max
    c = sweep_case(COFFEE)
    _load(ctx, c.pc.hs)
    s = c.sweeps[::4]
    q = with_max(c.pc.pts[::16])
    closest = ctx.query_points(q)
    addr = ctx.debug_buffer_addresses()
    hits = ctx.query_sweeps(s)
    ctx.query_sweeps(s, "any")
    assert ctx.debug_buffer_addresses() == addr
    assert same_bits(ctx.query_points(q), closest)
    ctx.refit_accel()                                           # keeps the sweep queries' overflow area with the others
    assert same_bits(ctx.query_sweeps(s), hits) and same_bits(ctx.query_points(q), closest)
