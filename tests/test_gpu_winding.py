"""Winding-number queries on the device: the kernel's words and the moments table against the CPU mirror (tests/windingsim) on whole
buffers, on both paths and under both node-format settings; the lazy rebuild of the table across a refit and a rebuild; stream order
of the _device entry; argument errors."""
import ctypes as C
import os

import numpy as np
import pytest

import lbvh_cases
from common import M, HostsimHandle, REPO
from point_helpers import point_case
from refit_helpers import RefitSim, moved_faces, same_words
from stream_helpers import N, behind_busy_stream, busy
from winding_helpers import (INF, QNAN, Geometry, box_points, cube, mesh_scene, rows, same_bits, uv_sphere, winding_table, winding_work,
                             windingsim)

pytestmark = pytest.mark.gpu
K = M._capi
LDS_ENTRIES = 16                       # windingkernel.hip kLdsStack: the stack entries a lane keeps in LDS
SCENES = ("cube", "open_cube", "uv_sphere", "random_spheres", "case:degenerate", "case:offset", "case:mixed")


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_stream(0)
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0)
    gpu_ctx.set_option("query_blocks_per_cu", 32)


def _load(ctx, hs, node_format=0, leaf_size=4):
    ctx.set_option("node_format", node_format); ctx.set_option("leaf_size", leaf_size)
    ctx.load(hs)


_scenes = {}


def _scene(name):
    """(scene, leaf-4 mirror, 1,000 points uniform in 1.5 x its box plus its vertices' neighbourhood), made once."""
    if name not in _scenes:
        if name.startswith("case:"):
            hs = lbvh_cases.case_scene(name[5:])
        elif name == "random_spheres":
            hs = point_case(name).hs
        else:
            hs = mesh_scene({"cube": cube, "open_cube": lambda: cube(top=False), "uv_sphere": uv_sphere}[name]())
        if name == "random_spheres":
            pc = point_case(name)
            lo, hi = pc.lo, pc.hi
        else:
            lo, hi = Geometry(hs).box()
        _scenes[name] = (hs, HostsimHandle(hs, 4), box_points(lo, hi, 1000, 21))
    return _scenes[name]


def _mixed_beta(n):
    """A per-point mix of 1, 2, 3.5 and +inf."""
    return np.array([1.0, 2.0, np.inf, 3.5], np.float32)[np.arange(n) % 4]


def _np(t):
    return t.cpu().numpy()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("name", SCENES, ids=[s.replace("case:", "") for s in SCENES])
def test_device_is_the_cpu_mirrors_bits(ctx, name, fmt):
    """Whole buffers at beta 1, 2, +inf and a per-point mix, on the host path and the tensor path, with option "node_format" 64 and 128:
    the walk reads references and moments alone, so the setting changes nothing."""
    import torch
    hs, sim, pts = _scene(name)
    _load(ctx, hs, fmt)
    for beta in (1.0, 2.0, INF, _mixed_beta(len(pts))):
        want = windingsim(sim, pts, beta)
        got = ctx.query_winding(pts, beta)
        assert got.dtype == np.float32 and got.shape == (len(pts),)
        assert same_bits(got, want), (name, fmt, beta if np.ndim(beta) == 0 else "mix", np.where(got.view(np.uint32) != want.view(np.uint32))[0][:8])
    q = rows(pts, _mixed_beta(len(pts)))
    want = windingsim(sim, q)
    t3 = torch.from_numpy(pts).to("cuda:0")
    t4 = torch.from_numpy(q).to("cuda:0")
    for t in (ctx.query_winding(t4), ctx.query_winding(t3, torch.from_numpy(q[:, 3].copy()).to("cuda:0"))):
        assert t.is_cuda and t.dtype == torch.float32 and same_bits(_np(t), want)
    assert same_bits(ctx.query_winding(q), want)                      # (n, 4) rows on the host path
    inside = ctx.inside(pts, 2.0)
    assert inside.dtype == np.bool_ and (inside == (windingsim(sim, pts, 2.0) > 0.5)).all()
    ti = ctx.inside(t3, 2.0)
    assert ti.is_cuda and ti.dtype == torch.bool and (_np(ti) == inside).all()
    if name == "uv_sphere":
        r = np.linalg.norm(pts.astype(np.float64), axis=1)
        assert inside[r < 0.95].all() and not inside[r > 1.05].any() and inside.any() and not inside.all()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_small_batches(ctx, n):
    hs, sim, pts = _scene("uv_sphere")
    _load(ctx, hs)
    q = rows(pts[:n], _mixed_beta(n))
    assert same_bits(ctx.query_winding(q), windingsim(sim, q))


@pytest.mark.timeout(300)
def test_deep_tree_spills_the_lds_stack(ctx):
    """Leaf size 1 on the UV sphere: the walk holds more entries than the lane's LDS part, so the overflow column is written and read."""
    hs, _, pts = _scene("uv_sphere")
    sim = HostsimHandle(hs, 1)
    _load(ctx, hs, leaf_size=1)
    q = rows(pts, _mixed_beta(len(pts)))
    assert winding_work(sim, q, None)[2].max() > LDS_ENTRIES
    assert same_bits(ctx.query_winding(q), windingsim(sim, q))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["uv_sphere", "case:mixed", "cube"], ids=["uv_sphere", "mixed", "cube"])
def test_device_table_is_the_mirrors(ctx, name):
    hs, sim, _ = _scene(name)
    _load(ctx, hs)
    want = winding_table(sim)
    info = ctx.winding_info()
    assert info["nodes"] == len(want) and info["stale"] == 1 and info["tableBytes"] == 0
    got = ctx.winding_table_read()
    assert got.shape == want.shape and same_words(got, want)
    info = ctx.winding_info()
    assert info["stale"] == 0 and info["tableBytes"] >= 128 * len(want)


@pytest.mark.timeout(300)
def test_table_is_rebuilt_after_a_refit_and_after_a_build_and_not_otherwise(ctx):
    hs, sim, pts = _scene("uv_sphere")
    _load(ctx, hs)
    q = rows(pts, 2.0)
    builds = ctx.winding_info()["tableBuilds"]
    before = ctx.query_winding(q)
    assert same_bits(before, windingsim(sim, q)) and ctx.winding_info()["tableBuilds"] == builds + 1
    ctx.query_winding(q)
    assert ctx.winding_info()["tableBuilds"] == builds + 1 and ctx.winding_info()["stale"] == 0
    fp, moved = moved_faces(hs, 0.05)
    ctx.update_faces(0, moved)
    assert ctx.winding_info()["stale"] == 1
    with pytest.raises(M.MoptixError) as e:
        ctx.query_winding(q)
    assert e.value.code == K.ERR_STATE                          # faces dirty
    import torch
    with pytest.raises(M.MoptixError) as e:
        ctx.query_winding(torch.from_numpy(q).to("cuda:0"))
    assert e.value.code == K.ERR_STATE
    assert ctx.winding_info()["tableBuilds"] == builds + 1
    ctx.refit_accel()
    rs = RefitSim(hs, 4)
    try:
        rs.update(0, fp); rs.refit()
        want = windingsim(rs._sim, q)
        after = ctx.query_winding(q)
        assert same_bits(after, want) and not same_bits(after, before)
        assert ctx.winding_info()["tableBuilds"] == builds + 2
        assert same_bits(ctx.query_winding(q), want) and ctx.winding_info()["tableBuilds"] == builds + 2
        assert same_words(ctx.winding_table_read(), winding_table(rs._sim)) and ctx.winding_info()["tableBuilds"] == builds + 2
    finally:
        rs.close()
    ctx.build_accel(hs.accel)                                           # a rebuild drops the table with the tree
    info = ctx.winding_info()
    assert info["stale"] == 1 and info["tableBytes"] == 0 and info["tableBuilds"] == builds + 2
    ctx.query_winding(q)
    assert ctx.winding_info()["tableBuilds"] == builds + 3 and ctx.winding_info()["stale"] == 0


@pytest.mark.timeout(300)
def test_argument_errors_empty_batch_and_empty_scene(ctx):
    import torch
    hs, sim, pts = _scene("cube")
    _load(ctx, hs)
    L, h = K.device_lib(), ctx._h
    q = rows(pts[:4], 2.0)
    out = np.full(4, 7.0, np.float32)
    qp, op = q.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float))
    assert L.moptix_query_winding(h, qp, 4, op) == K.MOPTIX_OK and same_bits(out, windingsim(sim, q))
    out[:] = 7.0
    assert L.moptix_query_winding(h, qp, 0, op) == K.MOPTIX_OK and (out == 7.0).all()          # n = 0: a no-op
    assert L.moptix_query_winding(h, None, 0, None) == K.MOPTIX_OK
    assert L.moptix_query_winding(h, qp, -1, op) == K.ERR_INVALID
    assert L.moptix_query_winding(h, None, 4, op) == K.ERR_INVALID
    assert L.moptix_query_winding(h, qp, 4, None) == K.ERR_INVALID
    assert L.moptix_query_winding(None, qp, 4, op) == K.ERR_INVALID
    assert L.moptix_get_winding_info(h, None) == K.ERR_INVALID and L.moptix_get_winding_info(None, None) == K.ERR_INVALID
    dev = torch.device("cuda", 0)
    dq = torch.from_numpy(np.concatenate([q, q[:1]])).to(dev)
    do = torch.zeros(8, dtype=torch.float32, device=dev)
    vp = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    assert L.moptix_query_winding_device(h, vp(dq), 4, vp(do)) == K.MOPTIX_OK
    ctx.sync()
    assert same_bits(_np(do)[:4], windingsim(sim, q))
    assert L.moptix_query_winding_device(h, vp(dq, 16), 4, vp(do, 4)) == K.MOPTIX_OK          # 16 and 4 bytes are all they need
    ctx.sync()
    for o in (4, 8, 12):
        assert L.moptix_query_winding_device(h, vp(dq, o), 4, vp(do)) == K.ERR_INVALID          # a misaligned pointer
    assert L.moptix_query_winding_device(h, vp(dq), 4, vp(do, 2)) == K.ERR_INVALID              # misaligned results
    assert L.moptix_query_winding_device(h, None, 4, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_winding_device(h, vp(dq), 4, None) == K.ERR_INVALID
    assert L.moptix_query_winding_device(h, vp(dq), -1, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_winding_device(h, vp(dq), 0, vp(do)) == K.MOPTIX_OK
    assert ctx.query_winding(np.zeros((0, 3), np.float32)).shape == (0,)
    for bad in (np.zeros((4, 2), np.float32), np.zeros(12, np.float32)):
        with pytest.raises(ValueError):
            ctx.query_winding(bad)
    for bad in (dq[:4, :2], dq[:4].cpu(), dq[:4].double()):
        with pytest.raises(ValueError):
            ctx.query_winding(bad)
    # invalid rows on the device
    bad = np.array([[np.nan, 0, 0, 2], [0, np.inf, 0, 2], [0, 0, 0, 0.5], [0, 0, 0, np.nan], [0, 0, 0, -1], [0, 0, 0, 1]], np.float32)
    got = ctx.query_winding(bad)
    assert (got[:5].view(np.uint32) == QNAN).all() and same_bits(got, windingsim(sim, bad)) and np.isfinite(got[5])
    fresh = M.Context(0)
    try:
        assert L.moptix_query_winding(fresh._h, qp, 4, op) == K.ERR_STATE      # no params, no tree
        assert L.moptix_query_winding_device(fresh._h, vp(dq), 4, vp(do)) == K.ERR_STATE
        assert fresh.winding_info() == dict(tableBuilds=0, nodes=0, tableBytes=0, stale=1)
    finally:
        fresh.close()
    # an empty scene: zeros, and no table
    mesh_scene(np.zeros((0, 3, 3), np.float32)).upload(ctx)      # not load(): moptix_validate refuses a scene without geometry, the queries do not
    got = ctx.query_winding(pts[:65], 2.0)
    assert (got.view(np.uint32) == 0).all() and ctx.winding_info()["tableBytes"] == 0
    # a root that is a leaf
    one = mesh_scene(cube()[:1])
    _load(ctx, one)
    assert same_bits(ctx.query_winding(pts[:65], 1.0), windingsim(HostsimHandle(one, 4), pts[:65], 1.0))


def test_kernel_resources_of_the_shipped_code_objects():
    """No spilled registers and no scratch in pt_windingquery and k_winding_level, and the 16 KB of LDS of the stack."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec); spec.loader.exec_module(kr)
    res = {k: v for k, v in kr.kernel_resources(os.path.join(REPO, "minimaloptix_amd", "lib", "libmoptix.so")).items() if "winding" in k}
    assert len(res) == 2, sorted(res)
    for name, r in sorted(res.items()):
        print("%s %s" % (name, r))
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["vgpr_count"] <= 128 and r["group_segment_fixed_size"] == (16384 if "pt_windingquery" in name else 0), (name, r)


# ---- stream order: the _device entry behind a busy stream ----
@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream(torch.device("cuda", 0))


@pytest.mark.timeout(120)
def test_device_entry_is_ordered_behind_a_busy_stream(ctx, stream):
    """moptix_query_winding_device on a caller's stream that is busy: the staged points hold the poison (every float NaN: an invalid row,
    the quiet NaN) until a copy queued behind the delay brings the real ones, the output holds 0xA5 until the kernel writes it and a clone
    queued behind the call reads it.  The call returns while the delay is running; the clone holds the host path's bits.  The table and
    the plan exist before the stream is busy (a warm call): making the plan reads the nodes back once per built tree."""
    import torch
    hs, sim, pts = _scene("uv_sphere")
    _load(ctx, hs)
    real_np = rows(pts[np.arange(N) % len(pts)], _mixed_beta(N))
    want = ctx.query_winding(real_np)
    assert same_bits(want, windingsim(sim, real_np))
    poison_np = np.full((N, 4), np.nan, np.float32)
    assert (ctx.query_winding(poison_np).view(np.uint32) == QNAN).all() and np.isfinite(want).all()
    dev = torch.device("cuda", 0)
    real, bad = torch.from_numpy(real_np).to(dev), torch.from_numpy(poison_np).to(dev)
    staged = torch.empty_like(real)
    out = torch.empty(N, dtype=torch.float32, device=dev)
    ctx.query_winding(real[:256].contiguous())                  # a warm call: table, plan and overflow area exist before the stream is busy
    builds = ctx.winding_info()["tableBuilds"]
    ctx.set_stream(stream.cuda_stream)
    L, h, vp = K.device_lib(), ctx._h, lambda t: C.c_void_p(t.data_ptr())
    rc, free = [], []

    def call():
        free.append(torch.cuda.mem_get_info(dev))
        rc.append(L.moptix_query_winding_device(h, vp(staged), N, vp(out)))
        free.append(torch.cuda.mem_get_info(dev))
    clone, pending = behind_busy_stream(ctx, stream, lambda: staged.copy_(real), call, lambda: out.clone(), staged=[(staged, bad)], outputs=[out])
    assert rc == [K.MOPTIX_OK], ctx.last_error()
    assert pending, "the call waited for the stream"
    assert free[0] == free[1], "a warm call allocated or freed device memory"
    assert ctx.winding_info()["tableBuilds"] == builds
    assert same_bits(_np(clone), want)
    # Context.query_winding on a tensor with torch's current stream the context's: ordered on that stream, no wait on the host
    staged.copy_(bad)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        delay = busy(stream)
        staged.copy_(real)
        t = ctx.query_winding(staged)
        pending = not delay.query()
    stream.synchronize()
    assert pending, "the wrapper waited for the stream"
    assert t.is_cuda and same_bits(_np(t), want)
