"""Triangle queries on the MI355X (trikernel.hip pt_triquery): bit for bit the CPU mirror of the kernel's code (tests/trisim/trisim.cpp),
whole buffers -- any, count, the CSR list and the fixed-capacity list -- on the host path and the tensor path; the capped grid; after a
refit; the two asynchronous entries behind a busy stream; the family's stack overflow area; Context.self_intersections."""
import ctypes as C

import numpy as np
import pytest

from common import M, HostsimHandle
from point_helpers import Geometry, point_case
from query_helpers import coffee_rays
from refit_helpers import RefitSim, moved_faces
from sign_helpers import mesh_scene
from stream_helpers import N, all_same_bits, behind_busy_stream, poison_differs
from tri_helpers import MirrorContext, csr, mesh_hs, pushed_torus, same_bits, tri_sets, trisim, trisim_list

pytestmark = pytest.mark.gpu
K = M._capi
COFFEE = "file:coffee"
LDS_ENTRIES = 16                       # trikernel.hip kLdsStack: the stack entries a lane keeps in LDS


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_stream(0)
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0)
    gpu_ctx.set_option("query_blocks_per_cu", 32)


def _load(ctx, hs, node_format=0, leaf=4):
    ctx.set_option("node_format", node_format); ctx.set_option("leaf_size", leaf)
    ctx.load(hs)


_scenes = {}


def _scene(name):
    """(scene, geometry, lo, hi, queries, parts) of "torus" or coffee, made once: tri_helpers.tri_sets, about 1,600 queries."""
    if name not in _scenes:
        if name == "torus":
            hs = mesh_scene("torus")
            geo = Geometry(hs)
            lo, hi = geo.box()
        else:
            pc = point_case(name)
            hs, geo, lo, hi = pc.hs, pc.geo, pc.lo, pc.hi
        _scenes[name] = (hs, geo, lo, hi) + tri_sets(geo, lo, hi)
    return _scenes[name]


_mirrors = {}


def _mirror(name, leaf):
    if (name, leaf) not in _mirrors:
        _mirrors[(name, leaf)] = point_case(name).sim if (name == COFFEE and leaf == 4) else HostsimHandle(_scene(name)[0], leaf)
    return _mirrors[(name, leaf)]


def _np(t):
    return t.cpu().numpy()


# ---- 1: the mirror's bits ----
@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", [0, 64, 128])
@pytest.mark.parametrize("leaf", [1, 4, 8])
@pytest.mark.parametrize("name", ["torus", COFFEE], ids=["torus", "coffee"])
def test_device_is_the_cpu_mirrors_bits(ctx, name, leaf, fmt):
    """Coffee is here for the overflow columns (its tree is deeper than the LDS part of the stack) and its quads.  Option node_format 0
    walks the 64-byte nodes where the tree has them, as 64 does."""
    import torch
    hs, _, _, _, b, parts = _scene(name)
    sim = _mirror(name, leaf)
    _load(ctx, hs, fmt, leaf)
    mfmt = 128 if fmt == 128 else 64
    n = len(b)
    want_any, want_c = trisim(sim, b, "any", mfmt), trisim(sim, b, "count", mfmt)
    want_p = trisim_list(sim, b, csr(want_c), mfmt)[0]
    cap = 2
    fixed = np.arange(n + 1, dtype=np.int64) * cap
    want_fp, want_fc = trisim_list(sim, b, fixed, mfmt)
    assert (want_c > cap).any() and ((want_c > 0) & (want_c < cap)).sum() > 20 and (want_c == 0).sum() > 20
    tb = torch.from_numpy(b).to("cuda:0")
    for mode, want in (("any", want_any), ("count", want_c)):
        got = ctx.query_tris(b, mode)
        assert got.dtype == np.int32 and got.shape == (n,) and same_bits(got, want), (mode, np.where(got != want)[0][:8])
        t = ctx.query_tris(tb, mode)
        assert t.is_cuda and t.dtype == torch.int32 and same_bits(_np(t), want), mode
    prims, offsets = ctx.query_tris(b, "list")
    assert prims.dtype == np.int32 and offsets.dtype == np.int64 and same_bits(offsets, csr(want_c)) and same_bits(prims, want_p)
    tp, to = ctx.query_tris(tb, "list")
    assert same_bits(_np(to), csr(want_c)) and same_bits(_np(tp), want_p)
    fp, fc = ctx.query_tris(b, "list", max_prims=cap)
    assert fp.shape == (n, cap) and same_bits(fc, want_c) and same_bits(fc, want_fc) and same_bits(fp.reshape(-1), want_fp)
    assert (fp[want_c > cap] == -1).all()
    assert not want_c[parts["invalid"]].any()


# ---- 2: the capped grid ----
@pytest.mark.timeout(300)
def test_capped_grid_walks_several_queries_per_lane(ctx):
    """One workgroup per CU and more queries than that grid has lanes, with a partial last block: lanes walk a second query through the
    same stack columns, on a tree deeper than the LDS part of the stack, so the overflow columns of the capped grid are in use.  The
    mirror's bits, and the bits at the default grid.  The grid cannot be capped below one workgroup per CU, hence the number of queries;
    they are small triangles."""
    hs, geo, lo, hi, sets, parts = _scene(COFFEE)
    sim = _mirror(COFFEE, 4)
    _load(ctx, hs)
    assert 3 * ctx.accel_info().treeDepth + 1 > LDS_ENTRIES
    cus = ctx.get_option("num_cus")
    n = 256 * cus + 257
    assert cus > 256 or n == 65793
    rng = np.random.default_rng(37)
    diag = float(np.linalg.norm(hi - lo))
    c = np.concatenate([rng.uniform(lo, hi, (n - n // 4, 3)), geo.surface_points(rng, n // 4)])
    bl = (c[:, None, :] + (diag * 10.0 ** rng.uniform(-3.0, -1.7, (n, 1, 1))) * rng.normal(size=(n, 3, 3))).reshape(n, 9).astype(np.float32)
    b = bl.copy()
    b[-1] = sets[parts["whole"]]                                # any / count: the triangle that cuts the whole scene, in the partial last block
    want_c, want_lc = trisim(sim, b, "count"), trisim(sim, bl, "count")
    want_p = trisim_list(sim, bl, csr(want_lc))[0]
    assert (want_c > 8).sum() > 100 and (want_c == 0).sum() > 1000 and want_c[-1] > 0
    default = (ctx.query_tris(b, "any"), ctx.query_tris(b, "count"), ctx.query_tris(bl, "list"))
    ctx.set_option("query_blocks_per_cu", 1)
    capped = (ctx.query_tris(b, "any"), ctx.query_tris(b, "count"), ctx.query_tris(bl, "list"))
    for anyone, counts, (prims, offsets) in (capped, default):
        assert same_bits(counts, want_c) and same_bits(anyone, (want_c > 0).astype(np.int32))
        assert same_bits(offsets, csr(want_lc)) and same_bits(prims, want_p)


# ---- 3: after a refit ----
@pytest.mark.timeout(300)
def test_after_update_faces_and_refit(ctx):
    hs, _, _, _, b, _ = _scene(COFFEE)
    sim = _mirror(COFFEE, 4)
    _load(ctx, hs)
    before = ctx.query_tris(b, "count")
    assert same_bits(before, trisim(sim, b, "count"))
    fp, rows = moved_faces(hs, 0.02)
    ctx.update_faces(0, rows)
    for kw in (dict(mode="any"), dict(mode="count"), dict(mode="list"), dict(mode="list", max_prims=4)):
        with pytest.raises(M.MoptixError) as e:
            ctx.query_tris(b, **kw)
        assert e.value.code == K.ERR_STATE
    ctx.refit_accel()
    rs = RefitSim(hs, 4)
    try:
        rs.update(0, fp); rs.refit()
        want_c = trisim(rs._sim, b, "count")
        assert same_bits(ctx.query_tris(b, "count"), want_c) and same_bits(ctx.query_tris(b, "any"), trisim(rs._sim, b, "any"))
        prims, offsets = ctx.query_tris(b, "list")
        assert same_bits(offsets, csr(want_c)) and same_bits(prims, trisim_list(rs._sim, b, csr(want_c))[0])
        assert not same_bits(want_c, before)                    # the move changed the answer
    finally:
        rs.close()


# ---- 4: the torch path ----
@pytest.mark.timeout(300)
def test_tensor_path_reads_in_place_and_answers_on_the_device(ctx):
    import torch
    hs, _, _, _, b, _ = _scene("torus")
    _load(ctx, hs)
    want_c = trisim(hs, b, "count")
    n = len(b)
    dev = torch.device("cuda", 0)
    flat = torch.from_numpy(b).to(dev)
    folded = flat.view(n, 3, 3)
    for t in (flat, folded):
        before = t.clone()
        c = ctx.query_tris(t, "count")
        assert c.device == t.device and c.dtype == torch.int32 and same_bits(_np(c), want_c)
        assert same_bits(_np(ctx.query_tris(t, "any")), (want_c > 0).astype(np.int32))
        prims, offsets = ctx.query_tris(t, "list")
        assert prims.is_cuda and offsets.is_cuda and prims.dtype == torch.int32 and offsets.dtype == torch.int64
        assert same_bits(_np(offsets), csr(want_c)) and same_bits(_np(prims), trisim_list(hs, b, csr(want_c))[0])
        fp, fc = ctx.query_tris(t, "list", max_prims=3)
        want_fp, want_fc = trisim_list(hs, b, np.arange(n + 1, dtype=np.int64) * 3)
        assert tuple(fp.shape) == (n, 3) and fp.is_cuda and same_bits(_np(fc), want_fc) and same_bits(_np(fp).reshape(-1), want_fp)
        assert same_bits(_np(t), _np(before))                   # the queries were only read (bits: the invalid ones hold NaNs)
    # read where it is: a view into a larger tensor at an offset of 36 bytes, not a copy of it
    room = torch.zeros(9 * (n + 1), dtype=torch.float32, device=dev)
    room[9:] = flat.reshape(-1)
    view = room[9:].view(n, 9)
    assert view.data_ptr() == room.data_ptr() + 36 and same_bits(_np(ctx.query_tris(view, "count")), want_c)
    for bad in (flat[:, :8], flat.cpu(), flat.double(), flat.reshape(-1), folded.transpose(1, 2), flat[::2]):
        with pytest.raises(ValueError):
            ctx.query_tris(bad, "count")
    assert len(ctx.query_tris(np.zeros((0, 9), np.float32), "count")) == 0
    ep, eo = ctx.query_tris(np.zeros((0, 3, 3), np.float32), "list")
    assert len(ep) == 0 and same_bits(eo, np.zeros(1, np.int64))
    L = K.device_lib()
    assert L.moptix_query_tris(ctx._h, None, 0, K.BOX_ANY, None) == K.MOPTIX_OK
    assert L.moptix_query_tris_device(ctx._h, None, 0, K.BOX_COUNT, None) == K.MOPTIX_OK
    assert L.moptix_query_tris_list(ctx._h, None, 0, None, None, None) == K.MOPTIX_OK
    assert L.moptix_query_tris_list_device(ctx._h, None, 0, None, None, None) == K.MOPTIX_OK
    vp = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    out = torch.zeros(8, dtype=torch.int32, device=dev)
    assert L.moptix_query_tris_device(ctx._h, vp(flat, 2), 4, K.BOX_COUNT, vp(out)) == K.ERR_INVALID         # misaligned queries
    assert L.moptix_query_tris_device(ctx._h, vp(flat), 4, K.BOX_COUNT, vp(out, 2)) == K.ERR_INVALID         # misaligned results
    assert L.moptix_query_tris_device(ctx._h, vp(flat), 4, 2, vp(out)) == K.ERR_INVALID                      # an unknown mode
    assert L.moptix_query_tris_device(ctx._h, vp(flat), -1, K.BOX_ANY, vp(out)) == K.ERR_INVALID


@pytest.mark.timeout(300)
def test_self_intersections_on_the_device(ctx):
    """The pairs of the pushed torus (tests/test_tri_cpu.py checks them against the exact evaluation) from the mirror behind the stub, from
    the host path and from tensors (the id of face 0 in a scene with quads in front of the faces: the overflow-area test, on coffee)."""
    import torch
    v, f = pushed_torus(2.2)
    hs = mesh_hs(v, f)
    want = MirrorContext(M, hs).self_intersections(v, f)
    assert len(want) >= 8
    _load(ctx, hs)
    got = ctx.self_intersections(v, f)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(ctx.self_intersections(v, f, max_prims=64), want)
    dev = torch.device("cuda", 0)
    t = ctx.self_intersections(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))
    assert t.is_cuda and t.dtype == torch.int64 and np.array_equal(_np(t), want)
    with pytest.raises(ValueError):
        ctx.self_intersections(v, f[:-1])                       # not the mesh the tree was built on


# ---- 5: stream order ----
@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream(torch.device("cuda", 0))


_async = {}


def _async_set(kind):
    """N valid queries of the scene (copies of its own faces, cyclically: most of them meet something), their poison -- every float NaN,
    invalid by the header's rule --, and per mode the blocking host path's results for both.  Made once, with the GPU idle."""
    if kind not in _async:
        b, parts = _scene(kind)[4:]
        src = b[parts["faces"].start:parts["own"].stop]
        _async[kind] = dict(real=np.ascontiguousarray(src[np.arange(N) % len(src)]), poison=np.full((N, 9), np.nan, np.float32), want={})
    return _async[kind]


def _expected(ctx, kind, mode):
    s = _async_set(kind)
    if mode not in s["want"]:
        def host(x):
            if mode != "list":
                return (ctx.query_tris(x, mode),)
            prims, offsets = ctx.query_tris(x, "list")
            return (np.diff(offsets).astype(np.int32), prims)
        s["want"][mode] = (host(s["real"]), host(s["poison"]))
    want, bad = s["want"][mode]
    poison_differs(bad[:1], want[:1], "%s tris %s" % (kind, mode))      # a quarter of the records differ: one record per query
    return want


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", ["any", "count", "list"])
@pytest.mark.parametrize("kind", [COFFEE, "torus"], ids=["coffee", "torus"])
def test_device_entries_are_ordered_behind_a_busy_stream(ctx, stream, kind, mode):
    """moptix_query_tris_device (any, count) and moptix_query_tris_list_device on a caller's stream that is busy: the staged queries hold
    the poison until a copy queued behind the delay brings the real ones, the outputs hold 0xA5 until the kernel writes them and a clone
    queued behind the call reads them.  The call returns while the delay is running; the clone holds the host path's bits."""
    import torch
    _load(ctx, _scene(kind)[0])
    want = _expected(ctx, kind, mode)
    s = _async_set(kind)
    dev = torch.device("cuda", 0)
    real, bad = torch.from_numpy(s["real"]).to(dev), torch.from_numpy(s["poison"]).to(dev)
    staged = torch.empty_like(real)
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    outs = [counts]
    if mode == "list":
        # the offsets of the expected counts, uploaded while the GPU is idle and never poisoned: the kernel writes where they point
        offsets = torch.from_numpy(csr(want[0])).to(dev)
        total = int(csr(want[0])[-1])
        prims = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        outs.append(prims)
    ctx.query_tris(real[:256].contiguous(), "count")            # a warm call: the overflow area exists before the stream is busy
    ctx.set_stream(stream.cuda_stream)
    L, h, vp = K.device_lib(), ctx._h, lambda t: C.c_void_p(t.data_ptr())
    rc, free = [], []

    def call():
        free.append(torch.cuda.mem_get_info(dev))
        if mode == "list":
            rc.append(L.moptix_query_tris_list_device(h, vp(staged), N, vp(offsets), vp(prims), vp(counts)))
        else:
            rc.append(L.moptix_query_tris_device(h, vp(staged), N, M.Context.BOX_MODES[mode], vp(counts)))
        free.append(torch.cuda.mem_get_info(dev))
    clones, pending = behind_busy_stream(ctx, stream, lambda: staged.copy_(real), call, lambda: [o.clone() for o in outs],
                                         staged=[(staged, bad)], outputs=outs)
    assert rc == [K.MOPTIX_OK], ctx.last_error()
    assert pending, "the call waited for the stream"
    assert free[0] == free[1], "a warm call allocated or freed device memory"
    got = (_np(clones[0]),) if mode != "list" else (_np(clones[0]), _np(clones[1])[:total])
    assert all_same_bits(got, want), [int((g != w).sum()) if g.shape == w.shape else "shape" for g, w in zip(got, want)]


# ---- 6: the family's overflow area, and the rest of the context ----
@pytest.mark.timeout(300)
def test_overflow_area_lives_with_the_tree_and_the_context_is_left_alone(ctx):
    """Coffee's tree is deeper than the LDS part of the stack, so the first triangle query allocates the family's overflow area: device
    memory goes down once, stays where it is over further queries and a refit, comes back with a rebuild and with clear_scene.  A ray, a
    point and a box query give the same bits before and after, and the ray queries' own area keeps its address."""
    import torch
    dev = torch.device("cuda", 0)
    free = lambda: (ctx.sync(), torch.cuda.mem_get_info(dev)[0])[1]
    pc = point_case(COFFEE)
    hs, _, _, _, sets, _ = _scene(COFFEE)
    _load(ctx, hs)
    assert 3 * ctx.accel_info().treeDepth + 1 > LDS_ENTRIES
    assert ctx._first_face_id(pc.geo.nt) == pc.geo.ns + pc.geo.nq == 3      # what self_intersections takes off the ids: coffee's three quads
    b = np.ascontiguousarray(sets[::4])
    tb = torch.from_numpy(b).to(dev)
    out = torch.zeros(len(b), dtype=torch.int32, device=dev)
    L, vp = K.device_lib(), lambda t: C.c_void_p(t.data_ptr())
    device_count = lambda: (L.moptix_query_tris_device(ctx._h, vp(tb), len(b), K.BOX_COUNT, vp(out)), ctx.sync(), _np(out).copy())
    q = np.ascontiguousarray(np.concatenate([pc.pts[::16], np.full((len(pc.pts[::16]), 1), np.inf, np.float32)], axis=1))
    boxes = np.ascontiguousarray(np.concatenate([pc.pts[::16] - 0.01, pc.pts[::16] + 0.01], axis=1), np.float32)
    rays = coffee_rays()
    closest, hits, aligned = ctx.query_points(q), ctx.query_rays(rays), ctx.query_boxes(boxes, "count")
    addr = ctx.debug_buffer_addresses()
    f0 = free()
    rc, _, counts = device_count()
    assert rc == K.MOPTIX_OK and same_bits(counts, trisim(pc.sim, b, "count"))
    f1 = free()
    area = f0 - f1
    assert area > 0, "the first triangle query on a deep tree allocates the overflow area"
    assert same_bits(device_count()[2], counts) and free() == f1                # a warm call allocates nothing
    assert ctx.debug_buffer_addresses() == addr
    assert same_bits(ctx.query_points(q), closest) and same_bits(ctx.query_rays(rays), hits) and same_bits(ctx.query_boxes(boxes, "count"), aligned)
    f1 = free()
    ctx.refit_accel()                                                           # nothing moved: the same tree, the same answers
    f2 = free()
    assert same_bits(device_count()[2], counts) and free() == f2, "the area did not survive the refit"
    ctx.build_accel("Lbvh")
    assert free() >= f2 + area // 2, "a rebuild drops the area"
    f3 = free()
    assert same_bits(device_count()[2], counts) and free() <= f3 - area // 2    # and the next query on the new tree allocates it again
    f4 = free()
    assert L.moptix_clear_scene(ctx._h) == K.MOPTIX_OK
    assert free() >= f4 + area // 2, "clear_scene drops the area"
    _load(ctx, hs)
    assert same_bits(device_count()[2], counts)
    assert same_bits(ctx.query_points(q), closest) and same_bits(ctx.query_rays(rays), hits) and same_bits(ctx.query_boxes(boxes, "count"), aligned)
