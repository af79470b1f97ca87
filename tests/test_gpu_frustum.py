"""Frustum queries on the MI355X (frustumkernel.hip pt_frustumquery): bit for bit the CPU mirror of the kernel's code
(tests/frustumsim/frustumsim.cpp), whole buffers -- any, count, the CSR list and the fixed-capacity list -- on the host path and the
tensor path; the capped grid, the overflow columns, the errors, the kernels' resources; and the two asynchronous entries behind a busy
stream."""
import ctypes as C
import os

import numpy as np
import pytest

import lbvh_cases
from common import M, HostsimHandle, REPO, hostsim_bvh
from frustum_helpers import (csr, frustum_sets, frustum_stack_depth, frustumsim, frustumsim_list, pack, perspective, random_rotations,
                             same_bits, scene_camera, tiles)
from point_helpers import point_case
from query_helpers import coffee_rays
from refit_helpers import RefitSim, moved_faces
from stream_helpers import N, all_same_bits, behind_busy_stream, poison_differs

pytestmark = pytest.mark.gpu
K = M._capi
COFFEE = "file:coffee"
SMALL = ["spheres", "cornell_quads", "random_spheres", "case:mixed", "case:counts_2049"]
LDS_ENTRIES = 16                       # frustumkernel.hip kLdsStack: the stack entries a lane keeps in LDS


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_stream(0)
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0)
    gpu_ctx.set_option("query_blocks_per_cu", 32)


def _load(ctx, hs, node_format=0, leaf_size=4):
    ctx.set_option("node_format", node_format); ctx.set_option("leaf_size", leaf_size)
    ctx.load(hs)


_sets = {}


def _frusta(name):
    """The scene's frustum set (frustum_helpers.frustum_sets, about 900 queries) and its parts."""
    if name not in _sets:
        pc = point_case(name)
        _sets[name] = frustum_sets(pc.hs, pc.geo, pc.lo, pc.hi)
    return _sets[name]


def _np(t):
    return t.cpu().numpy()


def _whole_buffers(ctx, sim, b, fmt, leaf=4, cap=2):
    """Every mode on the host path and the tensor path against the mirror's bytes."""
    import torch
    n = len(b)
    want_any, want_c = frustumsim(sim, b, "any", fmt, leaf), frustumsim(sim, b, "count", fmt, leaf)
    want_p = frustumsim_list(sim, b, csr(want_c), fmt, leaf)[0]
    fixed = np.arange(n + 1, dtype=np.int64) * cap
    want_fp, want_fc = frustumsim_list(sim, b, fixed, fmt, leaf)
    tb = torch.from_numpy(b).to("cuda:0")
    for mode, want in (("any", want_any), ("count", want_c)):
        got = ctx.query_frusta(b, mode)
        assert got.dtype == np.int32 and got.shape == (n,) and same_bits(got, want), (mode, np.where(got != want)[0][:8])
        t = ctx.query_frusta(tb, mode)
        assert t.is_cuda and t.dtype == torch.int32 and same_bits(_np(t), want), mode
    prims, offsets = ctx.query_frusta(b, "list")
    assert prims.dtype == np.int32 and offsets.dtype == np.int64 and same_bits(offsets, csr(want_c)) and same_bits(prims, want_p)
    tp, to = ctx.query_frusta(tb, "list")
    assert tp.is_cuda and tp.dtype == torch.int32 and to.dtype == torch.int64
    assert same_bits(_np(to), csr(want_c)) and same_bits(_np(tp), want_p)
    fp, fc = ctx.query_frusta(b, "list", max_prims=cap)
    assert fp.shape == (n, cap) and same_bits(fc, want_c) and same_bits(fc, want_fc) and same_bits(fp.reshape(-1), want_fp)
    assert (fp[want_c > cap] == -1).all()
    tfp, tfc = ctx.query_frusta(tb, "list", max_prims=cap)
    assert tuple(tfp.shape) == (n, cap) and same_bits(_np(tfc), want_c) and same_bits(_np(tfp).reshape(-1), want_fp)
    zp, zc = ctx.query_frusta(b, "list", max_prims=0)
    assert zp.shape == (n, 0) and same_bits(zc, want_c)
    return want_c


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("name", SMALL, ids=[s.replace("case:", "") for s in SMALL])
def test_device_is_the_cpu_mirrors_bits(ctx, name, fmt):
    """The scene's whole set (about 900 queries: camera tiles, perspective frusta, beams, wedges, slabs, half-spaces, thin, empty, zero,
    scaled and invalid ones) in every mode on both paths; an (n, 6, 4) array is taken too."""
    pc = point_case(name)
    _load(ctx, pc.hs, fmt)
    b = _frusta(name)[0]
    assert 257 < len(b) <= 4096
    want_c = _whole_buffers(ctx, pc.sim, b, fmt)
    assert (want_c > 2).any() and ((want_c > 0) & (want_c <= 2)).sum() > 5 and (want_c == 0).sum() > 20
    assert same_bits(ctx.query_frusta(b.reshape(-1, 6, 4), "count"), want_c)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [1, 255, 257])
def test_small_batches(ctx, n):
    pc = point_case("case:mixed")
    _load(ctx, pc.hs)
    b, parts = _frusta("case:mixed")
    b = np.ascontiguousarray(b[parts["persp"]][:n])
    _whole_buffers(ctx, pc.sim, b, 64)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("leaf", [1, 8])
def test_leaf_sizes(ctx, leaf):
    pc = point_case("case:mixed")
    _load(ctx, pc.hs, 0, leaf)
    assert ctx.accel_info().maxLeafSize == leaf
    sim = HostsimHandle(pc.hs, leaf)
    try:
        for fmt in (64, 128):
            _load(ctx, pc.hs, fmt, leaf)
            _whole_buffers(ctx, sim, _frusta("case:mixed")[0], fmt, leaf)
    finally:
        sim.close()


@pytest.mark.timeout(300)
def test_empty_batch(ctx):
    hs = M.HostScene("spheres", 64, 36)
    _load(ctx, hs)
    assert len(ctx.query_frusta(np.zeros((0, 24), np.float32), "count")) == 0
    ep, eo = ctx.query_frusta(np.zeros((0, 24), np.float32), "list")
    assert len(ep) == 0 and same_bits(eo, np.zeros(1, np.int64))
    L, h = K.device_lib(), ctx._h
    assert L.moptix_query_frusta(h, None, 0, K.BOX_ANY, None) == K.MOPTIX_OK
    assert L.moptix_query_frusta_device(h, None, 0, K.BOX_COUNT, None) == K.MOPTIX_OK
    assert L.moptix_query_frusta_list(h, None, 0, None, None, None) == K.MOPTIX_OK
    assert L.moptix_query_frusta_list_device(h, None, 0, None, None, None) == K.MOPTIX_OK


@pytest.mark.timeout(300)
def test_capped_grid_walks_several_queries_per_lane(ctx):
    """One workgroup per CU and 256 x CUs + 257 queries -- the smallest batch that makes the grid-stride loop take a second pass, with a
    partial last block: lanes walk a second query through the same stack columns, on a tree deeper than the LDS part of the stack.  The
    mirror's bits, and the bits at the default grid.  Small frusta, so that the lists stay short."""
    pc = point_case(COFFEE)
    _load(ctx, pc.hs)
    assert 3 * ctx.accel_info().treeDepth + 1 > LDS_ENTRIES
    cus = ctx.get_option("num_cus")
    n = 256 * cus + 257
    rng = np.random.default_rng(37)
    diag = float(np.linalg.norm(pc.hi - pc.lo))
    far = diag * 10.0 ** rng.uniform(-3.0, -1.5, n)
    tan = np.tan(np.radians(rng.uniform(2.0, 30.0, (n, 2))))
    bl = pack(perspective(rng.uniform(pc.lo, pc.hi, (n, 3)), random_rotations(rng, n), tan[:, 0], tan[:, 1], 0.1 * far, far))
    b = bl.copy()
    b[-1] = 0.0                                                   # any / count: six zero planes, the deepest walk, in the partial last block
    want_c, want_lc = frustumsim(pc.sim, b, "count"), frustumsim(pc.sim, bl, "count")
    want_p = frustumsim_list(pc.sim, bl, csr(want_lc))[0]
    assert (want_c > 16).sum() > 30 and (want_c == 0).sum() > 1000 and want_c[-1] > 100000 and want_lc.max() < 20000
    default = (ctx.query_frusta(b, "any"), ctx.query_frusta(b, "count"), ctx.query_frusta(bl, "list"))
    ctx.set_option("query_blocks_per_cu", 1)
    capped = (ctx.query_frusta(b, "any"), ctx.query_frusta(b, "count"), ctx.query_frusta(bl, "list"))
    for anyone, counts, (prims, offsets) in (capped, default):
        assert same_bits(counts, want_c) and same_bits(anyone, (want_c > 0).astype(np.int32))
        assert same_bits(offsets, csr(want_lc)) and same_bits(prims, want_p)


@pytest.mark.timeout(300)
def test_region_that_meets_everything_spills_the_stack(ctx):
    """The lbvh_cases mesh whose tree has the largest stack bound -- three of them share it: the two geometric chains, whose walk never
    holds more than 3 entries, and `mixed`, which is taken: the mirror's walk holds 49 there --, and regions that meet every primitive
    (six zero planes; a half-space that holds the mesh): the walk visits every node, the stack goes past its 16 LDS entries into the
    overflow columns."""
    depth = {}
    for name in lbvh_cases.CASE_NAMES:
        depth[name] = hostsim_bvh(point_case("case:" + name).sim)[4]
    deepest = [name for name in depth if depth[name] == max(depth.values())]
    name = max(deepest, key=lambda k: frustum_stack_depth(point_case("case:" + k).sim, np.zeros((1, 24), np.float32), "count"))
    pc = point_case("case:" + name)
    assert 3 * depth[name] + 1 > LDS_ENTRIES
    zero = np.zeros((1, 6, 4))
    half = zero.copy(); half[0, 0] = [1.0, 0.0, 0.0, 1.0 - float(pc.lo[0])]
    b = np.repeat(pack(np.concatenate([zero, half])), 130, axis=0)
    n_prims = pc.geo.ns + pc.geo.nq + pc.geo.nt
    for fmt in (64, 128):
        _load(ctx, pc.hs, fmt)
        assert frustum_stack_depth(pc.sim, b[:2], "count", fmt) > LDS_ENTRIES
        counts = ctx.query_frusta(b, "count")
        assert (counts == n_prims).all() and same_bits(counts, frustumsim(pc.sim, b, "count", fmt))
        prims, offsets = ctx.query_frusta(b[:4], "list")
        assert same_bits(prims, np.tile(np.arange(n_prims, dtype=np.int32), 4)) and same_bits(offsets, csr(counts[:4]))


@pytest.mark.timeout(300)
def test_after_update_faces_and_refit(ctx):
    pc = point_case(COFFEE)
    _load(ctx, pc.hs)
    b, parts = _frusta(COFFEE)
    b = np.ascontiguousarray(np.concatenate([b[parts["tiles"]], b[parts["persp"]], b[parts["beams"]], b[parts["thin"]]]))
    b = np.ascontiguousarray(b[frustumsim(pc.sim, b, "count") <= 20000])      # one lane sorts one list: the long ones are left to any / count elsewhere
    before = ctx.query_frusta(b, "count")
    assert same_bits(before, frustumsim(pc.sim, b, "count"))
    fp, rows = moved_faces(pc.hs, 0.02)
    ctx.update_faces(0, rows)
    for kw in (dict(mode="any"), dict(mode="count"), dict(mode="list"), dict(mode="list", max_prims=4)):
        with pytest.raises(M.MoptixError) as e:
            ctx.query_frusta(b, **kw)
        assert e.value.code == K.ERR_STATE                         # faces dirty
    ctx.refit_accel()
    rs = RefitSim(pc.hs, 4)
    try:
        rs.update(0, fp); rs.refit()
        want_c = frustumsim(rs._sim, b, "count")
        assert same_bits(ctx.query_frusta(b, "count"), want_c) and same_bits(ctx.query_frusta(b, "any"), frustumsim(rs._sim, b, "any"))
        prims, offsets = ctx.query_frusta(b, "list")
        assert same_bits(offsets, csr(want_c)) and same_bits(prims, frustumsim_list(rs._sim, b, csr(want_c))[0])
        assert not same_bits(want_c, before)                    # the move changed the answer
    finally:
        rs.close()


@pytest.mark.timeout(300)
def test_camera_tiles_on_coffee_in_both_node_formats(ctx):
    """camera_frusta on the renderer's camera, whole frame and 8 x 8 tiles, any and count on the deep tree (the whole frame meets tens of
    thousands of faces: count alone)."""
    pc = point_case(COFFEE)
    cam = scene_camera(pc.hs)
    b = np.concatenate([M.camera_frusta(cam, [[0, 0, 1, 1]]), M.camera_frusta(cam, tiles(8)), M.camera_frusta(pc.hs.params.cam, tiles(4), 0.5, 3.0)])
    for fmt in (64, 128):
        _load(ctx, pc.hs, fmt)
        want = frustumsim(pc.sim, b, "count", fmt)
        assert want[0] > 10000
        assert same_bits(ctx.query_frusta(b, "count"), want) and same_bits(ctx.query_frusta(b, "any"), (want > 0).astype(np.int32))


@pytest.mark.timeout(300)
def test_leaves_the_context_alone(ctx):
    pc = point_case(COFFEE)
    _load(ctx, pc.hs)
    b = _frusta(COFFEE)[0][_frusta(COFFEE)[1]["persp"]]
    q = np.ascontiguousarray(np.concatenate([pc.pts[::16], np.full((len(pc.pts[::16]), 1), np.inf, np.float32)], axis=1))
    boxes = np.ascontiguousarray(np.concatenate([pc.pts[::16] - 0.01, pc.pts[::16] + 0.01], axis=1), np.float32)
    rays = coffee_rays()
    closest = ctx.query_points(q)
    hits = ctx.query_rays(rays)
    aligned = ctx.query_boxes(boxes, "count")
    addr = ctx.debug_buffer_addresses()
    assert addr["query_overflow"] != 0
    counts = ctx.query_frusta(b, "count")
    ctx.query_frusta(b, "any"); ctx.query_frusta(b, "list", max_prims=4)
    assert ctx.debug_buffer_addresses() == addr                  # moptix_debug_buffer_addresses is unchanged by a frustum query
    assert same_bits(ctx.query_points(q), closest) and same_bits(ctx.query_rays(rays), hits) and same_bits(ctx.query_boxes(boxes, "count"), aligned)
    ctx.refit_accel()                                           # keeps the frustum queries' overflow area with the others
    assert ctx.debug_buffer_addresses()["query_overflow"] == addr["query_overflow"] and same_bits(ctx.query_frusta(b, "count"), counts)


@pytest.mark.timeout(300)
def test_argument_errors(ctx):
    import torch
    hs = M.HostScene("spheres", 64, 36)
    _load(ctx, hs)
    L, h = K.device_lib(), ctx._h
    b = np.zeros((4, 24), np.float32)
    out, prims, off = np.zeros(4, np.int32), np.zeros(16, np.int32), np.arange(5, dtype=np.int64) * 4
    bp, op, pp = b.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_int32)), prims.ctypes.data_as(C.POINTER(C.c_int32))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.moptix_query_frusta(h, bp, 4, K.BOX_ANY, op) == K.MOPTIX_OK
    assert L.moptix_query_frusta(h, bp, 4, K.BOX_COUNT, op) == K.MOPTIX_OK and (out == hs.sizes.nSpheres + hs.sizes.nQuads).all()
    for mode in (2, -1, 7):
        assert L.moptix_query_frusta(h, bp, 4, mode, op) == K.ERR_INVALID                       # an unknown mode
    assert L.moptix_query_frusta(h, bp, -1, K.BOX_ANY, op) == K.ERR_INVALID
    assert L.moptix_query_frusta(h, None, 4, K.BOX_ANY, op) == K.ERR_INVALID
    assert L.moptix_query_frusta(h, bp, 4, K.BOX_ANY, None) == K.ERR_INVALID
    assert L.moptix_query_frusta(None, bp, 4, K.BOX_ANY, op) == K.ERR_INVALID
    assert L.moptix_query_frusta_list(h, bp, 4, fp(off), pp, op) == K.MOPTIX_OK
    assert L.moptix_query_frusta_list(h, bp, -1, fp(off), pp, op) == K.ERR_INVALID
    assert L.moptix_query_frusta_list(h, None, 4, fp(off), pp, op) == K.ERR_INVALID
    assert L.moptix_query_frusta_list(h, bp, 4, None, pp, op) == K.ERR_INVALID
    assert L.moptix_query_frusta_list(h, bp, 4, fp(off), None, op) == K.ERR_INVALID
    assert L.moptix_query_frusta_list(h, bp, 4, fp(off), pp, None) == K.ERR_INVALID
    assert L.moptix_query_frusta_list(None, bp, 4, fp(off), pp, op) == K.ERR_INVALID
    falling = np.array([0, 4, 3, 8, 12], np.int64)
    assert L.moptix_query_frusta_list(h, bp, 4, fp(falling), pp, op) == K.ERR_INVALID         # offsets decrease
    negative = np.array([-4, 0, 4, 8, 12], np.int64)
    assert L.moptix_query_frusta_list(h, bp, 4, fp(negative), pp, op) == K.ERR_INVALID        # offsets[0] < 0
    dev = torch.device("cuda", 0)
    db = torch.from_numpy(np.concatenate([b, b[:1]])).to(dev)
    do = torch.zeros(8, dtype=torch.int32, device=dev)
    dp = torch.zeros(24, dtype=torch.int32, device=dev)
    doff = torch.from_numpy(np.concatenate([off, off[-1:]])).to(dev)
    vp = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    assert L.moptix_query_frusta_device(h, vp(db), 4, K.BOX_COUNT, vp(do)) == K.MOPTIX_OK
    assert L.moptix_query_frusta_list_device(h, vp(db), 4, vp(doff), vp(dp), vp(do)) == K.MOPTIX_OK
    ctx.sync()
    assert L.moptix_query_frusta_device(h, vp(db, 16), 4, K.BOX_COUNT, vp(do, 4)) == K.MOPTIX_OK          # 16 and 4 bytes are all they need
    ctx.sync()
    for o in (4, 8, 12):
        assert L.moptix_query_frusta_device(h, vp(db, o), 4, K.BOX_COUNT, vp(do)) == K.ERR_INVALID         # a misaligned pointer
        assert L.moptix_query_frusta_list_device(h, vp(db, o), 4, vp(doff), vp(dp), vp(do)) == K.ERR_INVALID
    assert L.moptix_query_frusta_device(h, vp(db), 4, K.BOX_COUNT, vp(do, 2)) == K.ERR_INVALID             # misaligned results
    assert L.moptix_query_frusta_device(h, vp(db), 4, 2, vp(do)) == K.ERR_INVALID                           # an unknown mode
    assert L.moptix_query_frusta_device(h, vp(db), -1, K.BOX_ANY, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_frusta_device(h, None, 4, K.BOX_ANY, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_frusta_device(h, vp(db), 4, K.BOX_ANY, None) == K.ERR_INVALID
    assert L.moptix_query_frusta_list_device(h, vp(db), 4, vp(doff, 4), vp(dp), vp(do)) == K.ERR_INVALID       # misaligned offsets
    assert L.moptix_query_frusta_list_device(h, vp(db), 4, vp(doff), vp(dp, 2), vp(do)) == K.ERR_INVALID
    assert L.moptix_query_frusta_list_device(h, vp(db), 4, vp(doff), vp(dp), vp(do, 1)) == K.ERR_INVALID
    assert L.moptix_query_frusta_list_device(h, vp(db), 4, None, vp(dp), vp(do)) == K.ERR_INVALID
    assert L.moptix_query_frusta_list_device(h, vp(db), 4, vp(doff), None, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_frusta_list_device(h, vp(db), 4, vp(doff), vp(dp), None) == K.ERR_INVALID
    assert L.moptix_query_frusta_list_device(h, vp(db), -1, vp(doff), vp(dp), vp(do)) == K.ERR_INVALID
    db = db[:4].contiguous()
    for bad in (db[:, :23], db.cpu(), db.double(), db.reshape(-1), db.reshape(8, 12), db.reshape(4, 6, 4)):
        with pytest.raises(ValueError):
            ctx.query_frusta(bad, "count")
    for bad in (b.reshape(-1), b[:, :23], np.zeros((4, 16), np.float32)):
        with pytest.raises(ValueError):
            ctx.query_frusta(bad, "count")
    for kw in (dict(mode="closest"), dict(mode="count", max_prims=4), dict(mode="list", max_prims=-1)):
        with pytest.raises(ValueError):
            ctx.query_frusta(b, **kw)
        with pytest.raises(ValueError):
            ctx.query_frusta(db, **kw)
    fresh = M.Context(0)
    try:
        assert L.moptix_query_frusta(fresh._h, bp, 4, K.BOX_ANY, op) == K.ERR_STATE      # no params, no tree
        assert L.moptix_query_frusta_device(fresh._h, vp(db), 4, K.BOX_ANY, vp(do)) == K.ERR_STATE
        assert L.moptix_query_frusta_list(fresh._h, bp, 4, fp(off), pp, op) == K.ERR_STATE
        assert L.moptix_query_frusta_list_device(fresh._h, vp(db), 4, vp(doff), vp(dp), vp(do)) == K.ERR_STATE
    finally:
        fresh.close()


def test_kernel_resources_of_the_shipped_code_objects():
    """No spilled registers and no scratch on all six instantiations of pt_frustumquery<MODE, N64>, and the 16 KB of LDS of the stack."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec); spec.loader.exec_module(kr)
    res = {k: v for k, v in kr.kernel_resources(K.DEVICE_LIB_PATH if hasattr(K, "DEVICE_LIB_PATH") else os.path.join(REPO, "minimaloptix_amd", "lib", "libmoptix.so")).items()
           if "pt_frustumquery" in k}
    assert len(res) == 6, sorted(res)
    for name, r in sorted(res.items()):
        print("%s %s" % (name, r))
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == 16384 and r["vgpr_count"] <= 128, (name, r)


# ---- stream order: the two _device entries behind a busy stream ----
@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream(torch.device("cuda", 0))


_async = {}


def _async_set(kind):
    """N valid queries of the scene (its perspective frusta, beams and thin regions, cyclically), their poison -- every float NaN, invalid
    by the header's rule --, and per mode the blocking host path's results for both.  Made once, with the GPU idle."""
    if kind not in _async:
        b, parts = _frusta(kind)
        pool = np.concatenate([b[parts["persp"]], b[parts["beams"]], b[parts["thin"]], b[parts["zero"]][:1] if kind != COFFEE else b[:0]])
        if kind == COFFEE:
            pool = pool[frustumsim(point_case(kind).sim, pool, "count") <= 5000]
        _async[kind] = dict(real=np.ascontiguousarray(pool[np.arange(N) % len(pool)]), poison=np.full((N, 24), np.nan, np.float32), want={})
    return _async[kind]


def _expected(ctx, kind, mode):
    s = _async_set(kind)
    if mode not in s["want"]:
        def host(x):
            if mode != "list":
                return (ctx.query_frusta(x, mode),)
            prims, offsets = ctx.query_frusta(x, "list")
            return (np.diff(offsets).astype(np.int32), prims)
        s["want"][mode] = (host(s["real"]), host(s["poison"]))
    want, bad = s["want"][mode]
    poison_differs(bad[:1], want[:1], "%s frusta %s" % (kind, mode))      # a quarter of the records differ: one record per query
    return want


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", ["any", "count", "list"])
@pytest.mark.parametrize("kind", [COFFEE, "spheres"], ids=["coffee", "spheres"])
def test_device_entries_are_ordered_behind_a_busy_stream(ctx, stream, kind, mode):
    """moptix_query_frusta_device (any, count) and moptix_query_frusta_list_device on a caller's stream that is busy: the staged queries
    hold the poison until a copy queued behind the delay brings the real ones, the outputs hold 0xA5 until the kernel writes them and a
    clone queued behind the call reads them.  The call returns while the delay is running; the clone holds the host path's bits."""
    import torch
    pc = point_case(kind)
    _load(ctx, pc.hs)
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
    ctx.query_frusta(real[:256].contiguous(), "count")          # a warm call: the overflow area exists before the stream is busy
    ctx.set_stream(stream.cuda_stream)
    L, h, vp = K.device_lib(), ctx._h, lambda t: C.c_void_p(t.data_ptr())
    rc, free = [], []

    def call():
        free.append(torch.cuda.mem_get_info(dev))
        if mode == "list":
            rc.append(L.moptix_query_frusta_list_device(h, vp(staged), N, vp(offsets), vp(prims), vp(counts)))
        else:
            rc.append(L.moptix_query_frusta_device(h, vp(staged), N, M.Context.BOX_MODES[mode], vp(counts)))
        free.append(torch.cuda.mem_get_info(dev))
    clones, pending = behind_busy_stream(ctx, stream, lambda: staged.copy_(real), call, lambda: [o.clone() for o in outs],
                                         staged=[(staged, bad)], outputs=outs)
    assert rc == [K.MOPTIX_OK], ctx.last_error()
    assert pending, "the call waited for the stream"
    assert free[0] == free[1], "a warm call allocated or freed device memory"
    got = (_np(clones[0]),) if mode != "list" else (_np(clones[0]), _np(clones[1])[:total])
    assert all_same_bits(got, want), [int((g != w).sum()) if g.shape == w.shape else "shape" for g, w in zip(got, want)]
