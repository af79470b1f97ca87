"""Oriented box queries on the MI355X (obbkernel.hip pt_obbquery): bit for bit the CPU mirror of the kernel's code
(tests/obbsim/obbsim.cpp), whole buffers -- any, count, the CSR list and the fixed-capacity list -- on the host path and the tensor path;
and the two asynchronous entries behind a busy stream."""
import ctypes as C

import numpy as np
import pytest

from common import M, MovedScene
from obb_helpers import csr, obb_sets, obbsim, obbsim_list, pack, random_rotations, same_bits
from point_helpers import point_case
from query_helpers import SCENES, coffee_rays
from refit_helpers import RefitSim, moved_faces
from stream_helpers import N, all_same_bits, behind_busy_stream, poison_differs

pytestmark = pytest.mark.gpu
K = M._capi
COFFEE = "file:coffee"
LDS_ENTRIES = 16                       # obbkernel.hip kLdsStack: the stack entries a lane keeps in LDS


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_stream(0)
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0)
    gpu_ctx.set_option("query_blocks_per_cu", 32)


def _load(ctx, hs, node_format=0):
    ctx.set_option("node_format", node_format)
    ctx.load(hs)


_sets = {}


def _obbs(name):
    """The scene's oriented box set (obb_helpers.obb_sets, about 1,500 boxes) and its parts."""
    if name not in _sets:
        pc = point_case(name)
        _sets[name] = obb_sets(pc.geo, pc.lo, pc.hi)
    return _sets[name]


def _np(t):
    return t.cpu().numpy()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("kind,iarg", SCENES, ids=[s[0].replace("file:", "") for s in SCENES])
def test_device_is_the_cpu_mirrors_bits(ctx, kind, iarg, fmt):
    """Coffee is here for the overflow columns (its tree is deeper than the LDS part of the stack), spheres for a scene without a tree."""
    import torch
    pc = point_case(kind)
    _load(ctx, pc.hs, fmt)
    b = _obbs(kind)[0]
    assert len(b) <= 4096
    if kind == COFFEE:
        # one lane sorts one list, and a list of all 168,196 ids takes it a second: the 60 boxes that meet more than 20,000 primitives are
        # left to the mirror's tests and to any / count below (test_capped_grid_walks_several_boxes_per_lane counts the whole-scene box)
        b = np.ascontiguousarray(b[obbsim(pc.sim, b, "count", fmt) <= 20000])
        assert len(b) > 1300
    n = len(b)
    want_any, want_c = obbsim(pc.sim, b, "any", fmt), obbsim(pc.sim, b, "count", fmt)
    want_p = obbsim_list(pc.sim, b, csr(want_c), fmt)[0]
    cap = 8 if kind == COFFEE else 2                            # a capacity that some of the scene's boxes overflow and some do not fill
    fixed = np.arange(n + 1, dtype=np.int64) * cap
    want_fp, want_fc = obbsim_list(pc.sim, b, fixed, fmt)
    assert (want_c > cap).any() and ((want_c > 0) & (want_c < cap)).sum() > 20 and (want_c == 0).sum() > 20
    tb = torch.from_numpy(b).to("cuda:0")
    # any / count: host path, tensor path
    for mode, want in (("any", want_any), ("count", want_c)):
        got = ctx.query_obbs(b, mode)
        assert got.dtype == np.int32 and got.shape == (n,) and same_bits(got, want), (mode, np.where(got != want)[0][:8])
        t = ctx.query_obbs(tb, mode)
        assert t.is_cuda and t.dtype == torch.int32 and same_bits(_np(t), want), mode
    # the CSR pair: the list at exact capacities
    prims, offsets = ctx.query_obbs(b, "list")
    assert prims.dtype == np.int32 and offsets.dtype == np.int64 and same_bits(offsets, csr(want_c)) and same_bits(prims, want_p)
    tp, to = ctx.query_obbs(tb, "list")
    assert tp.is_cuda and tp.dtype == torch.int32 and to.dtype == torch.int64
    assert same_bits(_np(to), csr(want_c)) and same_bits(_np(tp), want_p)
    # short slices: truncated ones are -1 throughout, the counts the true ones
    fp, fc = ctx.query_obbs(b, "list", max_prims=cap)
    assert fp.shape == (n, cap) and same_bits(fc, want_c) and same_bits(fc, want_fc) and same_bits(fp.reshape(-1), want_fp)
    assert (fp[want_c > cap] == -1).all()
    tfp, tfc = ctx.query_obbs(tb, "list", max_prims=cap)
    assert tuple(tfp.shape) == (n, cap) and same_bits(_np(tfc), want_c) and same_bits(_np(tfp).reshape(-1), want_fp)
    zp, zc = ctx.query_obbs(b, "list", max_prims=0)
    assert zp.shape == (n, 0) and same_bits(zc, want_c)


@pytest.mark.timeout(300)
def test_capped_grid_walks_several_boxes_per_lane(ctx):
    """One workgroup per CU and more boxes than that grid has lanes, with a partial last block: lanes walk a second box through the same
    stack columns, on a tree deeper than the LDS part of the stack, so the overflow columns of the capped grid are in use.  The mirror's
    bits, and the bits at the default grid.  The grid cannot be capped below one workgroup per CU, hence the number of boxes; they are
    small ones."""
    pc = point_case(COFFEE)
    _load(ctx, pc.hs)
    assert 3 * ctx.accel_info().treeDepth + 1 > LDS_ENTRIES
    cus = ctx.get_option("num_cus")
    n = 256 * cus + 257
    rng = np.random.default_rng(36)
    diag = float(np.linalg.norm(pc.hi - pc.lo))
    c = rng.uniform(pc.lo, pc.hi, (n, 3))
    h = diag * 10.0 ** rng.uniform(-3.0, -1.5, (n, 3))
    bl = pack(c, h, random_rotations(rng, n))
    b = bl.copy()
    b[-1] = _obbs(COFFEE)[0][_obbs(COFFEE)[1]["whole"]]        # any / count: the whole scene, the deepest walk, in the partial last block
    want_c, want_lc = obbsim(pc.sim, b, "count"), obbsim(pc.sim, bl, "count")
    want_p = obbsim_list(pc.sim, bl, csr(want_lc))[0]
    assert (want_c > 64).sum() > 100 and (want_c == 0).sum() > 1000 and want_c[-1] > 100000
    default = (ctx.query_obbs(b, "any"), ctx.query_obbs(b, "count"), ctx.query_obbs(bl, "list"))
    ctx.set_option("query_blocks_per_cu", 1)
    capped = (ctx.query_obbs(b, "any"), ctx.query_obbs(b, "count"), ctx.query_obbs(bl, "list"))
    for anyone, counts, (prims, offsets) in (capped, default):
        assert same_bits(counts, want_c) and same_bits(anyone, (want_c > 0).astype(np.int32))
        assert same_bits(offsets, csr(want_lc)) and same_bits(prims, want_p)


@pytest.mark.timeout(300)
def test_after_update_faces_and_refit(ctx):
    pc = point_case(COFFEE)
    _load(ctx, pc.hs)
    b = _obbs(COFFEE)[0]
    before = ctx.query_obbs(b, "count")
    assert same_bits(before, obbsim(pc.sim, b, "count"))
    fp, rows = moved_faces(pc.hs, 0.02)
    ctx.update_faces(0, rows)
    for kw in (dict(mode="any"), dict(mode="count"), dict(mode="list"), dict(mode="list", max_prims=4)):
        with pytest.raises(M.MoptixError) as e:
            ctx.query_obbs(b, **kw)
        assert e.value.code == K.ERR_STATE
    ctx.refit_accel()
    rs = RefitSim(pc.hs, 4)
    try:
        rs.update(0, fp); rs.refit()
        want_c = obbsim(rs._sim, b, "count")
        assert same_bits(ctx.query_obbs(b, "count"), want_c) and same_bits(ctx.query_obbs(b, "any"), obbsim(rs._sim, b, "any"))
        prims, offsets = ctx.query_obbs(b, "list")
        assert same_bits(offsets, csr(want_c)) and same_bits(prims, obbsim_list(rs._sim, b, csr(want_c))[0])
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
    b = _obbs("random_spheres")[0]
    before = ctx.query_obbs(b, "count")
    assert same_bits(before, obbsim(hs, b, "count"))
    for i in range(0, n, 3):
        sph[i].center.y += 0.75
    ctx.update_spheres(0, sph, n)
    moved = MovedScene(hs, spheres=sph)
    want_c = obbsim(moved, b, "count")
    assert not same_bits(want_c, before)
    assert same_bits(ctx.query_obbs(b, "count"), want_c)
    prims, offsets = ctx.query_obbs(b, "list")
    assert same_bits(offsets, csr(want_c)) and same_bits(prims, obbsim_list(moved, b, csr(want_c))[0])


@pytest.mark.timeout(300)
def test_leaves_the_context_alone(ctx):
    pc = point_case(COFFEE)
    _load(ctx, pc.hs)
    b = _obbs(COFFEE)[0][::4]
    q = np.ascontiguousarray(np.concatenate([pc.pts[::16], np.full((len(pc.pts[::16]), 1), np.inf, np.float32)], axis=1))
    boxes = np.ascontiguousarray(np.concatenate([pc.pts[::16] - 0.01, pc.pts[::16] + 0.01], axis=1), np.float32)
    rays = coffee_rays()
    seeds = M.launch_seeds(1)
    ctx.accum_clear(); ctx.render(seeds)
    accum = ctx.accum_read()
    closest, anyone = ctx.query_points(q), ctx.query_points(q, "any")
    hits = ctx.query_rays(rays)
    aligned = ctx.query_boxes(boxes, "count")
    addr = ctx.debug_buffer_addresses()
    assert addr["query_overflow"] != 0
    counts = ctx.query_obbs(b, "count")
    ctx.query_obbs(b, "any"); ctx.query_obbs(b, "list"); ctx.query_obbs(b, "list", max_prims=4)
    assert ctx.debug_buffer_addresses() == addr
    assert same_bits(ctx.accum_read(), accum)
    assert same_bits(ctx.query_points(q), closest) and same_bits(ctx.query_points(q, "any"), anyone)
    assert same_bits(ctx.query_rays(rays), hits) and same_bits(ctx.query_boxes(boxes, "count"), aligned)
    assert same_bits(ctx.query_obbs(b, "count"), counts)
    ctx.refit_accel()                                           # keeps the oriented box queries' overflow area with the others
    assert ctx.debug_buffer_addresses()["query_overflow"] == addr["query_overflow"] and same_bits(ctx.query_obbs(b, "count"), counts)


@pytest.mark.timeout(300)
def test_argument_errors(ctx):
    import torch
    hs = M.HostScene("spheres", 64, 36)
    _load(ctx, hs)
    L, h = K.device_lib(), ctx._h
    b = pack(np.zeros((4, 3)), np.ones((4, 3)), np.repeat(np.eye(3)[None], 4, axis=0))
    out, prims, off = np.zeros(4, np.int32), np.zeros(16, np.int32), np.arange(5, dtype=np.int64) * 4
    bp, op, pp = b.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_int32)), prims.ctypes.data_as(C.POINTER(C.c_int32))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.moptix_query_obbs(h, bp, 4, K.BOX_ANY, op) == K.MOPTIX_OK
    assert L.moptix_query_obbs(h, bp, 4, K.BOX_COUNT, op) == K.MOPTIX_OK
    for mode in (2, -1, 7):
        assert L.moptix_query_obbs(h, bp, 4, mode, op) == K.ERR_INVALID                       # an unknown mode
    assert L.moptix_query_obbs(h, bp, -1, K.BOX_ANY, op) == K.ERR_INVALID
    assert L.moptix_query_obbs(h, None, 4, K.BOX_ANY, op) == K.ERR_INVALID
    assert L.moptix_query_obbs(h, bp, 4, K.BOX_ANY, None) == K.ERR_INVALID
    assert L.moptix_query_obbs(None, bp, 4, K.BOX_ANY, op) == K.ERR_INVALID
    assert L.moptix_query_obbs(h, None, 0, K.BOX_ANY, None) == K.MOPTIX_OK
    assert L.moptix_query_obbs_device(h, None, 0, K.BOX_COUNT, None) == K.MOPTIX_OK
    assert L.moptix_query_obbs_list(h, bp, 4, fp(off), pp, op) == K.MOPTIX_OK
    assert L.moptix_query_obbs_list(h, bp, -1, fp(off), pp, op) == K.ERR_INVALID
    assert L.moptix_query_obbs_list(h, None, 4, fp(off), pp, op) == K.ERR_INVALID
    assert L.moptix_query_obbs_list(h, bp, 4, None, pp, op) == K.ERR_INVALID
    assert L.moptix_query_obbs_list(h, bp, 4, fp(off), None, op) == K.ERR_INVALID
    assert L.moptix_query_obbs_list(h, bp, 4, fp(off), pp, None) == K.ERR_INVALID
    assert L.moptix_query_obbs_list(None, bp, 4, fp(off), pp, op) == K.ERR_INVALID
    assert L.moptix_query_obbs_list(h, None, 0, None, None, None) == K.MOPTIX_OK
    assert L.moptix_query_obbs_list_device(h, None, 0, None, None, None) == K.MOPTIX_OK
    falling = np.array([0, 4, 3, 8, 12], np.int64)
    assert L.moptix_query_obbs_list(h, bp, 4, fp(falling), pp, op) == K.ERR_INVALID         # offsets decrease
    negative = np.array([-4, 0, 4, 8, 12], np.int64)
    assert L.moptix_query_obbs_list(h, bp, 4, fp(negative), pp, op) == K.ERR_INVALID        # offsets[0] < 0
    dev = torch.device("cuda", 0)
    db = torch.from_numpy(np.concatenate([b, b[:1]])).to(dev)
    do = torch.zeros(8, dtype=torch.int32, device=dev)
    dp = torch.zeros(24, dtype=torch.int32, device=dev)
    doff = torch.from_numpy(np.concatenate([off, off[-1:]])).to(dev)
    vp = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    assert L.moptix_query_obbs_device(h, vp(db), 4, K.BOX_COUNT, vp(do)) == K.MOPTIX_OK
    assert L.moptix_query_obbs_list_device(h, vp(db), 4, vp(doff), vp(dp), vp(do)) == K.MOPTIX_OK
    ctx.sync()
    assert L.moptix_query_obbs_device(h, vp(db, 16), 4, K.BOX_COUNT, vp(do, 4)) == K.MOPTIX_OK          # 16 and 4 bytes are all they need
    ctx.sync()
    for o in (4, 8, 12):
        assert L.moptix_query_obbs_device(h, vp(db, o), 4, K.BOX_COUNT, vp(do)) == K.ERR_INVALID         # misaligned dObbs
        assert L.moptix_query_obbs_list_device(h, vp(db, o), 4, vp(doff), vp(dp), vp(do)) == K.ERR_INVALID
    assert L.moptix_query_obbs_device(h, vp(db), 4, K.BOX_COUNT, vp(do, 2)) == K.ERR_INVALID             # misaligned results
    assert L.moptix_query_obbs_device(h, vp(db), 4, 2, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_obbs_device(h, vp(db), -1, K.BOX_ANY, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_obbs_device(h, None, 4, K.BOX_ANY, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_obbs_device(h, vp(db), 4, K.BOX_ANY, None) == K.ERR_INVALID
    assert L.moptix_query_obbs_list_device(h, vp(db), 4, vp(doff, 4), vp(dp), vp(do)) == K.ERR_INVALID       # misaligned offsets
    assert L.moptix_query_obbs_list_device(h, vp(db), 4, vp(doff), vp(dp, 2), vp(do)) == K.ERR_INVALID
    assert L.moptix_query_obbs_list_device(h, vp(db), 4, vp(doff), vp(dp), vp(do, 1)) == K.ERR_INVALID
    assert L.moptix_query_obbs_list_device(h, vp(db), 4, None, vp(dp), vp(do)) == K.ERR_INVALID
    assert L.moptix_query_obbs_list_device(h, vp(db), 4, vp(doff), None, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_obbs_list_device(h, vp(db), 4, vp(doff), vp(dp), None) == K.ERR_INVALID
    assert L.moptix_query_obbs_list_device(h, vp(db), -1, vp(doff), vp(dp), vp(do)) == K.ERR_INVALID
    db = db[:4].contiguous()
    for bad in (db[:, :15], db.cpu(), db.double(), db.reshape(-1), db.reshape(8, 8), db.reshape(4, 4, 4)):
        with pytest.raises(ValueError):
            ctx.query_obbs(bad, "count")
    for bad in (b.reshape(-1), b[:, :15], np.zeros((4, 6), np.float32)):
        with pytest.raises(ValueError):
            ctx.query_obbs(bad, "count")
    for kw in (dict(mode="closest"), dict(mode="count", max_prims=4), dict(mode="list", max_prims=-1)):
        with pytest.raises(ValueError):
            ctx.query_obbs(b, **kw)
        with pytest.raises(ValueError):
            ctx.query_obbs(db, **kw)
    assert len(ctx.query_obbs(np.zeros((0, 16), np.float32), "count")) == 0
    ep, eo = ctx.query_obbs(np.zeros((0, 16), np.float32), "list")
    assert len(ep) == 0 and same_bits(eo, np.zeros(1, np.int64))
    fresh = M.Context(0)
    try:
        assert L.moptix_query_obbs(fresh._h, bp, 4, K.BOX_ANY, op) == K.ERR_STATE      # no params, no tree
        assert L.moptix_query_obbs_device(fresh._h, vp(db), 4, K.BOX_ANY, vp(do)) == K.ERR_STATE
        assert L.moptix_query_obbs_list(fresh._h, bp, 4, fp(off), pp, op) == K.ERR_STATE
        assert L.moptix_query_obbs_list_device(fresh._h, vp(db), 4, vp(doff), vp(dp), vp(do)) == K.ERR_STATE
    finally:
        fresh.close()


# ---- stream order: the two _device entries behind a busy stream ----
@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream(torch.device("cuda", 0))


_async = {}


def _async_set(kind):
    """N valid oriented boxes of the scene (the parts of its set that are centred on the surface, cyclically), their poison -- every float
    NaN, invalid by the header's rule --, and per mode the blocking host path's results for both.  Made once, with the GPU idle."""
    if kind not in _async:
        b, parts = _obbs(kind)
        real = np.ascontiguousarray(b[512:parts["touching"].stop][np.arange(N) % (parts["touching"].stop - 512)])
        _async[kind] = dict(real=real, poison=np.full((N, 16), np.nan, np.float32), want={})
    return _async[kind]


def _expected(ctx, kind, mode):
    s = _async_set(kind)
    if mode not in s["want"]:
        def host(x):
            if mode != "list":
                return (ctx.query_obbs(x, mode),)
            prims, offsets = ctx.query_obbs(x, "list")
            return (np.diff(offsets).astype(np.int32), prims)
        s["want"][mode] = (host(s["real"]), host(s["poison"]))
    want, bad = s["want"][mode]
    poison_differs(bad[:1], want[:1], "%s obbs %s" % (kind, mode))      # a quarter of the records differ: one record per query
    return want


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", ["any", "count", "list"])
@pytest.mark.parametrize("kind", [COFFEE, "spheres"], ids=["coffee", "spheres"])
def test_device_entries_are_ordered_behind_a_busy_stream(ctx, stream, kind, mode):
    """moptix_query_obbs_device (any, count) and moptix_query_obbs_list_device on a caller's stream that is busy: the staged boxes hold the
    poison until a copy queued behind the delay brings the real ones, the outputs hold 0xA5 until the kernel writes them and a clone
    queued behind the call reads them.  The call returns while the delay is running; the clone holds the host path's bits."""
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
    ctx.query_obbs(real[:256].contiguous(), "count")            # a warm call: the overflow area exists before the stream is busy
    ctx.set_stream(stream.cuda_stream)
    L, h, vp = K.device_lib(), ctx._h, lambda t: C.c_void_p(t.data_ptr())
    rc, free = [], []

    def call():
        free.append(torch.cuda.mem_get_info(dev))
        if mode == "list":
            rc.append(L.moptix_query_obbs_list_device(h, vp(staged), N, vp(offsets), vp(prims), vp(counts)))
        else:
            rc.append(L.moptix_query_obbs_device(h, vp(staged), N, M.Context.BOX_MODES[mode], vp(counts)))
        free.append(torch.cuda.mem_get_info(dev))
    clones, pending = behind_busy_stream(ctx, stream, lambda: staged.copy_(real), call, lambda: [o.clone() for o in outs],
                                         staged=[(staged, bad)], outputs=outs)
    assert rc == [K.MOPTIX_OK], ctx.last_error()
    assert pending, "the call waited for the stream"
    assert free[0] == free[1], "a warm call allocated or freed device memory"
    got = (_np(clones[0]),) if mode != "list" else (_np(clones[0]), _np(clones[1])[:total])
    assert all_same_bits(got, want), [int((g != w).sum()) if g.shape == w.shape else "shape" for g, w in zip(got, want)]
