"""Segment queries on the MI355X (segmentkernel.hip pt_segmentquery): bit for bit the CPU mirror of the kernel's code
(tests/segmentsim/segmentsim.cpp), whole buffers -- closest and any -- on the host path and the tensor path."""
import ctypes as C

import numpy as np
import pytest

from common import M
from query_helpers import SCENES
from refit_helpers import RefitSim, moved_faces
from segment_helpers import (SEGMENT_DTYPE, exact_mesh_cases, exact_mesh_scene, invalid_segments, make_segments, same_bits, segment_case,
                             segment_stack_depth, segmentsim)

pytestmark = pytest.mark.gpu
K = M._capi
COFFEE = "file:coffee"
LDS_ENTRIES = 16                       # segmentkernel.hip kLdsStack: the stack entries a lane keeps in LDS


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_stream(0)
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0)
    gpu_ctx.set_option("query_blocks_per_cu", 32)


def _load(ctx, hs, node_format=0):
    ctx.set_option("node_format", node_format)
    ctx.load(hs)


def _np(t):
    return t.cpu().numpy()


def _records(t):
    """The tensor path's (n, 8) float32 records as a SEGMENT_DTYPE array."""
    return np.ascontiguousarray(_np(t["records"])).view(SEGMENT_DTYPE).reshape(-1)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("kind,iarg", SCENES, ids=[s[0].replace("file:", "") for s in SCENES])
def test_device_is_the_cpu_mirrors_bits(ctx, kind, iarg, fmt):
    import torch
    c = segment_case(kind)
    _load(ctx, c.pc.hs, fmt)
    s = c.segments
    n = len(s)
    want, want_any = segmentsim(c.pc.sim, s, "closest", fmt), segmentsim(c.pc.sim, s, "any", fmt)
    assert same_bits(want_any, (want["prim"] >= 0).astype(np.int32)) and (want["prim"] >= 0).sum() > 100 and (want["prim"] < 0).sum() > 100
    got = ctx.query_segments(s)
    assert got.dtype == SEGMENT_DTYPE and got.shape == (n,)
    assert same_bits(got, want), np.where((got["dist"] != want["dist"]) | (got["prim"] != want["prim"]))[0][:8]
    anyone = ctx.query_segments(s, "any")
    assert anyone.dtype == np.int32 and anyone.shape == (n,) and same_bits(anyone, want_any)
    ts = torch.from_numpy(s).to("cuda:0")
    t = ctx.query_segments(ts)
    assert t["records"].is_cuda and t["records"].dtype == torch.float32 and tuple(t["records"].shape) == (n, 8)
    assert same_bits(_records(t), want)
    for f in ("dist", "prim", "mat", "s", "p", "feature"):
        assert same_bits(_np(t[f]), want[f]), f
    ta = ctx.query_segments(ts, "any")
    assert ta.is_cuda and ta.dtype == torch.int32 and same_bits(_np(ta), want_any)
    # the end points alone, with max_dist beside them: the same queries
    assert same_bits(ctx.query_segments(s[:, :6].reshape(-1, 2, 3), max_dist=s[:, 6]), want)
    assert same_bits(_records(ctx.query_segments(ts[:, :6].contiguous(), max_dist=ts[:, 6])), want)


@pytest.mark.timeout(300)
def test_capped_grid_walks_several_segments_per_lane(ctx):
    """One workgroup per CU and more segments than that grid has lanes, with a partial last block: lanes walk a second segment through
    the same stack columns, on walks deeper than the LDS part of the stack, so the overflow columns of the capped grid are in use.  The
    mirror's bits, and the bits at the default grid."""
    c = segment_case(COFFEE)
    _load(ctx, c.pc.hs)
    cus = ctx.get_option("num_cus")
    n = 256 * cus + 257
    rng = np.random.default_rng(37)
    lo, hi = np.asarray(c.pc.lo, np.float64), np.asarray(c.pc.hi, np.float64)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    a = rng.uniform(lo, hi, (n, 3))
    md = np.where(np.arange(n) % 2 == 0, np.inf, 0.02 * c.diag)
    s = make_segments(a, a + d * (c.diag * 10.0 ** rng.uniform(-3.0, -0.5, (n, 1))), md)
    s[-300:] = c.segments[np.linspace(0, len(c.segments) - 1, 300).astype(np.int64)]      # the set's own segments, in the partial last block too
    assert segment_stack_depth(c.pc.sim, s[::16]) > LDS_ENTRIES
    want = segmentsim(c.pc.sim, s)
    assert (want["prim"] >= 0).sum() > 1000 and (want["prim"] < 0).sum() > 100
    default = (ctx.query_segments(s), ctx.query_segments(s, "any"))
    ctx.set_option("query_blocks_per_cu", 1)
    capped = (ctx.query_segments(s), ctx.query_segments(s, "any"))
    for hits, anyone in (capped, default):
        assert same_bits(hits, want) and same_bits(anyone, (want["prim"] >= 0).astype(np.int32))


@pytest.mark.timeout(300)
def test_after_update_faces_and_refit(ctx):
    c = segment_case(COFFEE)
    _load(ctx, c.pc.hs)
    s = c.segments
    before = ctx.query_segments(s)
    assert same_bits(before, c.hits)
    fp, rows = moved_faces(c.pc.hs, 0.02)
    ctx.update_faces(0, rows)
    for mode in ("closest", "any"):
        with pytest.raises(M.MoptixError) as e:
            ctx.query_segments(s, mode)
        assert e.value.code == K.ERR_STATE
    ctx.refit_accel()
    rs = RefitSim(c.pc.hs, 4)
    try:
        rs.update(0, fp); rs.refit()
        want = segmentsim(rs._sim, s)
        assert same_bits(ctx.query_segments(s), want) and same_bits(ctx.query_segments(s, "any"), segmentsim(rs._sim, s, "any"))
        assert not same_bits(want, before)                      # the move changed the answer
    finally:
        rs.close()


@pytest.mark.timeout(300)
def test_invalid_segments_and_exact_cases(ctx):
    hs = exact_mesh_scene()
    hs.upload(ctx)
    names, s, want = exact_mesh_cases()
    got = ctx.query_segments(s)
    for k, nm in enumerate(names):
        assert same_bits(got[k:k + 1], want[k:k + 1]), (nm, got[k], want[k])
    assert same_bits(ctx.query_segments(s, "any"), (want["prim"] >= 0).astype(np.int32))
    bad = invalid_segments(s[0])
    got = ctx.query_segments(bad)
    assert (got["prim"] == -1).all() and (got["mat"] == -1).all() and same_bits(got["dist"], bad[:, 6])
    assert not got["s"].any() and not got["p"].any() and not got["feature"].any()
    assert not ctx.query_segments(bad, "any").any()
    # the mesh's own edges are at distance 0 from it; edge_proximity is query_segments on vertices[edges]
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [1, 1, 3]], np.float32)
    e = np.array([[0, 1], [1, 2], [3, 0], [3, 3]], np.int64)
    near = ctx.edge_proximity(v, e, 8.0)
    assert same_bits(near, ctx.query_segments(make_segments(v[e[:, 0]], v[e[:, 1]], 8.0)))
    assert (near["dist"][:3] == 0).all() and near["dist"][3] == 3 and (near["prim"] == 0).all()


@pytest.mark.timeout(300)
def test_argument_errors(ctx):
    import torch
    hs = M.HostScene("spheres", 64, 36)
    _load(ctx, hs)
    L, h = K.device_lib(), ctx._h
    s = np.ascontiguousarray(np.tile(np.array([0, 5, 0, 0, 6, 1, 10, 0], np.float32), (4, 1)))
    out = np.zeros(4, SEGMENT_DTYPE)
    sp, op = s.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(out.ctypes.data)
    assert L.moptix_query_segments(h, sp, 4, K.SEGMENT_CLOSEST, op) == K.MOPTIX_OK
    assert L.moptix_query_segments(h, sp, 4, K.SEGMENT_ANY, op) == K.MOPTIX_OK
    for mode in (2, -1, 7):
        assert L.moptix_query_segments(h, sp, 4, mode, op) == K.ERR_INVALID                     # an unknown mode
    assert L.moptix_query_segments(h, sp, -1, K.SEGMENT_CLOSEST, op) == K.ERR_INVALID
    assert L.moptix_query_segments(h, None, 4, K.SEGMENT_CLOSEST, op) == K.ERR_INVALID
    assert L.moptix_query_segments(h, sp, 4, K.SEGMENT_CLOSEST, None) == K.ERR_INVALID
    assert L.moptix_query_segments(None, sp, 4, K.SEGMENT_CLOSEST, op) == K.ERR_INVALID
    assert L.moptix_query_segments(h, None, 0, K.SEGMENT_CLOSEST, None) == K.MOPTIX_OK
    assert L.moptix_query_segments_device(h, None, 0, K.SEGMENT_ANY, None) == K.MOPTIX_OK
    dev = torch.device("cuda", 0)
    ds = torch.from_numpy(np.concatenate([s, s[:1]])).to(dev)
    do = torch.zeros((8, 8), dtype=torch.float32, device=dev)
    vp = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    assert L.moptix_query_segments_device(h, vp(ds), 4, K.SEGMENT_CLOSEST, vp(do)) == K.MOPTIX_OK
    assert L.moptix_query_segments_device(h, vp(ds), 4, K.SEGMENT_ANY, vp(do, 4)) == K.MOPTIX_OK          # int32 results need 4-byte alignment only
    ctx.sync()
    assert L.moptix_query_segments_device(h, vp(ds, 8), 4, K.SEGMENT_CLOSEST, vp(do)) == K.ERR_INVALID     # misaligned segments
    assert L.moptix_query_segments_device(h, vp(ds), 4, K.SEGMENT_CLOSEST, vp(do, 8)) == K.ERR_INVALID     # misaligned records
    assert L.moptix_query_segments_device(h, vp(ds), 4, K.SEGMENT_ANY, vp(do, 2)) == K.ERR_INVALID
    assert L.moptix_query_segments_device(h, vp(ds), 4, 2, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_segments_device(h, vp(ds), -1, K.SEGMENT_ANY, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_segments_device(h, None, 4, K.SEGMENT_ANY, vp(do)) == K.ERR_INVALID
    assert L.moptix_query_segments_device(h, vp(ds), 4, K.SEGMENT_ANY, None) == K.ERR_INVALID
    ds = ds[:4].contiguous()
    for bad in (ds[:, :7], ds.cpu(), ds.double(), ds.reshape(-1), ds.reshape(2, 16), ds.reshape(4, 2, 4), ds[:, :6]):
        with pytest.raises(ValueError):
            ctx.query_segments(bad)
    for bad in (s.reshape(-1), s[:, :7], np.zeros((4, 2, 4), np.float32), s[:, :6]):
        with pytest.raises(ValueError):
            ctx.query_segments(bad)
    with pytest.raises(ValueError):
        ctx.query_segments(s[:, :6], max_dist=np.ones(3, np.float32))
    for mode in ("count", "signed", 0):
        with pytest.raises(ValueError):
            ctx.query_segments(s, mode)
        with pytest.raises(ValueError):
            ctx.query_segments(ds, mode)
    assert len(ctx.query_segments(np.zeros((0, 8), np.float32))) == 0 and len(ctx.query_segments(np.zeros((0, 8), np.float32), "any")) == 0
    empty = ctx.query_segments(torch.zeros((0, 8), dtype=torch.float32, device=dev))
    assert tuple(empty["records"].shape) == (0, 8)
    fresh = M.Context(0)
    try:
        assert L.moptix_query_segments(fresh._h, sp, 4, K.SEGMENT_CLOSEST, op) == K.ERR_STATE      # no params, no tree
        assert L.moptix_query_segments_device(fresh._h, vp(ds), 4, K.SEGMENT_CLOSEST, vp(do)) == K.ERR_STATE
    finally:
        fresh.close()


@pytest.mark.timeout(300)
def test_leaves_the_context_alone(ctx):
    """A render before and after the segment queries has equal bits, the other queries' buffers stay where they are, and a refit keeps
    the segment queries' overflow area with the others."""
    from point_helpers import with_max
    c = segment_case(COFFEE)
    _load(ctx, c.pc.hs)
    seeds = M.launch_seeds(1)
    ctx.accum_clear(); ctx.render_counted(seeds)
    frame = ctx.accum_read().copy()
    s = c.segments[::4]
    q = with_max(c.pc.pts[::16])
    closest = ctx.query_points(q)
    addr = ctx.debug_buffer_addresses()
    hits = ctx.query_segments(s)
    ctx.query_segments(s, "any")
    assert ctx.debug_buffer_addresses() == addr
    assert same_bits(ctx.query_points(q), closest)
    ctx.accum_clear(); ctx.render_counted(seeds)
    assert same_bits(ctx.accum_read(), frame)
    ctx.refit_accel()
    assert same_bits(ctx.query_segments(s), hits) and same_bits(ctx.query_points(q), closest)


@pytest.mark.timeout(120)
def test_device_entry_is_ordered_on_the_contexts_stream(ctx):
    """moptix_query_segments_device behind a delay on the stream the context was given (stream_helpers.behind_busy_stream): the call
    returns while the delay is running, the kernel reads the segments that arrive on the stream behind the delay and not the poison
    that was there when it was enqueued, and a clone enqueued behind it holds the records."""
    import torch
    from stream_helpers import N, behind_busy_stream, poison_differs
    c = segment_case(COFFEE)
    _load(ctx, c.pc.hs)
    real = np.ascontiguousarray(c.segments[np.arange(N) % c.n_base])
    poison = real.copy(); poison[:, 6] = np.nan                                # invalid by the header's rule: every row a miss
    want = ctx.query_segments(real)
    poison_differs((ctx.query_segments(poison),), (want,), "segments")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    d_real, d_bad = torch.from_numpy(real).to(dev), torch.from_numpy(poison).to(dev)
    staged, out = torch.empty_like(d_real), torch.empty((N, 8), dtype=torch.float32, device=dev)
    rc = []
    vp = lambda t: C.c_void_p(t.data_ptr())
    clone, pending = behind_busy_stream(ctx, stream, lambda: staged.copy_(d_real),
                                        lambda: rc.append(K.device_lib().moptix_query_segments_device(ctx._h, vp(staged), N, K.SEGMENT_CLOSEST, vp(out))),
                                        lambda: out.clone(), staged=[(staged, d_bad)], outputs=[out])
    assert rc == [K.MOPTIX_OK], ctx.last_error()
    assert pending                                                              # the call did not wait for the stream
    assert same_bits(np.ascontiguousarray(_np(clone)).view(SEGMENT_DTYPE).reshape(-1), want)
