"""The asynchronous contract of include/moptix.h on the MI355X: every entry that promises asynchronous work on the context's stream, behind
a stream that is busy.  The expected bits are the blocking host path's on the same context, taken while the GPU is idle (the other
test files pin those to the CPU mirrors); here the staged input holds poison -- queries that are invalid by the header's own rule --
until a copy queued behind a delay on the caller's stream brings the real input, and the output holds a byte pattern until the entry's
kernel writes it and a clone queued behind the entry reads it.  An entry (or one of its helpers) that is not ordered on the stream works
on the poison or is read too early; one that waits for the stream is seen by the delay's event having passed when it returns."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from common import M, MovedScene
from refit_helpers import moved_faces, strip_scene
from stream_helpers import (DELAY_S, N, all_same_bits, async_sets, behind_busy_stream, busy, differing, fill_a5, poison_boxes,
                            poison_differs, poison_points, poison_rays, same_bits)

pytestmark = pytest.mark.gpu
K = M._capi
COFFEE, SPHERES, STRIP = "file:coffee", "spheres", "strip5"
SEEDS = [5, 0x9e3779b9, 77, 12345]
SEEDS_B = [9, 31337, 0x7fffffff, 2]
HIT, POINT, SWEEP = M.HIT_DTYPE, M.POINT_DTYPE, M.SWEEP_DTYPE

# The sentences of include/moptix.h the "no host wait" assertions rest on (test_the_quoted_sentences_are_the_headers checks them against
# the file, whitespace and comment stars apart).
Q_RAYS = ("Asynchronous on the context's stream (moptix_set_stream): moptix_sync, or the stream's own synchronisation, waits for it. "
          "Allocates nothing after the first query on a tree")
Q_MULTI = ("Asynchronous on the context's stream. While a ray is walked its slice of dHits holds the candidates; nothing else is allocated "
           "or written.")
Q_RADIANCE = ("Asynchronous on the context's stream: moptix_sync, or the stream's own synchronisation, waits for it. The per-sample scratch "
              "(\"radiance_buffer_mb\") is allocated at first use and kept")
Q_POINTS = ("Asynchronous on the context's stream: moptix_sync, or the stream's own synchronisation, waits for it. Allocates nothing after "
            "the first point query on a tree")
Q_SIGNED = ("the next signed query enqueues its build in front of the query kernel on the context's stream, without a host synchronisation "
            "and without an allocation after the first.")
Q_PMULTI = ("Asynchronous on the context's stream. While a point is walked its slice of dHits holds the candidates; nothing else is "
            "allocated or written.")
Q_BOXES = "4-byte aligned. Asynchronous on the context's stream."
Q_BOXLIST = "dPrims, dCounts: 4-byte aligned. Asynchronous."
Q_SWEEPS = "(any). Asynchronous on the context's stream."
Q_FACES = "as device-to-device copies enqueued on the context's stream"
Q_RENDER = "non-blocking variant for stream overlap; moptix_sync() waits."


# ---- fixtures and the scenes ----
@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_stream(0)                                  # the context's own stream again, whatever the test did
    gpu_ctx.accum_bind(0)


@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def stream_b():
    import torch
    return torch.cuda.Stream(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def other():
    """A second context: the reference of the tests that change a scene, and the other party of the two-context test."""
    c = M.Context(0)
    yield c
    c.close()


class StripSets:
    """Five triangles in coffee's frame (refit_helpers.strip_scene): a tree that fits the LDS stacks, so no family has an overflow area.
    Coffee's rays and points, of which the closest modes are used."""

    def __init__(self):
        s = async_sets(COFFEE)
        self.kind, self.hs, self.diag = STRIP, strip_scene(5), s.diag
        self.rays, self.aimed, self.points, self.points_near, self.boxes, self.sweeps = s.rays, s.aimed, s.points, s.points_near, s.boxes, s.sweeps


_strip = []
_scene = {}                                                # id(context) -> the scene it holds, pristine


def sets_of(kind):
    if kind == STRIP:
        if not _strip:
            _strip.append(StripSets())
        return _strip[0]
    return async_sets(kind)


def _load(c, kind):
    """One scene load per group: the context keeps `kind` until a test says it changed it (_changed)."""
    if _scene.get(id(c)) != kind:
        c.load(sets_of(kind).hs)
        _scene[id(c)] = kind


def _changed(c):
    _scene.pop(id(c), None)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _np(t):
    return np.ascontiguousarray(t.cpu().numpy())


def _rec(t, dtype, shape):
    return _np(t).view(dtype).reshape(shape)


# ---- the entries: input, poison, the blocking host path, the device call, the tensor wrapper ----
class Entry:
    """One asynchronous entry in one mode on one scene's set.  host(ctx, x) -> the blocking host path's results, a tuple of arrays, of
    which the first per_query are one record per query; outs(dev, want) -> the output tensors of the device call; call(L, h, staged,
    outs) -> its return code; got(outs) -> the outputs as host's arrays; wrap(ctx, staged) -> the same through api.py's tensor path."""

    def __init__(self, name, quote, real, poison, host, outs, call, got, wrap, per_query=None):
        self.name, self.quote, self.real, self.poison = name, quote, np.ascontiguousarray(real, np.float32), np.ascontiguousarray(poison, np.float32)
        self.host, self.outs, self.call, self.got, self.wrap, self.per_query = host, outs, call, got, wrap, per_query
        self.aux = {}


def _entries(s):
    import torch
    f32, i32 = torch.float32, torch.int32
    e = {}

    def add(*a, **k):
        e[a[0]] = Entry(*a, **k)
    n = N
    for mode, m in (("closest", K.QUERY_CLOSEST), ("any", K.QUERY_ANY)):
        closest = mode == "closest"
        add("rays_" + mode, Q_RAYS, s.rays, poison_rays(),
            lambda c, x, mode=mode: (c.query_rays(x, mode),),
            lambda dev, want, closest=closest: [torch.empty((n, 8), dtype=f32, device=dev) if closest else torch.empty(n, dtype=i32, device=dev)],
            lambda L, h, x, o, m=m: L.moptix_query_rays_device(h, _vp(x), n, m, _vp(o[0])),
            lambda o, closest=closest: (_rec(o[0], HIT, -1) if closest else _np(o[0]),),
            lambda c, x, mode=mode, closest=closest: (_rec(c.query_rays(x, mode)["records"], HIT, -1) if closest else _np(c.query_rays(x, mode)),))
    for name, call_all in (("rays_multi_k4", False), ("rays_multi_k4_all", True)):
        flags = K.MULTI_COUNT_ALL if call_all else 0

        def wrap_multi(c, x, call_all=call_all):
            hits, counts = c.query_rays_multi(x, 4, call_all)
            return _rec(hits["records"], HIT, (n, 4)), _np(counts)
        add(name, Q_MULTI, s.rays, poison_rays(),
            lambda c, x, call_all=call_all: tuple(c.query_rays_multi(x, 4, call_all)),
            lambda dev, want: [torch.empty((n, 4, 8), dtype=f32, device=dev), torch.empty(n, dtype=i32, device=dev)],
            lambda L, h, x, o, flags=flags: L.moptix_query_rays_multi_device(h, _vp(x), n, 4, flags, _vp(o[0]), _vp(o[1])),
            lambda o: (_rec(o[0], HIT, (n, 4)), _np(o[1])), wrap_multi)
    for name, seeds in (("radiance", SEEDS), ("radiance_b", SEEDS_B)):
        sd = np.asarray(seeds, np.uint32).view(np.int32).copy()
        add(name, Q_RADIANCE, s.rays, poison_rays(),
            lambda c, x, seeds=seeds: (c.query_radiance(x, seeds=seeds),),
            lambda dev, want: [torch.empty((n, 4), dtype=f32, device=dev)],
            lambda L, h, x, o, sd=sd: L.moptix_query_radiance_device(h, _vp(x), n, sd.ctypes.data_as(C.POINTER(C.c_int32)), None, len(sd), 0, 0, _vp(o[0])),
            lambda o: (_np(o[0]),),
            lambda c, x, seeds=seeds: (_np(c.query_radiance(x, seeds=seeds)),))
    for mode, m in (("closest", K.POINT_CLOSEST), ("any", K.POINT_ANY), ("signed", K.POINT_SIGNED)):
        flag = mode == "any"
        add("points_" + mode, Q_SIGNED if mode == "signed" else Q_POINTS, s.points, poison_points(s.points),
            lambda c, x, mode=mode: (c.query_points(x, mode),),
            lambda dev, want, flag=flag: [torch.empty(n, dtype=i32, device=dev) if flag else torch.empty((n, 8), dtype=f32, device=dev)],
            lambda L, h, x, o, m=m: L.moptix_query_points_device(h, _vp(x), n, m, _vp(o[0])),
            lambda o, flag=flag: (_np(o[0]) if flag else _rec(o[0], POINT, -1),),
            lambda c, x, mode=mode, flag=flag: (_np(c.query_points(x, mode)) if flag else _rec(c.query_points(x, mode)["records"], POINT, -1),))
    for name, call_all in (("points_multi_k4", False), ("points_multi_k4_all", True)):
        flags = K.POINT_MULTI_COUNT_ALL if call_all else 0

        def wrap_near(c, x, call_all=call_all):
            hits, counts = c.query_points_multi(x, 4, call_all)
            return _rec(hits["records"], POINT, (n, 4)), _np(counts)
        add(name, Q_PMULTI, s.points_near, poison_points(s.points_near),
            lambda c, x, call_all=call_all: tuple(c.query_points_multi(x, 4, call_all)),
            lambda dev, want: [torch.empty((n, 4, 8), dtype=f32, device=dev), torch.empty(n, dtype=i32, device=dev)],
            lambda L, h, x, o, flags=flags: L.moptix_query_points_multi_device(h, _vp(x), n, 4, flags, _vp(o[0]), _vp(o[1])),
            lambda o: (_rec(o[0], POINT, (n, 4)), _np(o[1])), wrap_near)
    for mode, m in (("any", K.BOX_ANY), ("count", K.BOX_COUNT)):
        add("boxes_" + mode, Q_BOXES, s.boxes, poison_boxes(),
            lambda c, x, mode=mode: (c.query_boxes(x, mode),),
            lambda dev, want: [torch.empty(n, dtype=i32, device=dev)],
            lambda L, h, x, o, m=m: L.moptix_query_boxes_device(h, _vp(x), n, m, _vp(o[0])),
            lambda o: (_np(o[0]),),
            lambda c, x, mode=mode: (_np(c.query_boxes(x, mode)),))

    # the list: counts first (one per box), the ids behind them.  The device call gets the offsets of the expected counts, uploaded while
    # the GPU is idle and never poisoned: the kernel writes where they point.
    def host_list(c, x):
        prims, offsets = c.query_boxes(x, "list")
        return np.diff(offsets).astype(np.int32), prims

    def outs_list(dev, want):
        off = np.zeros(n + 1, np.int64)
        np.cumsum(want[0], dtype=np.int64, out=off[1:])
        lst = e["boxes_list"]
        lst.aux["offsets"], lst.aux["total"] = torch.from_numpy(off).to(dev), int(off[-1])
        return [torch.empty(n, dtype=i32, device=dev), torch.empty(max(int(off[-1]), 1), dtype=i32, device=dev)]

    def wrap_list(c, x):
        prims, offsets = c.query_boxes(x, "list")
        return np.diff(_np(offsets)).astype(np.int32), _np(prims)
    add("boxes_list", Q_BOXLIST, s.boxes, poison_boxes(), host_list, outs_list,
        lambda L, h, x, o: L.moptix_query_boxes_list_device(h, _vp(x), n, _vp(e["boxes_list"].aux["offsets"]), _vp(o[1]), _vp(o[0])),
        lambda o: (_np(o[0]), _np(o[1])[:e["boxes_list"].aux["total"]]), wrap_list, per_query=1)
    for mode, m in (("closest", K.SWEEP_CLOSEST), ("any", K.SWEEP_ANY)):
        closest = mode == "closest"
        add("sweeps_" + mode, Q_SWEEPS, s.sweeps, poison_rays(),
            lambda c, x, mode=mode: (c.query_sweeps(x, mode),),
            lambda dev, want, closest=closest: [torch.empty((n, 8), dtype=f32, device=dev) if closest else torch.empty(n, dtype=i32, device=dev)],
            lambda L, h, x, o, m=m: L.moptix_query_sweeps_device(h, _vp(x), n, m, _vp(o[0])),
            lambda o, closest=closest: (_rec(o[0], SWEEP, -1) if closest else _np(o[0]),),
            lambda c, x, mode=mode, closest=closest: (_rec(c.query_sweeps(x, mode)["records"], SWEEP, -1) if closest else _np(c.query_sweeps(x, mode)),))
    return e


ENTRY_NAMES = ["rays_closest", "rays_any", "rays_multi_k4", "rays_multi_k4_all", "radiance", "points_closest", "points_any", "points_signed",
               "points_multi_k4", "points_multi_k4_all", "boxes_any", "boxes_count", "boxes_list", "sweeps_closest", "sweeps_any"]
CASES = [(kind, name) for kind in (COFFEE, SPHERES) for name in ENTRY_NAMES]
CASE_IDS = ["%s-%s" % (kind.replace("file:", ""), name) for kind, name in CASES]
_entry_tables, _expected_cache = {}, {}


def entry(kind, name):
    if kind not in _entry_tables:
        _entry_tables[kind] = _entries(sets_of(kind))
    return _entry_tables[kind][name]


def expected(c, kind, e):
    """The blocking host path's results of the entry on the context's pristine scene `kind`, and the precondition of every test here: what
    the poison gives differs from them in at least a quarter of the records.  Computed once per context and scene, then only read."""
    key = (id(c), kind, e.name)
    _load(c, kind)
    if key not in _expected_cache:
        want, bad = e.host(c, e.real), e.host(c, e.poison)
        _expected_cache[key] = (want, bad)
    want, bad = _expected_cache[key]
    q = len(want) if e.per_query is None else e.per_query
    poison_differs(bad[:q], want[:q], "%s %s" % (kind, e.name))
    return want


class Queued:
    """An entry made ready for a stream: the real input and the poison on the device, the staged buffer, the outputs."""

    def __init__(self, c, e, want):
        import torch
        self.c, self.e, self.want = c, e, want
        self.real, self.bad = torch.from_numpy(e.real).to(_dev()), torch.from_numpy(e.poison).to(_dev())
        self.staged = torch.empty_like(self.real)
        self.outs = e.outs(_dev(), want)
        self.rc, self.clones = None, None

    def produce(self):
        self.staged.copy_(self.real)

    def call(self):
        self.rc = self.e.call(K.device_lib(), self.c._h, self.staged, self.outs)

    def consume(self):
        self.clones = [o.clone() for o in self.outs]
        return self.clones

    def enqueue(self):
        self.produce(); self.call(); self.consume()

    def poison(self):
        self.staged.copy_(self.bad)
        for o in self.outs:
            fill_a5(o)

    def check(self, what=""):
        assert self.rc == K.MOPTIX_OK, (what, self.e.name, self.c.last_error())
        got = self.e.got(self.clones)
        assert all_same_bits(got, self.want), (what, self.e.name, [differing(g, w) if np.shape(g) == np.shape(w) else "shape" for g, w in zip(got, self.want)])


def run_behind(c, s, e, want, seconds=DELAY_S, probe=None):
    """behind_busy_stream for one entry.  probe: a dict that receives what the context holds just before and just after the call."""
    import torch
    q = Queued(c, e, want)

    def state():
        return (torch.cuda.mem_get_info(), c.debug_buffer_addresses())

    def produce():
        q.produce()
        if probe is not None:
            probe["before"] = state()

    def consume():
        if probe is not None:
            probe["after"] = state()
        return q.consume()
    _, pending = behind_busy_stream(c, s, produce, q.call, consume, staged=[(q.staged, q.bad)], outputs=q.outs, seconds=seconds)
    q.check()
    return pending


def test_the_quoted_sentences_are_the_headers():
    text = open(os.path.join(K.REPO_ROOT, "include", "moptix.h")).read()
    text = re.sub(r"\s+", " ", re.sub(r"\n\s*\*", " ", text))
    for q in (Q_RAYS, Q_MULTI, Q_RADIANCE, Q_POINTS, Q_SIGNED, Q_PMULTI, Q_BOXES, Q_BOXLIST, Q_SWEEPS, Q_FACES, Q_RENDER):
        assert re.sub(r"\s+", " ", q) in text, q


# ---- 1. ordered in and out, per entry ----
@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind,name", CASES, ids=CASE_IDS)
def test_entry_is_ordered_behind_a_busy_stream(ctx, stream, kind, name):
    """coffee's tree is deeper than both LDS stacks (the overflow columns are in use); `spheres` has no tree and no overflow area."""
    e = entry(kind, name)
    want = expected(ctx, kind, e)
    ctx.set_stream(stream.cuda_stream)
    run_behind(ctx, stream, e, want)
    if name == "rays_closest":
        assert (ctx.debug_buffer_addresses()["query_overflow"] != 0) == (kind == COFFEE)


def _faces_case(other):
    """coffee's faces moved (refit_helpers.moved_faces) by 2 % of the extent, and as poison by 5 %; the aimed rays' and the points' answers
    on a context that took either set of rows through the host entry, then refitted.  Made once."""
    key = ("faces", id(other))
    if key not in _expected_cache:
        s = sets_of(COFFEE)
        rows, rows_bad = moved_faces(s.hs, 0.02)[1], moved_faces(s.hs, 0.05)[1]
        _load(other, COFFEE)
        _changed(other)
        res = []
        for r in (rows_bad, rows):
            other.update_faces(0, r)
            other.refit_accel()
            res.append((other.query_rays(s.aimed), other.query_points(s.points)))
        _expected_cache[key] = (rows, rows_bad, res[1], res[0])
    rows, rows_bad, want, bad = _expected_cache[key]
    poison_differs(bad, want, "update_faces")
    return rows, rows_bad, want


def _update_faces_behind(ctx, stream, other, warm):
    import torch
    rows, rows_bad, want = _faces_case(other)
    s = sets_of(COFFEE)
    _load(ctx, COFFEE)
    _changed(ctx)
    ctx.set_stream(stream.cuda_stream)
    L, h, nf = K.device_lib(), ctx._h, len(rows)
    real, bad = torch.from_numpy(rows).to(_dev()), torch.from_numpy(rows_bad).to(_dev())
    staged = torch.empty_like(real)
    rc = []

    def call():
        rc.append(L.moptix_update_faces_device(h, 0, nf, _vp(staged), None))
    if warm:
        staged.copy_(real)
        torch.cuda.synchronize()
        call()
        stream.synchronize()
    _, pending = behind_busy_stream(ctx, stream, lambda: staged.copy_(real), call, lambda: None, staged=[(staged, bad)])
    assert set(rc) == {K.MOPTIX_OK}, ctx.last_error()
    ctx.refit_accel()                                      # blocking, as the header asks before anything traces
    assert all_same_bits((ctx.query_rays(s.aimed), ctx.query_points(s.points)), want)
    return pending


@pytest.mark.timeout(120)
def test_update_faces_device_is_ordered_behind_a_busy_stream(ctx, stream, other):
    """The result of moptix_update_faces_device is the scene after the blocking moptix_refit_accel that must follow: a ray query and a
    point query against a context that took the same rows through the host entry."""
    _update_faces_behind(ctx, stream, other, warm=False)


def _render_behind(ctx, stream, warm):
    """moptix_render_async into a bound accumulation buffer that holds 1.0 everywhere until a zero_() queued behind the delay clears it:
    the frame of a blocking render of the same seeds from a zeroed buffer."""
    import torch
    _load(ctx, COFFEE)
    ctx.set_stream(stream.cuda_stream)
    seeds = M.launch_seeds(4)
    acc = torch.zeros(ctx.height * ctx.width * 3, dtype=torch.float32, device=_dev())
    ones = torch.ones_like(acc)
    torch.cuda.synchronize()
    ctx.accum_bind(acc.data_ptr())
    ctx.render(seeds)
    want = _np(acc)
    acc.copy_(ones); torch.cuda.synchronize()
    ctx.render(seeds)
    poison_differs((_np(acc),), (want,), "render_async")
    if warm:
        acc.zero_(); torch.cuda.synchronize()
        ctx.render_async(seeds); ctx.sync()
    got, pending = behind_busy_stream(ctx, stream, lambda: acc.zero_(), lambda: ctx.render_async(seeds), lambda: acc.clone(), staged=[(acc, ones)])
    ctx.sync()
    assert same_bits(_np(got), want)
    return pending


@pytest.mark.timeout(120)
def test_render_async_is_ordered_behind_a_busy_stream(ctx, stream):
    _render_behind(ctx, stream, warm=False)


# ---- 2. no host wait where the header promises none ----
@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind,name", CASES, ids=CASE_IDS)
def test_warm_entry_returns_while_the_stream_is_busy(ctx, stream, kind, name):
    """After one warm call of the same size the entry comes back while the delay in front of it is still running, and neither the device's
    free memory nor the addresses the context reports change across the call."""
    e = entry(kind, name)
    want = expected(ctx, kind, e)
    ctx.set_stream(stream.cuda_stream)
    run_behind(ctx, stream, e, want, seconds=0.0)          # the warm call
    probe = {}
    pending = run_behind(ctx, stream, e, want, probe=probe)
    assert pending, "%s waited for the stream; include/moptix.h: \"%s\"" % (name, e.quote)
    assert probe["before"] == probe["after"], "%s allocated; include/moptix.h: \"%s\"" % (name, e.quote)


@pytest.mark.timeout(120)
def test_signed_query_rebuilds_a_stale_table_without_a_host_wait(ctx, stream):
    """moptix_update_faces + moptix_refit_accel mark the sign table stale; the next signed query rebuilds it on the stream."""
    s = sets_of(COFFEE)
    e = entry(COFFEE, "points_signed")
    expected(ctx, COFFEE, e)                               # the precondition, on the pristine scene; the table exists from here on
    rows = moved_faces(s.hs, 0.02)[1]
    _changed(ctx)
    ctx.update_faces(0, rows); ctx.refit_accel()
    want, bad = e.host(ctx, e.real), e.host(ctx, e.poison)      # the host path rebuilds the table
    poison_differs(bad, want, "signed, moved")
    builds = ctx.sign_info()["tableBuilds"]
    ctx.update_faces(0, rows); ctx.refit_accel()           # the same rows again: stale again, the same answers
    ctx.set_stream(stream.cuda_stream)
    probe = {}
    pending = run_behind(ctx, stream, e, want, probe=probe)
    assert ctx.sign_info()["tableBuilds"] == builds + 1
    assert pending, "the signed query waited for the stream; include/moptix.h: \"%s\"" % Q_SIGNED
    assert probe["before"] == probe["after"], "the signed query allocated; include/moptix.h: \"%s\"" % Q_SIGNED


@pytest.mark.timeout(120)
def test_warm_update_faces_device_returns_while_the_stream_is_busy(ctx, stream, other):
    assert _update_faces_behind(ctx, stream, other, warm=True), "moptix_update_faces_device waited; include/moptix.h: \"%s\"" % Q_FACES


@pytest.mark.timeout(120)
def test_warm_render_async_returns_while_the_stream_is_busy(ctx, stream):
    assert _render_behind(ctx, stream, warm=True), "moptix_render_async waited for the stream; include/moptix.h: \"%s\"" % Q_RENDER


@pytest.mark.timeout(120)
def test_second_radiance_call_allocates_nothing(ctx, stream):
    """The second of two back-to-back radiance calls may wait for the first call's seed upload (api_radiance.hip upload_seeds): its bits,
    and that it allocates nothing after the first."""
    import torch
    a, b = entry(COFFEE, "radiance"), entry(COFFEE, "radiance_b")
    qa, qb = Queued(ctx, a, expected(ctx, COFFEE, a)), Queued(ctx, b, expected(ctx, COFFEE, b))
    ctx.set_stream(stream.cuda_stream)
    qa.poison(); qb.poison()
    torch.cuda.synchronize()
    qa.produce(); qa.call(); stream.synchronize()          # the warm call
    qa.poison()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        busy(stream)
        qa.enqueue()
        qb.produce()
        before = (torch.cuda.mem_get_info(), ctx.debug_buffer_addresses())
        qb.call()
        after = (torch.cuda.mem_get_info(), ctx.debug_buffer_addresses())
        qb.consume()
    stream.synchronize()
    qa.check("first"); qb.check("second")
    assert before == after


# ---- 3. shared scratch, no host synchronisation between the calls ----
@pytest.mark.timeout(120)
def test_calls_that_share_scratch_queue_up_behind_one_delay(ctx, stream):
    """Closest rays, multi-hit, any rays (one overflow area); two radiance calls with different seeds (one seed staging, one scratch);
    points closest, K-nearest, signed (one overflow area, the sign table); boxes count, a torch cumsum on the stream, boxes list; sweeps.
    One stream.synchronize() at the end."""
    import torch
    names = ["rays_closest", "rays_multi_k4", "rays_any", "radiance", "radiance_b", "points_closest", "points_multi_k4", "points_signed",
             "boxes_count", "boxes_list", "sweeps_closest"]
    qs = {nm: Queued(ctx, entry(COFFEE, nm), expected(ctx, COFFEE, entry(COFFEE, nm))) for nm in names}
    ctx.set_stream(stream.cuda_stream)
    L, h = K.device_lib(), ctx._h
    for q in qs.values():
        q.poison()
    lst = qs["boxes_list"]
    offsets = torch.full((N + 1,), -1, dtype=torch.int64, device=_dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        busy(stream)
        for nm in names:
            if nm != "boxes_list":
                qs[nm].enqueue()
                continue
            offsets[0] = 0                                 # the list's offsets from the count call's own output, on the stream
            # (clamped to the ids' buffer: counts that are not the count call's must not send the list kernel out of bounds)
            offsets[1:] = torch.clamp(torch.cumsum(qs["boxes_count"].outs[0], 0, dtype=torch.int64), 0, lst.e.aux["total"])
            lst.produce()
            lst.rc = L.moptix_query_boxes_list_device(h, _vp(lst.staged), N, _vp(offsets), _vp(lst.outs[1]), _vp(lst.outs[0]))
            lst.consume()
    stream.synchronize()
    for nm in names:
        qs[nm].check()


# ---- 4. a device-only pipeline ----
@pytest.mark.timeout(120)
def test_device_only_pipeline(ctx, stream):
    """rays -> hit records -> (torch) points o + d t -> closest points -> (torch) boxes round them -> counts, all on the caller's stream
    behind a delay; the host touches nothing until the end.  The same chain through the blocking numpy calls."""
    import torch
    s = sets_of(COFFEE)
    _load(ctx, COFFEE)
    half = np.float32(0.02 * s.diag)
    inf = np.float32(np.inf)

    def chain(rays):
        t = ctx.query_rays(rays)["t"]
        with np.errstate(all="ignore"):
            pts = (rays[:, 0:3] + (rays[:, 3:6] * t[:, None]).astype(np.float32)).astype(np.float32)
        p = ctx.query_points(np.ascontiguousarray(np.concatenate([pts, np.full((len(rays), 1), inf, np.float32)], axis=1)))["p"]
        boxes = np.ascontiguousarray(np.concatenate([p - half, p + half], axis=1), np.float32)
        return (ctx.query_boxes(boxes, "count"),)
    rays = np.ascontiguousarray(s.aimed, np.float32)
    want = chain(rays)
    poison_differs(chain(poison_rays()), want, "pipeline")
    ctx.set_stream(stream.cuda_stream)
    L, h, dev = K.device_lib(), ctx._h, _dev()
    real, staged = torch.from_numpy(rays).to(dev), torch.from_numpy(poison_rays()).to(dev)
    hits, near = torch.empty((N, 8), dtype=torch.float32, device=dev), torch.empty((N, 8), dtype=torch.float32, device=dev)
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    infs = torch.full((N, 1), float("inf"), dtype=torch.float32, device=dev)
    for o in (hits, near, counts):
        fill_a5(o)
    torch.cuda.synchronize()
    rc = []
    with torch.cuda.stream(stream):
        busy(stream)
        staged.copy_(real)
        rc.append(L.moptix_query_rays_device(h, _vp(staged), N, K.QUERY_CLOSEST, _vp(hits)))
        moved = staged[:, 3:6] * hits[:, 0:1]
        q = torch.cat([staged[:, 0:3] + moved, infs], dim=1).contiguous()
        rc.append(L.moptix_query_points_device(h, _vp(q), N, K.POINT_CLOSEST, _vp(near)))
        p = near[:, 5:8]
        boxes = torch.cat([p - float(half), p + float(half)], dim=1).contiguous()
        rc.append(L.moptix_query_boxes_device(h, _vp(boxes), N, K.BOX_COUNT, _vp(counts)))
        result = counts.clone()
    stream.synchronize()
    assert rc == [K.MOPTIX_OK] * 3, ctx.last_error()
    assert same_bits(_np(result), want[0])


# ---- 5. the render as the busy work ----
@pytest.mark.timeout(120)
def test_queries_queued_behind_an_asynchronous_render(ctx):
    """render_async(8 seeds) on coffee at 128 x 72, a ray query and a radiance query queued at once on the context's own stream, then
    moptix_sync: the frame of a blocking render, both queries' host-path bits, the kernel timers advanced once."""
    import torch
    ea, eb = entry(COFFEE, "rays_closest"), entry(COFFEE, "radiance")
    qa, qb = Queued(ctx, ea, expected(ctx, COFFEE, ea)), Queued(ctx, eb, expected(ctx, COFFEE, eb))
    _changed(ctx)
    ctx.load(M.HostScene(COFFEE, 128, 72))
    seeds = M.launch_seeds(8)
    ctx.accum_clear(); ctx.render(seeds)
    frame = ctx.accum_read()
    assert frame.any()
    ctx.accum_clear()
    for q in (qa, qb):
        q.poison(); q.produce()
    torch.cuda.synchronize()
    launches = ctx.kernel_time()[1]
    ctx.render_async(seeds)
    qa.call(); qb.call()
    assert K.device_lib().moptix_sync(ctx._h) == K.MOPTIX_OK, ctx.last_error()
    assert ctx.kernel_time()[1] == launches + 1
    qa.consume(); qb.consume()
    torch.cuda.synchronize()
    qa.check(); qb.check()
    assert same_bits(ctx.accum_read(), frame)


# ---- 6. lifecycle calls with queries in flight ----
def _moved_spheres(hs, dx):
    sph = (K.SphereParams * hs.sizes.nSpheres)()
    for i in range(hs.sizes.nSpheres):
        C.memmove(C.byref(sph[i]), C.byref(hs.flat()["spheres"][i]), C.sizeof(K.SphereParams))
        sph[i].center.x += dx
    return sph


def _in_flight(c, s, kind, op):
    """A ray query and a point query queued behind a delay on the context's stream `s`, then op() from the host while they are in
    flight; both outputs are those of the scene as it was when they were queued."""
    import torch
    ea, eb = entry(kind, "rays_closest"), entry(kind, "points_closest")
    qa, qb = Queued(c, ea, expected(c, kind, ea)), Queued(c, eb, expected(c, kind, eb))
    _changed(c)
    c.set_stream(s.cuda_stream)
    qa.poison(); qb.poison()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        busy(s)
        qa.enqueue(); qb.enqueue()
    out = op()
    s.synchronize()
    qa.check("in flight"); qb.check("in flight")
    return qa, qb, out


def _host_answers(c, kind):
    s = sets_of(kind)
    return c.query_rays(s.rays), c.query_points(s.points)


@pytest.mark.timeout(120)
def test_update_spheres_with_queries_in_flight(ctx, stream, other):
    hs = sets_of(SPHERES).hs
    sph = _moved_spheres(hs, 0.25)
    qa, qb, _ = _in_flight(ctx, stream, SPHERES, lambda: ctx.update_spheres(0, sph, hs.sizes.nSpheres))
    _changed(other)
    other.load(MovedScene(hs, spheres=sph))
    want = _host_answers(other, SPHERES)
    assert not same_bits(want[0], qa.want[0]) and not same_bits(want[1], qb.want[0])      # the move changed the answers
    assert all_same_bits(_host_answers(ctx, SPHERES), want)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", [COFFEE, STRIP], ids=["coffee", "strip5"])
def test_update_faces_and_refit_with_queries_in_flight(ctx, stream, other, kind):
    import torch
    hs = sets_of(kind).hs
    rows = moved_faces(hs, 0.02)[1]
    drows = torch.from_numpy(rows).to(_dev())
    torch.cuda.synchronize()

    def op():
        assert K.device_lib().moptix_update_faces_device(ctx._h, 0, len(rows), _vp(drows), None) == K.MOPTIX_OK, ctx.last_error()
        ctx.refit_accel()
    qa, qb, _ = _in_flight(ctx, stream, kind, op)
    _load(other, kind)
    _changed(other)
    other.update_faces(0, rows); other.refit_accel()
    want = _host_answers(other, kind)
    assert not same_bits(want[1], qb.want[0])            # the move changed the answers
    assert all_same_bits(_host_answers(ctx, kind), want)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", [COFFEE, STRIP], ids=["coffee", "strip5"])
def test_build_accel_with_queries_in_flight(ctx, stream, other, kind):
    """The rebuild follows a device-side face update queued behind the queries: the new tree is the moved faces', the queued queries saw
    the old one."""
    import torch
    hs = sets_of(kind).hs
    rows = moved_faces(hs, 0.02)[1]
    drows = torch.from_numpy(rows).to(_dev())
    torch.cuda.synchronize()

    def op():
        assert K.device_lib().moptix_update_faces_device(ctx._h, 0, len(rows), _vp(drows), None) == K.MOPTIX_OK, ctx.last_error()
        ctx.build_accel(hs.accel)
    qa, qb, _ = _in_flight(ctx, stream, kind, op)
    _load(other, kind)
    _changed(other)
    other.update_faces(0, rows); other.build_accel(hs.accel)
    want = _host_answers(other, kind)
    assert not same_bits(want[1], qb.want[0])            # the move changed the answers
    assert all_same_bits(_host_answers(ctx, kind), want)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", [COFFEE, STRIP], ids=["coffee", "strip5"])
def test_clear_scene_and_reload_with_queries_in_flight(ctx, stream, kind):
    hs = sets_of(kind).hs

    def op():
        assert K.device_lib().moptix_clear_scene(ctx._h) == K.MOPTIX_OK
        ctx.load(hs)
    _in_flight(ctx, stream, kind, op)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", [COFFEE, STRIP], ids=["coffee", "strip5"])
def test_set_stream_with_queries_in_flight(ctx, stream, kind):
    qa, qb, _ = _in_flight(ctx, stream, kind, lambda: ctx.set_stream(0))
    assert all_same_bits(_host_answers(ctx, kind), (qa.want[0], qb.want[0]))      # on the context's own stream now
    _scene[id(ctx)] = kind                                 # nothing of the scene changed


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", [COFFEE, STRIP], ids=["coffee", "strip5"])
def test_close_with_queries_in_flight(stream, kind):
    second = M.Context(0)
    try:
        _in_flight(second, stream, kind, second.close)
    finally:
        second.close()
        for key in [k for k in _expected_cache if k[0] == id(second)]:
            del _expected_cache[key]
        _changed(second)


# ---- 7. two contexts, two streams ----
@pytest.mark.timeout(120)
def test_two_contexts_on_two_streams(ctx, other, stream, stream_b):
    """The session's context with coffee and a second one with `spheres`, each on its own stream behind its own delay, calls of the same
    family interleaved from the host: each gets its own scene's bits."""
    import torch
    names = ["rays_closest", "points_closest", "boxes_count", "sweeps_closest", "radiance"]
    qa = [Queued(ctx, entry(COFFEE, nm), expected(ctx, COFFEE, entry(COFFEE, nm))) for nm in names]
    qb = [Queued(other, entry(SPHERES, nm), expected(other, SPHERES, entry(SPHERES, nm))) for nm in names]
    ctx.set_stream(stream.cuda_stream); other.set_stream(stream_b.cuda_stream)
    try:
        for q in qa + qb:
            q.poison()
        torch.cuda.synchronize()
        busy(stream); busy(stream_b)
        for a, b in zip(qa, qb):
            with torch.cuda.stream(stream):
                a.enqueue()
            with torch.cuda.stream(stream_b):
                b.enqueue()
        stream.synchronize(); stream_b.synchronize()
        for q in qa + qb:
            q.check()
    finally:
        other.set_stream(0)


# ---- 8. the tensor wrappers' own synchronisation ----
def _wrapped(c, s, e, want, wrap=None):
    """The wrapper of api.py on a tensor whose real content arrives by a copy queued behind a delay on torch's current stream, the
    context on its own stream: the wrapper's synchronisation of the current stream is all that orders the two."""
    import torch
    real, staged = torch.from_numpy(e.real).to(_dev()), torch.from_numpy(e.poison).to(_dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        busy(s)
        staged.copy_(real)
        got = (wrap or e.wrap)(c, staged)
    s.synchronize()
    assert all_same_bits(got, want), e.name


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", ["rays_closest", "rays_any", "rays_multi_k4", "radiance", "points_closest", "points_signed", "points_multi_k4",
                                  "boxes_count", "boxes_list", "sweeps_closest"])
def test_tensor_wrapper_waits_for_the_callers_stream(ctx, stream, name):
    e = entry(COFFEE, name)
    _wrapped(ctx, stream, e, expected(ctx, COFFEE, e))


@pytest.mark.timeout(120)
def test_tensor_wrapper_of_the_capped_list_waits_for_the_callers_stream(ctx, stream):
    e = entry(COFFEE, "boxes_count")
    expected(ctx, COFFEE, e)
    want, bad = ctx.query_boxes(e.real, "list", max_prims=8), ctx.query_boxes(e.poison, "list", max_prims=8)
    poison_differs(bad, want, "list, 8 slots")

    def wrap(c, x):
        prims, counts = c.query_boxes(x, "list", max_prims=8)
        return _np(prims), _np(counts)
    _wrapped(ctx, stream, e, want, wrap)


@pytest.mark.timeout(120)
def test_update_faces_wrapper_waits_for_the_callers_stream(ctx, stream, other):
    import torch
    rows, rows_bad, want = _faces_case(other)
    s = sets_of(COFFEE)
    _load(ctx, COFFEE)
    _changed(ctx)
    real, staged = torch.from_numpy(rows).to(_dev()), torch.from_numpy(rows_bad).to(_dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        busy(stream)
        staged.copy_(real)
        ctx.update_faces(0, staged)
    ctx.refit_accel()
    assert all_same_bits((ctx.query_rays(s.aimed), ctx.query_points(s.points)), want)
