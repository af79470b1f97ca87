"""What the stream-order tests (test_gpu_async.py) share: a finite delay on a caller's stream, the pattern "poison, delay, produce, call,
consume" that shows whether an asynchronous entry is ordered on the context's stream, the query sets and their poison, and how two
results are compared record by record."""
import math

import numpy as np

from query_helpers import box_rays, coffee_rays, same_bits      # noqa: F401  (same_bits: for the tests)

N = 4096 + 37                          # queries per call: more than one block, a partial last one
DELAY_S = 0.2                          # profiles/r29_async.txt: 50 x the longest warm entry call is far below it, so the floor of 0.2 s holds
DELAY_CAP_S = 1.0
MM = 4096                              # the delay's unit of work: one MM x MM binary32 torch.mm
MARGIN = 1.5                           # the chain is made this much longer than the calibration asks: the clocks rise under load

_calib = {}


def _operands(device):
    import torch
    key = ("ops", str(device))
    if key not in _calib:
        g = torch.Generator(device="cpu"); g.manual_seed(29)
        a = (torch.rand((MM, MM), generator=g) / MM).to(device)
        _calib[key] = (a, a.clone(), torch.empty_like(a))
    return _calib[key]


def mm_seconds(stream):
    """Seconds one unit of the delay takes, from an event-timed chain of 16 on `stream` after a warm-up of 4 (made once per process)."""
    import torch
    key = ("mm", str(stream.device))
    if key not in _calib:
        a, b, c = _operands(stream.device)
        with torch.cuda.stream(stream):
            for _ in range(4):
                torch.mm(a, b, out=c)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(16):
                torch.mm(a, b, out=c)
            e1.record(stream)
        e1.synchronize()
        _calib[key] = max(e0.elapsed_time(e1) / 16.0 * 1e-3, 1e-6)
    return _calib[key]


def busy(stream, seconds=DELAY_S):
    """Queues at least `seconds` (of at most DELAY_CAP_S) of ordinary, finite work on `stream` -- a chain of torch.mm calls whose length comes
    from mm_seconds -- and returns an event recorded behind it: event.query() is False while the delay is still running."""
    import torch
    per = mm_seconds(stream)
    links = max(1, int(math.ceil(MARGIN * min(float(seconds), DELAY_CAP_S) / per)))
    a, b, c = _operands(stream.device)
    with torch.cuda.stream(stream):
        for _ in range(links):
            torch.mm(a, b, out=c)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def fill_a5(t):
    """Every byte of the tensor becomes 0xA5: no record, count or flag any query writes."""
    import torch
    t.view(torch.uint8).fill_(0xA5)


def behind_busy_stream(ctx, stream, produce, call, consume, staged=(), outputs=(), seconds=DELAY_S):
    """The pattern of the stream-order tests, for a context whose stream is `stream` (moptix_set_stream):
      1. with the GPU idle, every (tensor, poison) pair of `staged` gets its poison and every tensor of `outputs` the 0xA5 pattern;
      2. on `stream`: the delay, produce() -- the real input arrives, e.g. staged.copy_(real) -- then call(), the library's entry through
         ctypes, then consume(), e.g. out.clone();
      3. straight after call() returns the delay's event is read;
      4. stream.synchronize().
    Returns (consume()'s value, still_pending): still_pending is True when call() came back while the delay was running, i.e. it did not
    wait for the stream.  A kernel or helper that is not ordered behind produce() works on the poison, one not ordered in front of
    consume() leaves the pattern in the clone."""
    import torch
    for t, poison in staged:
        t.copy_(poison)
    for t in outputs:
        fill_a5(t)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        delay = busy(stream, seconds)
        produce()
        call()
        pending = not delay.query()
        result = consume()
    stream.synchronize()
    return result, pending


# ---- comparing results ----
def rows(a, n=None):
    """A result array as bytes, one row per record (n records; default: its first axis)."""
    a = np.ascontiguousarray(a)
    n = a.shape[0] if n is None else n
    return a.view(np.uint8).reshape(n, -1) if a.size else np.zeros((n, 0), np.uint8)


def _differ(a, b):
    ra, rb = rows(a), rows(b)
    assert ra.shape == rb.shape, (ra.shape, rb.shape)
    return (ra != rb).any(axis=1)


def differing(a, b):
    """The share of records in which two results differ (same dtype and shape)."""
    d = _differ(a, b)
    return float(d.mean()) if len(d) else 0.0


def poison_differs(poisoned, expected, where=""):
    """The tests' precondition: what the poison gives differs from the expected result in at least a quarter of the records.  A call
    with several per-query outputs (records and counts) has one record per query: it differs where any of its outputs does."""
    d = _differ(poisoned[0], expected[0])
    for p, e in zip(poisoned[1:], expected[1:]):
        d = d | _differ(p, e)
    share = float(d.mean()) if len(d) else 0.0
    assert share >= 0.25, "%s: the poison's result differs from the expected one in %.3f of the records only" % (where, share)


def all_same_bits(got, expected):
    return len(got) == len(expected) and all(same_bits(g, e) for g, e in zip(got, expected))


# ---- the query sets: N queries of each family per scene, from the sets the families' own tests use, and their poison ----
def _take(a, n=N):
    """n rows of `a`, cyclically."""
    return np.ascontiguousarray(a[np.arange(n) % len(a)])


def poison_rays(n=N):
    """Invalid rays by the header's rule (a non-finite component): every row NaN."""
    return np.full((n, 8), np.nan, np.float32)


def poison_points(real):
    """The real positions with maxDist = NaN: invalid by the header's rule."""
    p = np.array(real, np.float32, copy=True)
    p[:, 3] = np.nan
    return p


def poison_boxes(n=N):
    return np.full((n, 6), np.nan, np.float32)


class AsyncSets:
    """The inputs of one scene ("file:coffee" or "spheres"): rays, points (x y z maxDist), boxes and sweeps, N rows each."""

    def __init__(self, kind):
        from box_helpers import box_sets
        from point_helpers import point_case
        from sweep_helpers import sweep_case
        self.kind = kind
        self.pc = point_case(kind)
        self.hs = self.pc.hs
        lo, hi = np.asarray(self.pc.lo, np.float64), np.asarray(self.pc.hi, np.float64)
        self.diag = float(np.linalg.norm(hi - lo))
        self.rays = np.ascontiguousarray(coffee_rays(n=N) if kind == "file:coffee" else box_rays(self.hs, n=N), np.float32)
        pts = _take(self.pc.pts)
        # every other point looks as far as it likes, the others a fifth of the box's diagonal
        md = np.where(np.arange(N) % 2 == 0, np.float32(np.inf), np.float32(0.2 * self.diag)).astype(np.float32)
        self.points = np.ascontiguousarray(np.concatenate([pts, md[:, None]], axis=1), np.float32)
        # the K-nearest walk with COUNT_ALL prunes at maxDist alone: every point of that set has a finite one
        self.points_near = self.points.copy()
        self.points_near[:, 3] = np.float32(0.2 * self.diag)
        # rays aimed at surface points from the ray set's origins: nearly all of them hit, and where the scene is a mesh, the mesh
        target = _take(self.pc.pts[self.pc.parts["near"]]).astype(np.float64)
        d = target - self.rays[:, 0:3].astype(np.float64)
        d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)
        self.aimed = self.rays.copy()
        self.aimed[:, 3:6] = d.astype(np.float32)
        boxes, parts = box_sets(self.pc.geo, lo, hi)
        self.boxes = _take(boxes[:parts["special"].start])      # the uniform and surface boxes: valid ones
        self.sweeps = _take(sweep_case(kind).sweeps)


_sets = {}


def async_sets(kind):
    if kind not in _sets:
        _sets[kind] = AsyncSets(kind)
    return _sets[kind]
