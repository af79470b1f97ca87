"""The frustum queries of the CPU mirror (tests/frustumsim/frustumsim.cpp, a library of its own beside libhostsim.so): the walk through the
kernel's per-query code and the definition itself as a loop over every primitive record; the query sets the frustum tests share; and an
exact rational reference -- Sutherland-Hodgman clipping of the triangle by the six half-spaces in Python fractions, on the float inputs
themselves -- which shares no code with the mirror."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np

from box_helpers import BOX_ANY, BOX_COUNT, MODES, csr, membership, scene_extent      # noqa: F401  (for the tests)
from common import M, REPO, _f32, _ptr, hostsim_handle, hostsim_lib
from obb_helpers import frame_from, padded_boxes_meeting, random_rotations              # noqa: F401  (for the tests)
from point_helpers import Geometry      # noqa: F401  (for the tests)
from query_helpers import same_bits     # noqa: F401  (for the tests)

STAGES = {-1: "invalid", 0: "none", 1: "R", 2: "A", 3: "E", 4: "V"}        # pt_frustum.h FRUSTUM_*, spelled out here
R, A, E, V = 1, 2, 3, 4

_DIR = os.path.join(REPO, "tests", "frustumsim")
_frustumsim = None


def _lib():
    """tests/frustumsim/libfrustumsim.so (built here if it is missing, as common.hostsim_lib builds its library) with the signatures of
    its entries.  They take the handles of common.HostsimHandle."""
    global _frustumsim
    if _frustumsim is None:
        hostsim_lib()
        path = os.path.join(_DIR, "libfrustumsim.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _DIR, "-s"])
        L = C.CDLL(path)
        vp, f32p, i32p, i64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        L.frustumsim_query.argtypes, L.frustumsim_query.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int, i32p], C.c_int
        L.frustumsim_list.argtypes, L.frustumsim_list.restype = [vp, C.c_int, f32p, C.c_int64, i64p, i32p, i32p], C.c_int
        L.frustumsim_brute.argtypes, L.frustumsim_brute.restype = [vp, f32p, C.c_int64, C.c_int, i32p], C.c_int
        L.frustumsim_brute_list.argtypes, L.frustumsim_brute_list.restype = [vp, f32p, C.c_int64, i64p, i32p, i32p], C.c_int
        L.frustumsim_stack_depth.argtypes, L.frustumsim_stack_depth.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int], C.c_int
        L.frustumsim_work.argtypes, L.frustumsim_work.restype = [vp, C.c_int, f32p, C.c_int64, i64p, i64p], C.c_int
        L.frustumsim_tri.argtypes, L.frustumsim_tri.restype = [f32p, f32p, C.c_int64, i32p, i32p], C.c_int
        for name in ("frustumsim_sphere", "frustumsim_quad"):
            getattr(L, name).argtypes, getattr(L, name).restype = [f32p, f32p, C.c_int64, i32p], C.c_int
        _frustumsim = L
    return _frustumsim


def _rows(frusta):
    return _f32(np.asarray(frusta, np.float32).reshape(-1, 24))


def frustumsim(hs, frusta, mode="any", node_format=64, leaf_size=4):
    """moptix_query_frusta on the CPU, by the walk: int32 per query.  hs: a scene, or a built one."""
    sim = hostsim_handle(hs, leaf_size)
    b = _rows(frusta)
    out = np.zeros(len(b), np.int32)
    assert _lib().frustumsim_query(sim._h, int(node_format), _ptr(b), len(b), MODES[mode], _ptr(out, C.c_int32)) == 0
    return out


def frustumbrute(hs, frusta, mode="any", leaf_size=4):
    """The same from the definition: every primitive record through its predicate, no tree."""
    sim = hostsim_handle(hs, leaf_size)
    b = _rows(frusta)
    out = np.zeros(len(b), np.int32)
    assert _lib().frustumsim_brute(sim._h, _ptr(b), len(b), MODES[mode], _ptr(out, C.c_int32)) == 0
    return out


def _list(entry, sim, b, offsets, fill):
    offsets = np.ascontiguousarray(offsets, np.int64)
    prims = np.full(int(offsets[-1]) if len(offsets) else 0, fill, np.int32)
    counts = np.zeros(len(b), np.int32)
    keep = np.zeros(1, np.int32) if len(prims) == 0 else prims      # a valid address for an empty list
    assert entry(sim, _ptr(b), len(b), _ptr(offsets, C.c_int64), _ptr(keep, C.c_int32), _ptr(counts, C.c_int32)) == 0
    return prims, counts


def frustumsim_list(hs, frusta, offsets, node_format=64, leaf_size=4, fill=-7):
    """moptix_query_frusta_list on the CPU, by the walk: (prims, counts); prims starts out as `fill` throughout."""
    sim = hostsim_handle(hs, leaf_size)
    L = _lib()
    return _list(lambda s, *a: L.frustumsim_list(s._h, int(node_format), *a), sim, _rows(frusta), offsets, fill)


def frustumbrute_list(hs, frusta, offsets, leaf_size=4, fill=-7):
    """The same from the definition, the ids sorted by the library's sort."""
    sim = hostsim_handle(hs, leaf_size)
    L = _lib()
    return _list(lambda s, *a: L.frustumsim_brute_list(s._h, *a), sim, _rows(frusta), offsets, fill)


def frustum_stack_depth(hs, frusta, mode="count", node_format=64, leaf_size=4):
    """Most stack entries the walk of any of the queries holds."""
    sim = hostsim_handle(hs, leaf_size)
    b = _rows(frusta)
    d = _lib().frustumsim_stack_depth(sim._h, int(node_format), _ptr(b), len(b), MODES[mode])
    assert d >= 0
    return d


def frustum_work(hs, frusta, node_format=64, leaf_size=4):
    """(node steps, triangles tested) of the count walk, int64 per query."""
    sim = hostsim_handle(hs, leaf_size)
    b = _rows(frusta)
    steps, tested = np.zeros(len(b), np.int64), np.zeros(len(b), np.int64)
    assert _lib().frustumsim_work(sim._h, int(node_format), _ptr(b), len(b), _ptr(steps, C.c_int64), _ptr(tested, C.c_int64)) == 0
    return steps, tested


def predicate(kind, prims, frusta):
    """The mirror's predicate `kind` ("tri": 9 floats, three vertices; "sphere": centre and radius; "quad": the record's v1, v2, anchor)
    pair by pair: prims [n, 9 or 4], frusta [n, 24] -> bool [n]; for "tri" the pair (bool [n], stage int32 [n])."""
    p, b = _f32(prims), _rows(frusta)
    assert len(p) == len(b)
    out = np.zeros(len(b), np.int32)
    if kind == "tri":
        stage = np.zeros(len(b), np.int32)
        assert _lib().frustumsim_tri(_ptr(p), _ptr(b), len(b), _ptr(out, C.c_int32), _ptr(stage, C.c_int32)) == 0
        return out != 0, stage
    assert getattr(_lib(), "frustumsim_" + kind)(_ptr(p), _ptr(b), len(b), _ptr(out, C.c_int32)) == 0
    return out != 0


# ---- building queries (binary64 planes [n, 6, 4]; rounded once by pack) ----
def pack(planes):
    return np.ascontiguousarray(np.asarray(planes, np.float64).reshape(-1, 24), np.float32)


def through(normal, point):
    """Planes [n, 4] with the normals [n, 3] through the points [n, 3]."""
    normal, point = np.asarray(normal, np.float64), np.asarray(point, np.float64)
    return np.concatenate([normal, -(normal * point).sum(axis=1, keepdims=True)], axis=1)


def box_planes(centre, half, axes):
    """The six planes [n, 6, 4] of oriented boxes: centres [n, 3], half-extents [n, 3], axes [n, 3, 3] (rows)."""
    c, h, a = np.asarray(centre, np.float64), np.asarray(half, np.float64), np.asarray(axes, np.float64)
    out = []
    for j in range(3):
        out.append(through(a[:, j], c - a[:, j] * h[:, j:j + 1]))
        out.append(through(-a[:, j], c + a[:, j] * h[:, j:j + 1]))
    return np.stack(out, axis=1)


def aabb_planes(boxes):
    """The six planes [n, 24] float32 of axis-aligned boxes [n, 6] lo, hi: unit normals and the box's own floats, nothing rounded."""
    b = np.asarray(boxes, np.float32).reshape(-1, 6)
    out = np.zeros((len(b), 6, 4), np.float32)
    for k in range(3):
        out[:, 2 * k, k] = 1.0; out[:, 2 * k, 3] = -b[:, k]
        out[:, 2 * k + 1, k] = -1.0; out[:, 2 * k + 1, 3] = b[:, 3 + k]
    return out.reshape(-1, 24)


def perspective(eye, frames, tan_x, tan_y, near, far):
    """Perspective frusta [n, 6, 4]: apex eye [n, 3], frames [n, 3, 3] whose row 0 is the view direction, half-angle tangents, near and
    far distances along the view direction.  Order left, right, bottom, top, near, far."""
    eye, f = np.asarray(eye, np.float64), np.asarray(frames, np.float64)
    w, u, v = f[:, 0], f[:, 1], f[:, 2]
    tx, ty = np.asarray(tan_x, np.float64)[:, None], np.asarray(tan_y, np.float64)[:, None]
    near, far = np.asarray(near, np.float64)[:, None], np.asarray(far, np.float64)[:, None]
    return np.stack([through(u + tx * w, eye), through(-u + tx * w, eye), through(v + ty * w, eye), through(-v + ty * w, eye),
                     through(w, eye + near * w), through(-w, eye + far * w)], axis=1)


def scene_camera(hs):
    """The scene's own camera as the mapping camera_frusta takes, from the params alone."""
    cam = hs.params.cam
    v3 = lambda v: [float(v.x), float(v.y), float(v.z)]
    return dict(origin=v3(cam.origin), horizontal=v3(cam.horizontal), vertical=v3(cam.vertical), scrLowerLeftCorner=v3(cam.scrLowerLeftCorner))


def tiles(k):
    """The k x k split of the frame as rects [k * k, 4]."""
    e = np.linspace(0.0, 1.0, k + 1)
    return np.array([[e[i], e[j], e[i + 1], e[j + 1]] for j in range(k) for i in range(k)])


def scale_planes(frusta, rng, lo=-20, hi=20):
    """Every plane of every query multiplied by its own power of two 2^k, k in lo .. hi."""
    f = np.asarray(frusta, np.float32).reshape(-1, 6, 4)
    k = rng.integers(lo, hi + 1, f.shape[:2])
    return np.ascontiguousarray((f * np.exp2(k)[:, :, None].astype(np.float32)).reshape(-1, 24), np.float32)


def frustum_sets(hs, geo, lo, hi, seed=31):
    """The queries of a scene as one float32 [n, 24] array (about 900) and the slices of its parts:
      tiles     camera_frusta on the scene's own camera: the whole frame, the 4 x 4 and the 8 x 8 split, and the 4 x 4 split between
                near and far distances of a tenth and twice the scene's diagonal
      persp     320 random perspective frusta, apex uniform in the scene box enlarged by half its size or on the surface, uniform random
                directions, half-angles 1 to 50 degrees, far distance diag x 10^k, k uniform in [-3, 0] (0.1 % to 100 % of the
                scene), near a random fraction of it
      beams     64 boxes of 100 : 1 on diagonals, as six planes
      wedges    48: two planes through a surface point, four zero planes
      slabs     48: two parallel planes, thickness 0.01 % to 10 % of the diagonal, four zero planes
      halves    48: one plane through a surface point (or outside the scene), five zero planes (some with d > 0)
      thin      48 regions that are a point or a segment: boxes with three or two zero half-extents on mesh vertices / surface points
      empty     16 with contradictory planes: a slab of negative thickness; a perspective frustum with far < near
      void      8: a valid region and one plane 0 0 0 -1
      zero      4: six planes 0 0 0 d with d = 0, -0, 1 and mixed
      scaled    64 of persp with every plane multiplied by a power of two 2^-20 .. 2^20
      invalid   48: NaN and +-infinity, each of the 24 slots once with one and once with another
    """
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    diag = max(float(np.linalg.norm(hi - lo)), 1e-30)
    size = np.maximum(hi - lo, 1e-3 * diag)
    parts, rows = {}, []
    zero = np.zeros((1, 4))

    def add(name, planes):
        block = pack(planes) if np.asarray(planes).dtype != np.float32 else np.asarray(planes).reshape(-1, 24)
        first = sum(len(r) for r in rows)
        rows.append(block); parts[name] = slice(first, first + len(block))

    def padded(planes):                     # [n, k, 4] -> [n, 6, 4] with zero planes behind
        planes = np.asarray(planes, np.float64)
        return np.concatenate([planes, np.zeros((len(planes), 6 - planes.shape[1], 4))], axis=1)

    cam = scene_camera(hs)
    add("tiles", np.concatenate([M.camera_frusta(cam, [[0, 0, 1, 1]]), M.camera_frusta(cam, tiles(4)), M.camera_frusta(cam, tiles(8)),
                                 M.camera_frusta(cam, tiles(4), 0.1 * diag, 2.0 * diag)]))
    n = 320
    eye = np.concatenate([rng.uniform(lo - 0.5 * size, hi + 0.5 * size, (n // 2, 3)), geo.surface_points(rng, n - n // 2)])
    far = diag * 10.0 ** rng.uniform(-3.0, 0.0, n)
    tan = np.tan(np.radians(rng.uniform(1.0, 50.0, (n, 2))))
    persp = perspective(eye, random_rotations(rng, n), tan[:, 0], tan[:, 1], far * rng.uniform(0.0, 0.5, n), far)
    add("persp", persp)
    n = 64
    long_half = diag * rng.uniform(0.05, 0.30, n)
    diagonals = [(1, 1, 1), (1, -1, 1), (-1, 1, 1), (1, 1, -1), (1, 1, 0), (1, 0, -1), (0, 1, 1), (1, -1, 0)]
    add("beams", box_planes(geo.surface_points(rng, n), np.stack([long_half, long_half / 100, long_half / 100], axis=1),
                            np.array([frame_from(diagonals[i % 8]) for i in range(n)])))
    n = 48
    p, r = geo.surface_points(rng, n), random_rotations(rng, n)
    add("wedges", padded(np.stack([through(r[:, 0], p), through(r[:, 1] * np.cos(0.3) + r[:, 0] * np.sin(0.3) * rng.choice([-1, 1], (n, 1)), p)], axis=1)))
    p, r, t = geo.surface_points(rng, n), random_rotations(rng, n), diag * 10.0 ** rng.uniform(-4.0, -1.0, (n, 1))
    slabs = padded(np.stack([through(r[:, 0], p - 0.5 * t * r[:, 0]), through(-r[:, 0], p + 0.5 * t * r[:, 0])], axis=1))
    add("slabs", slabs[:, rng.permutation(6)])
    p, r = np.concatenate([geo.surface_points(rng, n - 8), hi + size * rng.uniform(1.0, 2.0, (8, 3))]), random_rotations(rng, n)
    halves = padded(through(r[:, 0], p)[:, None, :])
    halves[::3, 1:, 3] = rng.uniform(0.0, 2.0, (len(halves[::3]), 5))
    add("halves", halves)
    if geo.nt:
        v = geo.tri.reshape(-1, 3)[rng.integers(0, 3 * geo.nt, n)]
    else:
        v = geo.surface_points(rng, n)
    h = np.zeros((n, 3)); h[1::2, 0] = diag * rng.uniform(0.01, 0.2, n // 2)
    axes = random_rotations(rng, n); axes[::4] = np.eye(3)
    add("thin", box_planes(v.astype(np.float32).astype(np.float64), h, axes))
    e1 = slabs[:8].copy(); e1[:, :, 3] -= np.where(np.abs(e1[:, :, :3]).sum(axis=2) > 0, diag * 0.2, 0.0)        # thickness at most 0.1 diag
    e2 = perspective(eye[:8], random_rotations(rng, 8), tan[:8, 0], tan[:8, 1], far[:8], 0.5 * far[:8])
    e3 = persp[8:16].copy(); e3[:, 5] = [0, 0, 0, -1]
    add("empty", np.concatenate([e1, e2]))
    add("void", e3)
    z = np.zeros((4, 6, 4)); z[1, :, 3] = -0.0; z[2, :, 3] = 1.0; z[3, ::2, 3] = 3.0
    add("zero", z)
    add("scaled", scale_planes(pack(persp[:64]), rng))
    whole = pack(box_planes([0.5 * (lo + hi)], [np.full(3, diag)], np.eye(3)[None]))
    bad = np.repeat(whole, 48, axis=0)
    vals = (np.nan, np.inf, -np.inf)
    for k in range(24):
        bad[k, k] = vals[k % 3]; bad[24 + k, k] = vals[(k + 1) % 3]
    add("invalid", bad)
    frusta = np.ascontiguousarray(np.concatenate(rows), np.float32)
    parts["whole_box"] = whole
    return frusta, parts


def valid_frusta(frusta):
    return np.isfinite(np.asarray(frusta, np.float32).reshape(-1, 24)).all(axis=1)


def enclosing_aabb(frusta, clip_lo, clip_hi):
    """The axis-aligned box [n, 6] float32 round each bounded region: the corners of the region (the crossings of three planes that satisfy
    the others, binary64), clamped to clip_lo .. clip_hi; rows of NaN where the region has no corner."""
    f = np.asarray(frusta, np.float64).reshape(-1, 6, 4)
    out = np.full((len(f), 6), np.nan, np.float32)
    trip = [(a, b, c) for a in range(6) for b in range(a + 1, 6) for c in range(b + 1, 6)]
    for i, q in enumerate(f):
        pts = []
        for t in trip:
            m = q[list(t), :3]
            if abs(np.linalg.det(m)) < 1e-12 * np.prod(np.linalg.norm(m, axis=1)) or not np.isfinite(m).all():
                continue
            x = np.linalg.solve(m, -q[list(t), 3])
            if (q[:, :3] @ x + q[:, 3] >= -1e-9 * (np.abs(q[:, :3]) @ np.abs(x) + np.abs(q[:, 3]))).all():
                pts.append(x)
        if pts:
            pts = np.clip(np.array(pts), clip_lo, clip_hi)
            out[i, :3] = np.nextafter(pts.min(axis=0).astype(np.float32), np.float32(-np.inf))
            out[i, 3:] = np.nextafter(pts.max(axis=0).astype(np.float32), np.float32(np.inf))
    return out


# ---- the exact reference: Sutherland-Hodgman in rationals ----
def _frac3(p):
    return [Fraction(float(p[0])), Fraction(float(p[1])), Fraction(float(p[2]))]


def tri_region_exact(tri, planes, tau=0):
    """Does the triangle [3, 3] meet the region of the planes [6, 4], each moved by tau x (|nx| + |ny| + |nz|) (tau > 0 grows the region,
    tau < 0 shrinks it; a Fraction or 0), in exact rational arithmetic on the float inputs: the triangle is clipped by one half-space after
    the other as a polygon; what is left is empty or not.  Degenerate triangles and zero planes need no special case."""
    poly = [_frac3(v) for v in np.asarray(tri, np.float64).reshape(3, 3)]
    tau = Fraction(tau)
    for p in np.asarray(planes, np.float64).reshape(6, 4):
        nx, ny, nz, d = (Fraction(float(x)) for x in p)
        d = d + tau * (abs(nx) + abs(ny) + abs(nz))
        s = [nx * v[0] + ny * v[1] + nz * v[2] + d for v in poly]
        out = []
        m = len(poly)
        for i in range(m):
            a, b, sa, sb = poly[i], poly[(i + 1) % m], s[i], s[(i + 1) % m]
            if sa >= 0:
                out.append(a)
            if (sa < 0) != (sb < 0) and sa != 0 and sb != 0 and m > 1:
                t = sa / (sa - sb)
                out.append([a[k] + t * (b[k] - a[k]) for k in range(3)])
        poly = out
        if not poly:
            return False
    return True


def pair_scale(tri, planes):
    """What a tolerance of a pair is relative to: the largest |coordinate| of the triangle and the largest distance |d| / (|nx| + |ny| +
    |nz|) of a plane from the origin in the same norm."""
    p = np.asarray(planes, np.float64).reshape(6, 4)
    nb = np.abs(p[:, :3]).sum(axis=1)
    dist = np.where(nb > 0, np.abs(p[:, 3]) / np.where(nb > 0, nb, 1.0), 0.0)
    return max(float(np.abs(np.asarray(tri, np.float64)).max()), float(dist.max()), 1e-300)


def smallest_tau(tri, planes, got, lo=2.0 ** -40, hi=2.0 ** -10):
    """The smallest tau / scale (to a factor 2^(1/4)) at which the mirror's verdict `got` agrees with the exact one: for a pair it
    accepts, exact on the region grown by tau; for one it rejects, not exact on the region shrunk by tau.  0 where they agree at tau = 0;
    inf where hi does not suffice."""
    if tri_region_exact(tri, planes) == bool(got):
        return 0.0
    scale = Fraction(pair_scale(tri, planes))
    ok = lambda rel: tri_region_exact(tri, planes, Fraction(rel) * scale if got else -Fraction(rel) * scale) == bool(got)
    if not ok(hi):
        return float("inf")
    a, b = np.log2(lo), np.log2(hi)
    if ok(lo):
        return lo
    while b - a > 0.25:
        mid = 0.5 * (a + b)
        if ok(2.0 ** mid):
            b = mid
        else:
            a = mid
    return 2.0 ** b


def predicate_pairs(seed=32, n=5400):
    """(tris [n, 3, 3] float32, frusta [n, 24] float32) for the comparison with exact rationals: random frusta and boxes in a unit scene
    (centres within +-1, sizes 0.02 to 1), triangles biased towards the region's size and placed on or near its boundary; a third of the
    pairs degenerate triangles (points, segments, collinear) or reduced plane sets (wedges, slabs, half-spaces, zero planes)."""
    rng = np.random.default_rng(seed)
    size = 10.0 ** rng.uniform(-1.7, 0.0, n)
    centre = rng.uniform(-1.0, 1.0, (n, 3))
    rot = random_rotations(rng, n)
    tan = np.tan(np.radians(rng.uniform(2.0, 45.0, (n, 2))))
    planes = perspective(centre - rot[:, 0] * size[:, None], rot, tan[:, 0], tan[:, 1], 0.5 * size, 1.5 * size)
    boxes = box_planes(centre, size[:, None] * rng.uniform(0.05, 0.5, (n, 3)), rot)
    planes[1::4] = boxes[1::4]
    # triangles: a centre near the region (within 1.5 sizes), an extent of 0.3 to 6 region sizes: the large ones surround the region (V) or
    # cut it with an edge (E), the small ones fall in or out (A, R)
    ext = size * 10.0 ** rng.uniform(-0.5, 0.8, n)
    tc = centre + rng.normal(size=(n, 3)) * (0.5 * size)[:, None]
    tris = tc[:, None, :] + rng.normal(size=(n, 3, 3)) * ext[:, None, None]
    # a fifth: a large triangle through the region's centre, whose plane cuts it and whose edges pass far outside (V)
    k = np.arange(0, n, 5)
    rng.choice([-1, 1], (len(k), 1))                                     # a draw that is not used: the figures recorded for this set were measured on the stream behind it
    mix = random_rotations(rng, len(k))
    a, b = mix[:, 0], mix[:, 1]
    big = (size[k] * rng.uniform(3.0, 8.0, len(k)))[:, None]
    c = centre[k] + rng.normal(size=(len(k), 3)) * (0.1 * size[k])[:, None]
    tris[k] = np.stack([c + big * a, c + big * (-0.5 * a + 0.866 * b), c + big * (-0.5 * a - 0.866 * b)], axis=1)
    # a seventh: touching up to rounding -- vertex 0 on a face of the region (the centre's foot on a plane), the others on the outer side
    k = np.arange(3, n, 7)
    j = rng.integers(0, 6, len(k))
    pl = planes[k, j]
    nn = (pl[:, :3] ** 2).sum(axis=1)
    foot = centre[k] - pl[:, :3] * ((pl[:, :3] * centre[k]).sum(axis=1) + pl[:, 3])[:, None] / nn[:, None]
    for m in (1, 2):
        d = rng.normal(size=(len(k), 3)) * ext[k, None]
        out = (d * pl[:, :3]).sum(axis=1)
        d -= pl[:, :3] * (np.maximum(out, 0.0) * 2.0 / nn)[:, None]          # mirrored to the outer side
        tris[k, m] = foot + d
    tris[k, 0] = foot
    # degenerate triangles
    k = np.arange(2, n, 9)
    tris[k, 1] = tris[k, 0]; tris[k[::3], 2] = tris[k[::3], 0]                       # segments; every third a point
    k = np.arange(4, n, 9)
    tris[k, 2] = tris[k, 0] + (tris[k, 1] - tris[k, 0]) * rng.uniform(-1.0, 2.0, (len(k), 1))      # collinear (up to rounding)
    # reduced plane sets
    k = np.arange(1, n, 6)
    for i in k:
        keep = rng.permutation(6)[:rng.integers(0, 4)]
        drop = np.setdiff1d(np.arange(6), keep)
        planes[i, drop] = 0.0
        if rng.uniform() < 0.3:
            planes[i, drop[0], 3] = rng.uniform(0.0, 1.0)
    return np.ascontiguousarray(tris, np.float32), pack(planes)
