"""The segment queries of the CPU mirror (tests/segmentsim/segmentsim.cpp, a library of its own beside libhostsim.so): the walk through
the kernel's per-segment code, the definition itself as a loop over every primitive record, and the per-primitive distance on explicit
inputs; the segment sets the segment tests share; and a binary64 segment-triangle and segment-sphere distance (numpy) that shares no
code with the mirror."""
import ctypes as C
import os
import subprocess

import numpy as np

from box_helpers import scene_extent
from common import M, REPO, _f32, _ptr, hostsim_handle, hostsim_lib
from point_helpers import Geometry, point_case, tri_dist64      # noqa: F401  (Geometry: for the tests)
from query_helpers import same_bits     # noqa: F401  (for the tests)

SEGMENT_DTYPE = np.dtype([("dist", np.float32), ("prim", np.int32), ("mat", np.int32), ("s", np.float32), ("p", np.float32, (3,)), ("feature", np.int32)])
SEGMENT_CLOSEST, SEGMENT_ANY = 0, 1                       # MOPTIX_SEGMENT_*, spelled out here apart from the package's definition
MODES = dict(closest=SEGMENT_CLOSEST, any=SEGMENT_ANY)
KINDS = dict(tri=0, sphere=1, quad=2)
INF = np.float32(np.inf)

_DIR = os.path.join(REPO, "tests", "segmentsim")
_segmentsim = None


def _lib():
    """tests/segmentsim/libsegmentsim.so (built here if it is missing, as common.hostsim_lib builds its library) with the signatures of
    its entries.  They take the handles of common.HostsimHandle."""
    global _segmentsim
    if _segmentsim is None:
        hostsim_lib()
        path = os.path.join(_DIR, "libsegmentsim.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _DIR, "-s"])
        L = C.CDLL(path)
        vp, f32p = C.c_void_p, C.POINTER(C.c_float)
        L.segmentsim_query.argtypes, L.segmentsim_query.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int, vp], C.c_int
        L.segmentsim_brute.argtypes, L.segmentsim_brute.restype = [vp, f32p, C.c_int64, C.c_int, vp], C.c_int
        L.segmentsim_stack_depth.argtypes, L.segmentsim_stack_depth.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int], C.c_int
        L.segmentsim_dist.argtypes, L.segmentsim_dist.restype = [C.c_int, f32p, f32p, C.c_int64, vp], C.c_int
        _segmentsim = L
    return _segmentsim


def _segments(segments):
    return _f32(np.asarray(segments, np.float32).reshape(-1, 8))


def _out(n, mode):
    return np.zeros(n, SEGMENT_DTYPE if mode == "closest" else np.int32)


def segmentsim(hs, segments, mode="closest", node_format=64, leaf_size=4):
    """moptix_query_segments on the CPU, by the walk: a SEGMENT_DTYPE record array ("closest") or an int32 array ("any").  hs: a scene,
    or a built one."""
    sim = hostsim_handle(hs, leaf_size)
    s = _segments(segments)
    out = _out(len(s), mode)
    assert _lib().segmentsim_query(sim._h, int(node_format), _ptr(s), len(s), MODES[mode], out.ctypes.data) == 0
    return out


def segmentbrute(hs, segments, mode="closest", leaf_size=4):
    """The same from the definition: every primitive record through its distance function, no tree."""
    sim = hostsim_handle(hs, leaf_size)
    s = _segments(segments)
    out = _out(len(s), mode)
    assert _lib().segmentsim_brute(sim._h, _ptr(s), len(s), MODES[mode], out.ctypes.data) == 0
    return out


def segment_stack_depth(hs, segments, mode="closest", node_format=64, leaf_size=4):
    """Most stack entries the walk of any of the segments holds."""
    sim = hostsim_handle(hs, leaf_size)
    s = _segments(segments)
    d = _lib().segmentsim_stack_depth(sim._h, int(node_format), _ptr(s), len(s), MODES[mode])
    assert d >= 0
    return d


def segment_dist(kind, prims, segments):
    """The mirror's per-primitive function of `kind` ("tri": 9 floats, the record's p0, e0 = p1 - p0, e1 = p0 - p2; "sphere": centre and
    radius; "quad": the record's v1, v2, anchor) pair by pair: a SEGMENT_DTYPE array with prim 0 where d2 < maxDist^2, else the miss
    record."""
    s = _segments(segments)
    p = _f32(np.asarray(prims, np.float32).reshape(len(s), -1))
    out = np.zeros(len(s), SEGMENT_DTYPE)
    assert _lib().segmentsim_dist(KINDS[kind], _ptr(p), _ptr(s), len(s), out.ctypes.data) == 0
    return out


def tri_records(tri):
    """Triangles [n, 3, 3] as the device records hold them: p0, e0 = p1 - p0, e1 = p0 - p2, in binary32 (pt_refit.h)."""
    t = np.asarray(tri, np.float32).reshape(-1, 3, 3)
    return np.ascontiguousarray(np.concatenate([t[:, 0], t[:, 1] - t[:, 0], t[:, 0] - t[:, 2]], axis=1), np.float32)


def make_segments(a, b, max_dist=INF):
    """End points [n, 3] each -> [n, 8] queries ax ay az bx by bz maxDist pad; the pad is a value that must not matter."""
    n = len(a)
    md = np.broadcast_to(np.asarray(max_dist, np.float64).reshape(-1, 1) if np.ndim(max_dist) else np.float64(max_dist), (n, 1))
    return np.ascontiguousarray(np.concatenate([np.asarray(a, np.float64), np.asarray(b, np.float64), md, np.full((n, 1), 12345.0)], axis=1), np.float32)


# ---- the segment sets ----
def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def faces_of(geo, rng, n):
    """n triangles [n, 3, 3] of positive area to build segments around, each primitive kind in proportion to its count: random
    triangles of the mesh, halves of the quads, and for a sphere a triangle tangent to it at a random surface point (a third of its
    radius across)."""
    kinds = [k for k, c in (("tri", geo.nt), ("quad", geo.nq), ("sphere", geo.ns)) if c]
    share = {k: max(1, n // len(kinds)) for k in kinds}
    share[kinds[0]] += n - sum(share.values())
    out = []
    for k in kinds:
        m = share[k]
        if k == "tri":
            area = np.linalg.norm(np.cross(geo.tri[:, 1] - geo.tri[:, 0], geo.tri[:, 2] - geo.tri[:, 0]), axis=1)
            good = np.where(area > 0)[0]
            out.append(geo.tri[good[rng.integers(0, len(good), m)]] if len(good) else np.tile(np.eye(3)[None], (m, 1, 1)))
        elif k == "quad":
            i = rng.integers(0, geo.nq, m)
            c = [geo.anchor[i] + a * geo.E1[i] + b * geo.E2[i] for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))]
            first = np.stack([c[0], c[1], c[2]], axis=1)
            second = np.stack([c[0], c[2], c[3]], axis=1)
            out.append(np.where((np.arange(m) % 2 == 0)[:, None, None], first, second))
        else:
            i = rng.integers(0, geo.ns, m)
            nrm = _unit(rng, m)
            t1 = np.cross(nrm, _unit(rng, m)); t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
            t2 = np.cross(nrm, t1)
            p = geo.centre[i] + nrm * geo.radius[i, None]
            w = geo.radius[i, None] / 3.0
            out.append(np.stack([p, p + t1 * w, p + t2 * w], axis=1))
    return np.concatenate(out)[:n]


def _normals(t):
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def invalid_segments(base):
    """Segments that are misses by definition, one defect each, on top of the valid segment `base` (8 floats)."""
    base = np.asarray(base, np.float32)
    rows = []
    for k in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            r = base.copy(); r[k] = bad; rows.append(r)
    for bad in (np.nan, -np.inf, -0.0, 0.0, -1.0):
        r = base.copy(); r[6] = bad; rows.append(r)
    return np.ascontiguousarray(np.array(rows, np.float32))


def valid_segments(segments):
    s = np.asarray(segments, np.float32).reshape(-1, 8)
    return np.isfinite(s[:, :6]).all(axis=1) & (s[:, 6] > 0)


def base_segments(geo, lo, hi, seed=31):
    """The segments of a scene with maxDist = inf, float32 [n, 8], and the slices of the parts:
      uniform    1024: one end uniform in the box lo .. hi, a uniform direction, a length log-uniform from 0.1 % to 100 % of the box diagonal
      edges      1024: edges of faces_of's triangles displaced along the face normal by +0.1 %, -0.1 %, +1 %, -1 % of the diagonal (256 each)
      pierce      512: through a random interior point of a face, from 1 % .. 30 % of the diagonal on one side; rows 0, 1 of every four go on as
                       far beyond it (they cross), rows 2, 3 stop 0.5 % .. 2 % of the diagonal short of it
      parallel    512: 256 parallel to a face above its interior (in the face's plane direction of its first edge, half the edge long),
                       256 parallel to an edge beside it (outside the triangle, in its plane), both at 10^-4 .. 10^-1 of the diagonal
      zero        256: a == b: 128 of uniform's first ends, 128 points near the surface
      invalid     one defect each (invalid_segments)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    diag = max(float(np.linalg.norm(hi - lo)), 1e-30)
    parts, rows, first = {}, [], 0

    def add(name, s):
        nonlocal first
        parts[name] = slice(first, first + len(s)); first += len(s); rows.append(s)
    n = 1024
    a = rng.uniform(lo, hi, (n, 3))
    add("uniform", make_segments(a, a + _unit(rng, n) * (diag * 10.0 ** rng.uniform(-3.0, 0.0, (n, 1)))))
    n = 1024
    t = faces_of(geo, rng, n)
    k = rng.integers(0, 3, n)
    off = diag * np.repeat([1e-3, -1e-3, 1e-2, -1e-2], n // 4)[:, None] * _normals(t)
    add("edges", make_segments(t[np.arange(n), k] + off, t[np.arange(n), (k + 1) % 3] + off))
    n = 512
    t = faces_of(geo, rng, n)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    f = (t * w[:, :, None]).sum(axis=1)
    nrm = _normals(t)
    d = nrm * rng.choice([-1.0, 1.0], (n, 1)) + 0.5 * _unit(rng, n)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    far = diag * rng.uniform(0.01, 0.3, (n, 1))
    short = diag * rng.uniform(0.005, 0.02, (n, 1))
    add("pierce", make_segments(f - d * far, np.where((np.arange(n) % 4 < 2)[:, None], f + d * far, f - d * np.minimum(short, 0.5 * far))))
    n = 256
    t = faces_of(geo, rng, 2 * n)
    nrm = _normals(t)
    h = diag * 10.0 ** rng.uniform(-4.0, -1.0, (2 * n, 1))
    e = t[:, 1] - t[:, 0]
    c = t.mean(axis=1)
    above = make_segments(c[:n] - 0.25 * e[:n] + nrm[:n] * h[:n], c[:n] + 0.25 * e[:n] + nrm[:n] * h[:n])
    out = np.cross(e[n:], nrm[n:]); out /= np.linalg.norm(out, axis=1, keepdims=True)          # in the plane, away from the triangle's first edge
    side = np.sign(((t[n:, 2] - t[n:, 0]) * out).sum(axis=1, keepdims=True))
    out = -out * np.where(side == 0, 1.0, side)
    beside = make_segments(t[n:, 0] + 0.1 * e[n:] + out * h[n:], t[n:, 0] + 0.9 * e[n:] + out * h[n:])
    add("parallel", np.concatenate([above, beside]))
    n = 128
    pts = np.concatenate([rows[0][:n, :3].astype(np.float64), geo.surface_points(rng, n) + _unit(rng, n) * (diag * 10.0 ** rng.uniform(-6.0, -2.0, (n, 1)))])
    add("zero", make_segments(pts, pts))
    add("invalid", invalid_segments(rows[0][0]))
    return np.ascontiguousarray(np.concatenate(rows), np.float32), parts, diag


def with_finite_variants(base, dist, prim, diag):
    """[base (maxDist = inf); base with a finite maxDist]: alternately 0.5 x (even rows) and 2 x (odd rows) the distance the infinite
    query found, and 1 % of the diagonal where that distance is 0 or there is none; the invalid rows as they are."""
    fin = base.copy()
    f = np.where(np.arange(len(base)) % 2 == 0, np.float32(0.5), np.float32(2.0)).astype(np.float32)
    md = (f * dist).astype(np.float32)
    md[(prim < 0) | ~(dist > 0) | ~np.isfinite(md)] = np.float32(0.01 * diag)
    ok = valid_segments(base)
    fin[ok, 6] = md[ok]
    return np.ascontiguousarray(np.concatenate([base, fin]), np.float32)


class SegmentCase:
    """A scene of the point tests (point_helpers.point_case: the scene, its geometry, its box, its leaf-4 mirror handle) with its segment
    set -- base_segments at maxDist = inf and their finite variants from the leaf-4 walk of the 64-byte nodes -- and that walk's answers,
    computed once and only read afterwards."""

    def __init__(self, name):
        self.name = name
        self.pc = point_case(name)
        self.geo = self.pc.geo
        base, self.parts, self.diag = base_segments(self.geo, self.pc.lo, self.pc.hi)
        w = segmentsim(self.pc.sim, base)
        self.segments = with_finite_variants(base, w["dist"], w["prim"], self.diag)
        self.n_base = len(base)
        self.hits = segmentsim(self.pc.sim, self.segments)
        self.anyone = segmentsim(self.pc.sim, self.segments, "any")
        alo, ahi = scene_extent(self.geo)
        self.S = float((ahi - alo).max())                 # the scene's largest extent, every primitive counted

    def finite(self):
        """The rows with a finite maxDist that are valid."""
        rows = np.arange(self.n_base, len(self.segments))
        return rows[valid_segments(self.segments[rows])]


_made = {}


def segment_case(name):
    if name not in _made:
        _made[name] = SegmentCase(name)
    return _made[name]


# ---- the binary64 reference: numpy, no code of the mirror's.  The exact minimum over end-face, edge-edge and crossing ----
def _point_seg64(q, a, b):
    ab = b - a
    den = (ab * ab).sum(axis=1)
    s = np.where(den > 0, np.clip(((q - a) * ab).sum(axis=1) / np.where(den > 0, den, 1.0), 0.0, 1.0), 0.0)
    return np.linalg.norm(q - (a + s[:, None] * ab), axis=1)


def seg_seg_dist64(a, b, c, d):
    """Distances between the segments [a, b] and [c, d], pairwise [n, 3] each.  The squared distance is a convex quadratic over the unit
    square of the two parameters: its minimum is at the interior critical point where that lies in the square, else on the boundary,
    that is at one of the four end-to-segment distances."""
    best = np.minimum(np.minimum(_point_seg64(a, c, d), _point_seg64(b, c, d)), np.minimum(_point_seg64(c, a, b), _point_seg64(d, a, b)))
    u, v, w = b - a, d - c, a - c
    A, B, Cc = (u * u).sum(axis=1), (u * v).sum(axis=1), (v * v).sum(axis=1)
    D, E = (u * w).sum(axis=1), (v * w).sum(axis=1)
    det = A * Cc - B * B
    ok = det > 1e-30 * A * Cc
    det1 = np.where(ok, det, 1.0)
    s, t = (B * E - Cc * D) / det1, (A * E - B * D) / det1
    inside = ok & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
    mid = np.linalg.norm(w + s[:, None] * u - t[:, None] * v, axis=1)
    return np.where(inside, np.minimum(best, mid), best)


def seg_tri_dist64(a, b, t):
    """Distances from the segments [a, b] ([n, 3] each) to the triangles t [n, 3, 3], pairwise: 0 where the segment crosses the
    triangle, else the least of the two ends' distances to the triangle and the three edge-to-segment distances."""
    a, b, t = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(t, np.float64)
    best = np.minimum(tri_dist64(a, t)[0], tri_dist64(b, t)[0])
    for i, j in ((0, 1), (1, 2), (2, 0)):
        best = np.minimum(best, seg_seg_dist64(a, b, t[:, i], t[:, j]))
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    ha, hb = ((a - t[:, 0]) * n).sum(axis=1), ((b - t[:, 0]) * n).sum(axis=1)
    straddle = (ha * hb <= 0) & (ha != hb)
    s = np.where(straddle, ha / np.where(straddle, ha - hb, 1.0), 0.0)
    x = a + s[:, None] * (b - a)
    inside = straddle
    for i, j in ((0, 1), (1, 2), (2, 0)):
        inside = inside & ((np.cross(t[:, j] - t[:, i], x - t[:, i]) * n).sum(axis=1) >= 0)
    return np.where(inside, 0.0, best)


def seg_sphere_dist64(a, b, centre, radius):
    """Distances from the segments to the sphere surfaces: dmin - R outside, R - dmax inside, 0 where dmin <= R <= dmax."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dmin = _point_seg64(centre, a, b)
    dmax = np.maximum(np.linalg.norm(a - centre, axis=1), np.linalg.norm(b - centre, axis=1))
    return np.where(dmin > radius, dmin - radius, np.where(dmax < radius, radius - dmax, 0.0))


def scene_dist64(geo, segments, upper):
    """Binary64 distance from every segment to the whole scene.  upper[i]: any valid upper bound of it (the mirror's distance; slack is
    added here).  Triangles whose bounding sphere lies beyond the bound from the segment are left out, which changes no minimum."""
    s = np.asarray(segments, np.float64)
    a, b = s[:, 0:3], s[:, 3:6]
    best = np.full(len(s), np.inf)
    for i in range(geo.ns):
        best = np.minimum(best, seg_sphere_dist64(a, b, geo.centre[i][None], geo.radius[i]))
    for k in range(geo.nq):
        c = [geo.anchor[k] + u * geo.E1[k] + v * geo.E2[k] for u, v in ((0, 0), (1, 0), (1, 1), (0, 1))]
        for tri in ([c[0], c[1], c[2]], [c[0], c[2], c[3]]):
            best = np.minimum(best, seg_tri_dist64(a, b, np.broadcast_to(np.array(tri)[None], (len(s), 3, 3))))
    if not geo.nt:
        return best
    cen = geo.tri.mean(axis=1)
    rad = np.linalg.norm(geo.tri - cen[:, None, :], axis=2).max(axis=1)
    scale = max(float(np.abs(geo.tri).max()), float(np.abs(s[:, :6]).max()))
    reach = np.asarray(upper, np.float64) * 1.001 + 1e-6 * scale
    for i in range(len(s)):
        near = _point_seg64(cen, a[i][None], b[i][None]) <= reach[i] + rad
        if near.any():
            m = int(near.sum())
            best[i] = min(best[i], seg_tri_dist64(np.broadcast_to(a[i], (m, 3)), np.broadcast_to(b[i], (m, 3)), geo.tri[near]).min())
    return best


# ---- exact cases: one axis-aligned triangle, dyadic values, every intermediate of the definition exact ----
def exact_mesh_scene():
    """Two faces alone in a scene: 0 the triangle (0,0,0) (4,0,0) (0,4,0); 1 a small one far away."""
    from common import MovedScene
    from sign_helpers import _mesh_only
    t = [[0, 0, 0, 4, 0, 0, 0, 4, 0], [100, 100, 100, 101, 100, 100, 100, 101, 100]]
    return _mesh_only(MovedScene(M.HostScene("file:coffee", 64, 36), np.array(t, np.float32), new_faces=True))


def _rec(dist, prim, mat, s, p, feature):
    r = np.zeros(1, SEGMENT_DTYPE)
    r["dist"], r["prim"], r["mat"], r["s"], r["p"], r["feature"] = dist, prim, mat, s, p, feature
    return r


def exact_mesh_cases():
    """(names, segments [k, 8], expected records [k]) on exact_mesh_scene."""
    miss = lambda md: _rec(md, -1, -1, 0, (0, 0, 0), 0)
    rows = [("above the interior, parallel to it: the first end", [1, 1, 2, 2, 1, 2, 8, 0], _rec(2, 0, 0, 0, (1, 1, 0), 0)),
            ("crossing the interior", [1, 1, -1, 1, 1, 1, 8, 0], _rec(0, 0, 0, 0.5, (1, 1, 0), 5)),
            ("beside an edge, across it: edge 0", [1, -2, -1, 1, -2, 1, 8, 0], _rec(2, 0, 0, 0.5, (1, 0, 0), 2)),
            ("beyond a vertex, in the plane: edge 0 at its end, before edge 2 at its start", [6, -2, 0, 6, 2, 0, 8, 0], _rec(2, 0, 0, 0.5, (4, 0, 0), 2)),
            ("end b nearest", [1, 1, 4, 1, 1, 2, 8, 0], _rec(2, 0, 0, 1, (1, 1, 0), 1)),
            ("touching at maxDist exactly: the bound is exclusive", [1, 1, 2, 2, 1, 2, 2, 0], miss(2)),
            ("an ulp more reaches it", [1, 1, 2, 2, 1, 2, np.nextafter(np.float32(2), np.float32(3)), 0], _rec(2, 0, 0, 0, (1, 1, 0), 0))]
    return [r[0] for r in rows], np.array([r[1] for r in rows], np.float32), np.concatenate([r[2] for r in rows])


CROSSING_NOISE = 2.0 ** -19            # pt_segment.h "the crossing": the one number the header, the tests and the profile share


def crossing_slack(geo, segments, prim):
    """How far from the binary64 distance an answer may lie because of the crossing candidate, per row, from binary64 geometry and the
    winning primitive alone (never from the answer's dist or feature).  The ray queries' triangle test decides a crossing from
    t = n.(p0 - a) / n.(b - a) and two barycentrics of the same form; each numerator and denominator carries rounding noise of
    CROSSING_NOISE x (|b - a| + the largest |vertex - a|) in space.  So where the segment comes within that noise of the primitive's plane
    (it straddles it, or its nearer end is that close), the point where it meets the plane is known to noise / sin(angle to the plane)
    only, a crossing may be reported or not for a meeting point that far outside or inside the primitive's outline, and the distance is
    off by up to as much.  0 for a sphere, a miss, a zero-length segment (its triangle test sees 1 / 0 and never accepts) and a segment
    further from the plane than the noise; inf for a segment in the plane."""
    s = np.asarray(segments, np.float64)
    a, b = s[:, 0:3], s[:, 3:6]
    out = np.zeros(len(s))
    for i in np.where(prim >= geo.ns)[0]:
        if prim[i] < geo.ns + geo.nq:
            k = prim[i] - geo.ns
            v = np.array([geo.anchor[k] + u * geo.E1[k] + w * geo.E2[k] for u, w in ((0, 0), (1, 0), (1, 1), (0, 1))])
        else:
            v = geo.tri[prim[i] - geo.ns - geo.nq]
        n = np.cross(v[1] - v[0], v[2] - v[0])
        d = b[i] - a[i]
        ln, L = np.linalg.norm(n), np.linalg.norm(d)
        if L == 0:
            continue
        noise = CROSSING_NOISE * (L + np.linalg.norm(v - a[i], axis=1).max())
        if ln == 0:
            out[i] = np.inf
            continue
        ha, hb = float(n @ (a[i] - v[0])) / ln, float(n @ (b[i] - v[0])) / ln
        h = 0.0 if ha * hb <= 0 else min(abs(ha), abs(hb))
        if h <= noise:
            sine = abs(float(n @ d)) / (ln * L)
            out[i] = noise / sine if sine > 0 else np.inf
    return out
