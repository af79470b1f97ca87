"""The triangle queries of the CPU mirror (tests/trisim/trisim.cpp, a library of its own beside libhostsim.so): the walk through the
kernel's per-query code and the definition itself as a loop over every primitive record; the query sets the triangle tests share; and two
evaluations of a pair of triangles that share no code with the mirror and none with each other:
  * tri_tri_exact: exact, on Python integers or fractions.Fraction, written without an axis list -- does an edge of one cross the other,
    both ways, with a coplanar case (which holds containment) and the degenerate cases;
  * tri_tri_dist64 and penetration64: binary64, numpy -- d, the distance between the two triangles (0 where they intersect), and p, the
    penetration: the least normalised overlap of the two projections over the 23 axes."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np

from box_helpers import BOX_ANY, BOX_COUNT, MODES, csr, membership, scene_extent      # noqa: F401  (for the tests)
from common import REPO, _f32, _ptr, hostsim_handle, hostsim_lib
from obb_helpers import random_rotations
from point_helpers import Geometry, tri_dist64      # noqa: F401  (for the tests)
from query_helpers import same_bits     # noqa: F401  (for the tests)

_DIR = os.path.join(REPO, "tests", "trisim")
_trisim = None


def _lib():
    """tests/trisim/libtrisim.so (built here if it is missing, as common.hostsim_lib builds its library) with the signatures of its
    entries.  They take the handles of common.HostsimHandle."""
    global _trisim
    if _trisim is None:
        hostsim_lib()
        path = os.path.join(_DIR, "libtrisim.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _DIR, "-s"])
        L = C.CDLL(path)
        vp, f32p, i32p, i64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        L.trisim_query.argtypes, L.trisim_query.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int, i32p], C.c_int
        L.trisim_list.argtypes, L.trisim_list.restype = [vp, C.c_int, f32p, C.c_int64, i64p, i32p, i32p], C.c_int
        L.trisim_brute.argtypes, L.trisim_brute.restype = [vp, f32p, C.c_int64, C.c_int, i32p], C.c_int
        L.trisim_brute_list.argtypes, L.trisim_brute_list.restype = [vp, f32p, C.c_int64, i64p, i32p, i32p], C.c_int
        L.trisim_stack_depth.argtypes, L.trisim_stack_depth.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int], C.c_int
        for name in ("trisim_tri", "trisim_sphere", "trisim_quad"):
            getattr(L, name).argtypes, getattr(L, name).restype = [f32p, f32p, C.c_int64, i32p], C.c_int
        _trisim = L
    return _trisim


def _tris(tris):
    return _f32(np.asarray(tris, np.float32).reshape(-1, 9))


def trisim(hs, tris, mode="any", node_format=64, leaf_size=4):
    """moptix_query_tris on the CPU, by the walk: int32 per query.  hs: a scene, or a built one."""
    sim = hostsim_handle(hs, leaf_size)
    b = _tris(tris)
    out = np.zeros(len(b), np.int32)
    assert _lib().trisim_query(sim._h, int(node_format), _ptr(b), len(b), MODES[mode], _ptr(out, C.c_int32)) == 0
    return out


def tribrute(hs, tris, mode="any", leaf_size=4):
    """The same from the definition: every primitive record through its predicate, no tree."""
    sim = hostsim_handle(hs, leaf_size)
    b = _tris(tris)
    out = np.zeros(len(b), np.int32)
    assert _lib().trisim_brute(sim._h, _ptr(b), len(b), MODES[mode], _ptr(out, C.c_int32)) == 0
    return out


def _list(entry, sim, b, offsets, fill):
    offsets = np.ascontiguousarray(offsets, np.int64)
    prims = np.full(int(offsets[-1]) if len(offsets) else 0, fill, np.int32)
    counts = np.zeros(len(b), np.int32)
    keep = np.zeros(1, np.int32) if len(prims) == 0 else prims      # a valid address for an empty list
    assert entry(sim, _ptr(b), len(b), _ptr(offsets, C.c_int64), _ptr(keep, C.c_int32), _ptr(counts, C.c_int32)) == 0
    return prims, counts


def trisim_list(hs, tris, offsets, node_format=64, leaf_size=4, fill=-7):
    """moptix_query_tris_list on the CPU, by the walk: (prims, counts); prims starts out as `fill` throughout."""
    sim = hostsim_handle(hs, leaf_size)
    L = _lib()
    return _list(lambda s, *a: L.trisim_list(s._h, int(node_format), *a), sim, _tris(tris), offsets, fill)


def tribrute_list(hs, tris, offsets, leaf_size=4, fill=-7):
    """The same from the definition, the ids sorted by the library's sort."""
    sim = hostsim_handle(hs, leaf_size)
    L = _lib()
    return _list(lambda s, *a: L.trisim_brute_list(s._h, *a), sim, _tris(tris), offsets, fill)


def tri_stack_depth(hs, tris, mode="count", node_format=64, leaf_size=4):
    """Most stack entries the walk of any of the queries holds."""
    sim = hostsim_handle(hs, leaf_size)
    b = _tris(tris)
    d = _lib().trisim_stack_depth(sim._h, int(node_format), _ptr(b), len(b), MODES[mode])
    assert d >= 0
    return d


def predicate(kind, prims, tris):
    """The mirror's predicate `kind` ("tri": 9 floats, three vertices; "sphere": centre and radius; "quad": the record's v1, v2, anchor)
    pair by pair: prims [n, 9 or 4], tris [n, 9] -> bool [n]."""
    p, b = _f32(prims), _tris(tris)
    assert len(p) == len(b)
    out = np.zeros(len(b), np.int32)
    assert getattr(_lib(), "trisim_" + kind)(_ptr(p), _ptr(b), len(b), _ptr(out, C.c_int32)) == 0
    return out != 0


class MirrorContext:
    """Context.query_tris and what Context.self_intersections asks of a context besides, answered by the mirror on a scene: the stub the
    Python-level pairing is tested behind where there is no device."""

    def __init__(self, M, hs, first_face=0):
        self.hs, self.first_face = hs, first_face
        self.self_intersections = lambda *a, **kw: M.Context.self_intersections(self, *a, **kw)

    def _first_face_id(self, n_faces):
        return self.first_face

    def query_tris(self, tris, mode="any", max_prims=None):
        t = np.asarray(tris, np.float32).reshape(-1, 9)
        if mode != "list":
            return trisim(self.hs, t, mode)
        counts = trisim(self.hs, t, "count")
        if max_prims is None:
            return trisim_list(self.hs, t, csr(counts))[0], csr(counts)
        prims, counts = trisim_list(self.hs, t, np.arange(len(t) + 1, dtype=np.int64) * int(max_prims))
        return prims.reshape(len(t), int(max_prims)), counts


# ---- the query sets ----
def tri_sets(geo, lo, hi, seed=32):
    """The query triangles of a scene as one float32 [n, 9] array (about 1,600) and the slices of its parts:
      faces     512 copies of the scene's own faces (where it has none: of small triangles on surface points): a third moved by
                diag x 10^k, k uniform in [-4, -1], a third rotated about their centroid by a uniform random rotation, a third scaled about
                their centroid by 2^k, k uniform in [-2, 2]
      own       64 of the scene's faces as they are (binary32): every one meets itself and its neighbours
      random    512 random triangles centred uniformly in the box lo .. hi enlarged by a quarter of its size on each side, and 256 on
                surface points; vertices centre + size x a standard normal, size = diag x 10^k, k uniform in [log10 0.0005, log10 0.3]
      slivers   64 triangles 100:1 on surface points
      segments  96 zero-area queries on surface points: two equal vertices (each of the three ways) or three collinear ones
      points    64 queries a = b = c: half on mesh vertices (surface points where there is no mesh), half on random surface points
      far       16 small triangles centred 1e4 scene diagonals away
      special   one triangle cutting the whole scene, then the invalid ones: a NaN, an inf and a -inf in each of three slots"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    diag = max(float(np.linalg.norm(hi - lo)), 1e-30)
    size = np.maximum(hi - lo, 1e-3 * diag)
    parts, rows = {}, []

    def add(name, block):
        first = sum(len(r) for r in rows)
        block = np.asarray(block, np.float64).reshape(-1, 9)
        rows.append(block); parts[name] = slice(first, first + len(block))

    def small(centres, k_lo=np.log10(0.0005), k_hi=np.log10(0.3)):
        n = len(centres)
        return centres[:, None, :] + (diag * 10.0 ** rng.uniform(k_lo, k_hi, (n, 1, 1))) * rng.normal(size=(n, 3, 3))

    if geo.nt:
        base = geo.tri[rng.integers(0, geo.nt, 512)]
    else:
        base = small(geo.surface_points(rng, 512), np.log10(0.01), np.log10(0.1))
    ctr = base.mean(axis=1, keepdims=True)
    moved = base[:171] + (diag * 10.0 ** rng.uniform(-4, -1, (171, 1, 1))) * random_rotations(rng, 171)[:, :1]
    rot = ctr[171:342] + np.einsum("nij,nkj->nki", random_rotations(rng, 171), base[171:342] - ctr[171:342])
    scaled = ctr[342:] + (2.0 ** rng.uniform(-2, 2, (170, 1, 1))) * (base[342:] - ctr[342:])
    add("faces", np.concatenate([moved, rot, scaled]))
    add("own", geo.tri[rng.integers(0, geo.nt, 64)] if geo.nt else base[:64])
    c = np.concatenate([rng.uniform(lo - 0.25 * size, hi + 0.25 * size, (512, 3)), geo.surface_points(rng, 256)])
    add("random", small(c))
    c = geo.surface_points(rng, 64)
    fr = random_rotations(rng, 64)
    ln = diag * 10.0 ** rng.uniform(-2.5, -0.7, (64, 1))
    add("slivers", np.stack([c - 0.5 * ln * fr[:, 0], c + 0.5 * ln * fr[:, 0], c + 0.01 * ln * fr[:, 1]], axis=1))
    c = geo.surface_points(rng, 96)
    d = (diag * 10.0 ** rng.uniform(-3, -0.7, (96, 1))) * random_rotations(rng, 96)[:, 0]
    a, b = (c - 0.5 * d).astype(np.float32).astype(np.float64), (c + 0.5 * d).astype(np.float32).astype(np.float64)
    seg = np.stack([a, b, b], axis=1)
    seg[1::4] = np.stack([a, a, b], axis=1)[1::4]
    seg[2::4] = np.stack([a, b, a], axis=1)[2::4]
    seg[3::4] = np.stack([a, a + 0.25 * (b - a), b], axis=1)[3::4]           # collinear up to the rounding of the middle vertex
    add("segments", seg)
    if geo.nt:
        pv = geo.tri.reshape(-1, 3)[rng.integers(0, 3 * geo.nt, 32)]
    else:
        pv = geo.surface_points(rng, 32)
    pv = np.concatenate([pv, geo.surface_points(rng, 32)])
    add("points", np.repeat(pv[:, None, :], 3, axis=1))
    mid = 0.5 * (lo + hi)
    add("far", small(mid + 1e4 * diag * random_rotations(rng, 16)[:, 0], -3, -1))
    whole = np.stack([mid + 4 * diag * np.array([1.0, 0.1, 0.05]), mid + 4 * diag * np.array([-1.0, 1.0, 0.0]), mid + 4 * diag * np.array([-1.0, -1.0, -0.1])])
    bad = np.repeat(whole.reshape(1, 9), 9, axis=0)
    for r, (k, v) in enumerate([(0, np.nan), (4, np.nan), (8, np.nan), (1, np.inf), (3, np.inf), (7, np.inf), (2, -np.inf), (5, -np.inf), (6, -np.inf)]):
        bad[r, k] = v
    add("special", np.concatenate([whole.reshape(1, 9), bad]))
    with np.errstate(over="ignore"):
        tris = np.ascontiguousarray(np.concatenate(rows), np.float32)
    parts["whole"] = parts["special"].start
    parts["invalid"] = slice(parts["special"].start + 1, parts["special"].stop)
    return tris, parts


def valid_tris(tris):
    return np.isfinite(np.asarray(tris, np.float32).reshape(-1, 9)).all(axis=1)


# ---- exact, on Python integers or Fractions; no axis list ----
def _sub(a, b): return (a[0] - b[0], a[1] - b[1], a[2] - b[2])
def _dot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
def _cross(a, b): return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
def _zero(a): return a[0] == 0 and a[1] == 0 and a[2] == 0
def _sgn(x): return (x > 0) - (x < 0)


def _drop(n):
    """The two coordinate indices kept when a plane of normal n is projected along its largest |component|."""
    k = max(range(3), key=lambda i: abs(n[i]))
    return [i for i in range(3) if i != k]


def _orient2(a, b, c): return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _on_seg2(a, b, x):
    return min(a[0], b[0]) <= x[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= x[1] <= max(a[1], b[1])


def _seg_seg2(p, q, r, s):
    o1, o2, o3, o4 = _orient2(p, q, r), _orient2(p, q, s), _orient2(r, s, p), _orient2(r, s, q)
    if (o1 == 0 and _on_seg2(p, q, r)) or (o2 == 0 and _on_seg2(p, q, s)) or (o3 == 0 and _on_seg2(r, s, p)) or (o4 == 0 and _on_seg2(r, s, q)):
        return True
    return _sgn(o1) * _sgn(o2) < 0 and _sgn(o3) * _sgn(o4) < 0


def _in_tri2(x, a, b, c):
    s = (_sgn(_orient2(a, b, x)), _sgn(_orient2(b, c, x)), _sgn(_orient2(c, a, x)))
    return not (min(s) < 0 and max(s) > 0)


def _point_on_seg(x, a, b):
    ab, ax = _sub(b, a), _sub(x, a)
    return _zero(_cross(ax, ab)) and 0 <= _dot(ax, ab) <= _dot(ab, ab)


def _seg_seg3(p, q, r, s):
    d1, d2, w = _sub(q, p), _sub(s, r), _sub(r, p)
    c = _cross(d1, d2)
    if not _zero(c):
        if _dot(w, c) != 0:
            return False                                    # skew lines
        i, j = _drop(c)
        return _seg_seg2((p[i], p[j]), (q[i], q[j]), (r[i], r[j]), (s[i], s[j]))
    if _zero(d1):
        return _point_on_seg(p, r, s)
    if _zero(d2):
        return _point_on_seg(r, p, q)
    if not _zero(_cross(w, d1)):
        return False                                        # parallel, apart
    t0, t1, ln = _dot(w, d1), _dot(_sub(s, p), d1), _dot(d1, d1)
    return max(min(t0, t1), 0) <= min(max(t0, t1), ln)


def _seg_tri(p, q, t, n):
    """Does the closed segment p q meet the closed triangle t (normal n, possibly zero)?"""
    a, b, c = t
    if _zero(n):                                            # the triangle is a segment or a point: its longest side is all of it
        u, v = max(((a, b), (b, c), (c, a)), key=lambda e: _dot(_sub(e[1], e[0]), _sub(e[1], e[0])))
        return _seg_seg3(p, q, u, v)
    sp, sq = _dot(n, _sub(p, a)), _dot(n, _sub(q, a))
    if _sgn(sp) * _sgn(sq) > 0:
        return False
    if sp == 0 and sq == 0:                                 # coplanar: in the plane, an end inside or a side crossed
        i, j = _drop(n)
        f = lambda x: (x[i], x[j])
        if _in_tri2(f(p), f(a), f(b), f(c)) or _in_tri2(f(q), f(a), f(b), f(c)):
            return True
        return any(_seg_seg2(f(p), f(q), f(u), f(v)) for u, v in ((a, b), (b, c), (c, a)))
    den = sp - sq                                           # the one point on the plane is x = X / den
    pq = _sub(q, p)
    big = tuple(p[k] * den + pq[k] * sp for k in range(3))
    sg = _sgn(den)
    for u, v in ((a, b), (b, c), (c, a)):
        if sg * _dot(n, _cross(_sub(v, u), tuple(big[k] - u[k] * den for k in range(3)))) < 0:
            return False
    return True


def tri_tri_exact(t1, t2):
    """Do the closed triangles t1, t2 (three points each, of Python integers or Fractions; zero area allowed) have a point in common?
    Two convex sets of dimension <= 2 that meet have a boundary point of one inside the other, so: some edge of one meets the other."""
    for k in range(3):
        if max(v[k] for v in t1) < min(v[k] for v in t2) or max(v[k] for v in t2) < min(v[k] for v in t1):
            return False
    n1 = _cross(_sub(t1[1], t1[0]), _sub(t1[2], t1[0]))
    n2 = _cross(_sub(t2[1], t2[0]), _sub(t2[2], t2[0]))
    for u, v in ((0, 1), (1, 2), (2, 0)):
        if _seg_tri(t1[u], t1[v], t2, n2) or _seg_tri(t2[u], t2[v], t1, n1):
            return True
    return False


def fractions_of(tri):
    """A [3, 3] array of binary32 or binary64 numbers as three points of exact Fractions."""
    return [tuple(Fraction(float(x)) for x in v) for v in np.asarray(tri).reshape(3, 3)]


def zero_area_exact(t):
    return _zero(_cross(_sub(t[1], t[0]), _sub(t[2], t[0])))


def largest_intermediate(q, t):
    """For pairs of integer triangles q, t [n, 3, 3] (int64, coordinates in units of 1/2): an upper bound, in units of 1/16 for the
    projections on the cross-normal axes, of the magnitude of every intermediate of pt_tri.h's step B -- differences, products, the partial
    sums of the dots and crosses -- as the largest sum of |products| any of them is made of."""
    q, t = np.asarray(q, np.int64), np.asarray(t, np.int64)
    q1, q2 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]
    u = t - q[:, :1]
    e = [q1, q2 - q1, -q2]
    f = [u[:, 1] - u[:, 0], u[:, 2] - u[:, 1], u[:, 0] - u[:, 2]]
    worst = max(int(np.abs(x).max()) for x in [q1, q2, u] + e + f)

    def cross(a, b):
        nonlocal worst
        worst = max(worst, int((np.abs(a[:, [1, 2, 0]] * b[:, [2, 0, 1]]) + np.abs(a[:, [2, 0, 1]] * b[:, [1, 2, 0]])).max()))
        return np.cross(a, b)
    n1, n2 = cross(e[0], e[1]), cross(f[0], f[1])
    axes = [n1, n2] + [cross(e[i], f[j]) for i in range(3) for j in range(3)]
    axes += [cross(n1, x) for x in e] + [cross(n1, x) for x in f] + [cross(n2, x) for x in e] + [cross(n2, x) for x in f]
    for ax in axes:
        for w in (q1, q2, u[:, 0], u[:, 1], u[:, 2]):
            worst = max(worst, int(np.abs(ax * w).sum(axis=1).max()))
    return worst


# ---- binary64, numpy: the distance between two triangles and the penetration over the axis list ----
def _seg_seg_dist64(p1, q1, p2, q2):
    """Distance between the segments p1 q1 and p2 q2, pairwise [n] (Ericson 5.1.9, the degenerate cases by masks)."""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, f = (d1 * d1).sum(axis=1), (d2 * d2).sum(axis=1), (d2 * r).sum(axis=1)
    c, b = (d1 * r).sum(axis=1), (d1 * d2).sum(axis=1)
    den = a * e - b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(den > 0, np.clip((b * f - c * e) / np.where(den > 0, den, 1.0), 0.0, 1.0), 0.0)
        s = np.where(a > 0, s, 0.0)
        t = np.where(e > 0, (b * s + f) / np.where(e > 0, e, 1.0), 0.0)
        s = np.where(t < 0, np.where(a > 0, np.clip(-c / np.where(a > 0, a, 1.0), 0.0, 1.0), 0.0),
                     np.where(t > 1, np.where(a > 0, np.clip((b - c) / np.where(a > 0, a, 1.0), 0.0, 1.0), 0.0), s))
        t = np.clip(t, 0.0, 1.0)
    return np.linalg.norm((p1 + d1 * s[:, None]) - (p2 + d2 * t[:, None]), axis=1)


def _pierces64(p, q, t):
    """Does the segment p q cross the plane of triangle t [n, 3, 3] at a point inside it?  bool [n]; zero-area triangles: False."""
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    n = np.cross(b - a, c - a)
    sp, sq = ((p - a) * n).sum(axis=1), ((q - a) * n).sum(axis=1)
    den = sp - sq
    ok = (sp * sq <= 0) & (den != 0)
    x = p + (sp / np.where(ok, den, 1.0))[:, None] * (q - p)
    side = lambda u, v: (np.cross(v - u, x - u) * n).sum(axis=1)
    return ok & (side(a, b) >= 0) & (side(b, c) >= 0) & (side(c, a) >= 0)


def tri_tri_dist64(t1, t2):
    """The distance between triangles t1 and t2 [n, 3, 3], pairwise, binary64: 0 where an edge of one pierces the other, else the least
    of the nine edge-edge and six vertex-triangle distances."""
    t1, t2 = np.asarray(t1, np.float64), np.asarray(t2, np.float64)
    best = np.full(len(t1), np.inf)
    hit = np.zeros(len(t1), bool)
    for i in range(3):
        best = np.minimum(best, tri_dist64(t1[:, i], t2)[0])
        best = np.minimum(best, tri_dist64(t2[:, i], t1)[0])
        hit |= _pierces64(t1[:, i], t1[:, (i + 1) % 3], t2) | _pierces64(t2[:, i], t2[:, (i + 1) % 3], t1)
        for j in range(3):
            best = np.minimum(best, _seg_seg_dist64(t1[:, i], t1[:, (i + 1) % 3], t2[:, j], t2[:, (j + 1) % 3]))
    return np.where(hit, 0.0, best)


def penetration64(q, t):
    """The least overlap of the two projections, per unit length of the axis, over the 23 axes of the list (those of zero length left
    out), for queries q and triangles t [n, 3, 3] pairwise in the frame at q's first vertex, binary64: negative where an axis separates
    the pair.  +inf where every axis is zero."""
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    a = q[:, :1]
    qs, u = q - a, t - a
    e = [qs[:, 1] - qs[:, 0], qs[:, 2] - qs[:, 1], qs[:, 0] - qs[:, 2]]
    f = [u[:, 1] - u[:, 0], u[:, 2] - u[:, 1], u[:, 0] - u[:, 2]]
    n1, n2 = np.cross(e[0], e[1]), np.cross(f[0], f[1])
    axes = [n1, n2] + [np.cross(e[i], f[j]) for i in range(3) for j in range(3)]
    axes += [np.cross(n1, x) for x in e] + [np.cross(n1, x) for x in f] + [np.cross(n2, x) for x in e] + [np.cross(n2, x) for x in f]
    pen = np.full(len(q), np.inf)
    for ax in axes:
        ln = np.linalg.norm(ax, axis=1)
        ok = ln > 0
        ax = ax / np.where(ok, ln, 1.0)[:, None]
        s = (qs * ax[:, None, :]).sum(axis=2)
        w = (u * ax[:, None, :]).sum(axis=2)
        over = np.minimum(s.max(axis=1), w.max(axis=1)) - np.maximum(s.min(axis=1), w.min(axis=1))
        pen = np.where(ok, np.minimum(pen, over), pen)
    return pen


def pair_scale(q, t):
    """The pair's scale: its largest |coordinate| plus its largest extent."""
    both = np.concatenate([np.asarray(q, np.float64), np.asarray(t, np.float64)], axis=1)
    return np.abs(both).max(axis=(1, 2)) + (both.max(axis=1) - both.min(axis=1)).max(axis=1)


def zero_area64(t):
    t = np.asarray(t, np.float64)
    return (np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]) == 0).all(axis=1)


def quad_triangles(geo, i):
    """The two triangles [2, 3, 3] of quad i, from the corners anchor + a1 E1 + a2 E2."""
    k = [geo.anchor[i] + a1 * geo.E1[i] + a2 * geo.E2[i] for a1, a2 in ((0, 0), (1, 0), (1, 1), (0, 1))]
    return np.array([[k[0], k[1], k[2]], [k[0], k[2], k[3]]])


# ---- a self-intersecting mesh ----
def mesh_hs(v, f):
    """The mesh (vertices [V, 3], faces [F, 3]) alone as a scene, sign_helpers.mesh_scene's way."""
    from common import M, MovedScene
    from sign_helpers import _mesh_only
    fp = np.asarray(v, np.float32)[np.asarray(f).reshape(-1)].reshape(len(f), 9)
    return _mesh_only(MovedScene(M.HostScene("file:coffee", 64, 36), fp, new_faces=True))


def pushed_torus(amount=1.8):
    """sign_helpers.torus with one vertex of the outer equator pushed through the hole and the opposite wall: (vertices float32 [V, 3],
    faces int64 [F, 3])."""
    from sign_helpers import torus
    v, f = torus()
    v = v.astype(np.float32)
    k = int(np.argmax(v[:, 0] - 10 * np.abs(v[:, 1]) - 10 * np.abs(v[:, 2])))       # (1.4, 0, 0)
    v[k, 0] -= np.float32(amount)
    return v, f
