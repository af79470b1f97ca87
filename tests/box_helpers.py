"""The box overlap queries of the CPU mirror (tests/boxsim/boxsim.cpp, a library of its own beside libhostsim.so): the walk through the
kernel's per-box code and the definition itself as a loop over every primitive record; the box sets the box tests share; and two
references that share no code with the mirror -- an exact rational evaluation of the predicates (fractions.Fraction) and a binary64
separating-axis gap from the scene's original vertices (numpy)."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np

from common import REPO, _f32, _ptr, hostsim_handle, hostsim_lib
from point_helpers import Geometry      # noqa: F401  (for the tests)
from query_helpers import same_bits     # noqa: F401  (for the tests)

BOX_ANY, BOX_COUNT = 0, 1                                 # MOPTIX_BOX_ANY / MOPTIX_BOX_COUNT, spelled out here apart from the package's definition
MODES = dict(any=BOX_ANY, count=BOX_COUNT)

_DIR = os.path.join(REPO, "tests", "boxsim")
_boxsim = None


def _lib():
    """tests/boxsim/libboxsim.so (built here if it is missing, as common.hostsim_lib builds its library) with the signatures of its
    entries.  They take the handles of common.HostsimHandle."""
    global _boxsim
    if _boxsim is None:
        hostsim_lib()
        path = os.path.join(_DIR, "libboxsim.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _DIR, "-s"])
        L = C.CDLL(path)
        vp, f32p, i32p, i64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        L.boxsim_query.argtypes, L.boxsim_query.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int, i32p], C.c_int
        L.boxsim_list.argtypes, L.boxsim_list.restype = [vp, C.c_int, f32p, C.c_int64, i64p, i32p, i32p], C.c_int
        L.boxsim_brute.argtypes, L.boxsim_brute.restype = [vp, f32p, C.c_int64, C.c_int, i32p], C.c_int
        L.boxsim_brute_list.argtypes, L.boxsim_brute_list.restype = [vp, f32p, C.c_int64, i64p, i32p, i32p], C.c_int
        L.boxsim_stack_depth.argtypes, L.boxsim_stack_depth.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int], C.c_int
        for name in ("boxsim_tri", "boxsim_sphere", "boxsim_quad"):
            getattr(L, name).argtypes, getattr(L, name).restype = [f32p, f32p, C.c_int64, i32p], C.c_int
        _boxsim = L
    return _boxsim


def _boxes(boxes):
    return _f32(np.asarray(boxes, np.float32).reshape(-1, 6))


def boxsim(hs, boxes, mode="any", node_format=64, leaf_size=4):
    """moptix_query_boxes on the CPU, by the walk: int32 per box.  hs: a scene, or a built one."""
    sim = hostsim_handle(hs, leaf_size)
    b = _boxes(boxes)
    out = np.zeros(len(b), np.int32)
    assert _lib().boxsim_query(sim._h, int(node_format), _ptr(b), len(b), MODES[mode], _ptr(out, C.c_int32)) == 0
    return out


def boxbrute(hs, boxes, mode="any", leaf_size=4):
    """The same from the definition: every primitive record through its predicate, no tree."""
    sim = hostsim_handle(hs, leaf_size)
    b = _boxes(boxes)
    out = np.zeros(len(b), np.int32)
    assert _lib().boxsim_brute(sim._h, _ptr(b), len(b), MODES[mode], _ptr(out, C.c_int32)) == 0
    return out


def _list(entry, sim, b, offsets, fill):
    offsets = np.ascontiguousarray(offsets, np.int64)
    prims = np.full(int(offsets[-1]) if len(offsets) else 0, fill, np.int32)
    counts = np.zeros(len(b), np.int32)
    keep = np.zeros(1, np.int32) if len(prims) == 0 else prims      # a valid address for an empty list
    assert entry(sim, _ptr(b), len(b), _ptr(offsets, C.c_int64), _ptr(keep, C.c_int32), _ptr(counts, C.c_int32)) == 0
    return prims, counts


def boxsim_list(hs, boxes, offsets, node_format=64, leaf_size=4, fill=-7):
    """moptix_query_boxes_list on the CPU, by the walk: (prims, counts); prims starts out as `fill` throughout."""
    sim = hostsim_handle(hs, leaf_size)
    L = _lib()
    return _list(lambda s, *a: L.boxsim_list(s._h, int(node_format), *a), sim, _boxes(boxes), offsets, fill)


def boxbrute_list(hs, boxes, offsets, leaf_size=4, fill=-7):
    """The same from the definition, the ids sorted by the library's sort."""
    sim = hostsim_handle(hs, leaf_size)
    L = _lib()
    return _list(lambda s, *a: L.boxsim_brute_list(s._h, *a), sim, _boxes(boxes), offsets, fill)


def csr(counts):
    """The offsets of exact capacities."""
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, dtype=np.int64, out=off[1:])
    return off


def box_stack_depth(hs, boxes, mode="count", node_format=64, leaf_size=4):
    """Most stack entries the walk of any of the boxes holds."""
    sim = hostsim_handle(hs, leaf_size)
    b = _boxes(boxes)
    d = _lib().boxsim_stack_depth(sim._h, int(node_format), _ptr(b), len(b), MODES[mode])
    assert d >= 0
    return d


def predicate(kind, prims, boxes):
    """The mirror's predicate `kind` ("tri": 9 floats, three vertices; "sphere": centre and radius; "quad": the record's v1, v2, anchor)
    pair by pair: prims [n, 9 or 4], boxes [n, 6] -> bool [n]."""
    p, b = _f32(prims), _boxes(boxes)
    assert len(p) == len(b)
    out = np.zeros(len(b), np.int32)
    assert getattr(_lib(), "boxsim_" + kind)(_ptr(p), _ptr(b), len(b), _ptr(out, C.c_int32)) == 0
    return out != 0


# ---- the box sets ----
def scene_extent(geo):
    """lo, hi over every primitive of a Geometry: triangles, spheres with their radii, quad corners."""
    pts = [geo.tri.reshape(-1, 3)] if geo.nt else []
    if geo.ns:
        pts += [geo.centre - geo.radius[:, None], geo.centre + geo.radius[:, None]]
    for k in range(geo.nq):
        pts.append(np.array([geo.anchor[k] + a * geo.E1[k] + b * geo.E2[k] for a in (0, 1) for b in (0, 1)]))
    p = np.concatenate(pts)
    return p.min(axis=0), p.max(axis=0)


def box_sets(geo, lo, hi, seed=17):
    """The boxes of a scene as one float32 [n, 6] array and the slices of its parts:
      uniform  1,024 boxes centred uniformly in the box lo .. hi enlarged by half its size on each side, half-sizes diag x 10^k per axis,
               k uniform in [-3, -0.5]
      surface  512 boxes centred on random surface points, half-sizes diag x 10^k per axis, k uniform in [-6, -1]
      special  of every 37th triangle: its exact vertex box; lo == hi == its first vertex; a box over the triangle's y, z extent whose hi.x
               is the triangle's least x exactly, and the same box with hi.x one ulp lower; then the box of every primitive (a little
               enlarged), an inverted box, a box with a NaN and one with an inf."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    diag = max(float(np.linalg.norm(hi - lo)), 1e-30)
    size = np.maximum(hi - lo, 1e-3 * diag)
    c = rng.uniform(lo - 0.5 * size, hi + 0.5 * size, (1024, 3))
    h = diag * 10.0 ** rng.uniform(-3.0, -0.5, (1024, 3))
    uni = np.concatenate([c - h, c + h], axis=1)
    c = geo.surface_points(rng, 512)
    h = diag * 10.0 ** rng.uniform(-6.0, -1.0, (512, 3))
    surf = np.concatenate([c - h, c + h], axis=1)
    t = geo.tri[::37].astype(np.float32)
    special = []
    if len(t):
        tlo, thi = t.min(axis=1), t.max(axis=1)
        touch = np.concatenate([tlo, thi], axis=1)
        touch[:, 0] = tlo[:, 0] - np.float32(0.25 * diag)
        touch[:, 3] = tlo[:, 0]
        below = touch.copy()
        below[:, 3] = np.nextafter(tlo[:, 0], np.float32(-np.inf))
        special += [np.concatenate([tlo, thi], axis=1), np.concatenate([t[:, 0], t[:, 0]], axis=1), touch, below]
    alo, ahi = scene_extent(geo)
    pad = 0.01 * max(float(np.linalg.norm(ahi - alo)), 1e-30)
    whole = np.concatenate([alo - pad, ahi + pad])
    inverted = whole.copy(); inverted[0], inverted[3] = whole[3], whole[0]
    nan = whole.copy(); nan[4] = np.nan
    inf = whole.copy(); inf[5] = np.inf
    special.append(np.array([whole, inverted, nan, inf]))
    special = np.concatenate(special)
    boxes = np.ascontiguousarray(np.concatenate([uni, surf, special]), np.float32)
    # rounding to binary32 may invert a box thinner than an ulp: such a box is made a valid degenerate one (lo == hi on that axis)
    fix = slice(0, 1536)
    flipped = boxes[fix, :3] > boxes[fix, 3:]
    boxes[fix, 3:] = np.where(flipped, boxes[fix, :3], boxes[fix, 3:])
    n = len(boxes)
    parts = dict(uniform=slice(0, 1024), surface=slice(1024, 1536), special=slice(1536, n), whole=n - 4, inverted=n - 3, nan=n - 2, inf=n - 1)
    return boxes, parts


def valid_boxes(boxes):
    b = np.asarray(boxes, np.float32).reshape(-1, 6)
    return np.isfinite(b).all(axis=1) & (b[:, :3] <= b[:, 3:]).all(axis=1)


# ---- reference 1: exact rational evaluation (every input a binary32 value, so Fraction holds it exactly) ----
def _integers(values):
    """The binary32 values as exact rationals over their common denominator (a power of two), times 2: their numerators, Python integers.
    Both predicates compare homogeneous expressions of the coordinates, so the common factor changes no verdict; the 2 keeps the box's
    centre and half-size integers too."""
    fr = [Fraction(float(x)) for x in values]
    den = max(f.denominator for f in fr)
    return [int(f * den) * 2 for f in fr]


def tri_box_exact(tri, box):
    """(overlap, touching) of the closed triangle tri [3, 3] and the closed box [6] by the 13-axis separating-axis theorem in exact rational
    arithmetic.  touching: they overlap and the largest separation over the axes of non-zero length is exactly 0."""
    z = _integers(list(np.asarray(tri).reshape(-1)) + list(box))
    v, lo, hi = [z[0:3], z[3:6], z[6:9]], z[9:12], z[12:15]
    c = [(lo[k] + hi[k]) // 2 for k in range(3)]
    h = [(hi[k] - lo[k]) // 2 for k in range(3)]
    u = [[p[k] - c[k] for k in range(3)] for p in v]
    f = [[u[(j + 1) % 3][k] - u[j][k] for k in range(3)] for j in range(3)]
    n = [f[0][1] * f[1][2] - f[0][2] * f[1][1], f[0][2] * f[1][0] - f[0][0] * f[1][2], f[0][0] * f[1][1] - f[0][1] * f[1][0]]
    axes = [[int(k == a) for k in range(3)] for a in range(3)]
    for e in range(3):
        for fj in f:
            ex = axes[e]
            axes.append([ex[1] * fj[2] - ex[2] * fj[1], ex[2] * fj[0] - ex[0] * fj[2], ex[0] * fj[1] - ex[1] * fj[0]])
    axes.append(n)
    worst = None
    for a in axes:
        if not any(a):
            continue
        p = [sum(a[k] * q[k] for k in range(3)) for q in u]
        r = sum(h[k] * abs(a[k]) for k in range(3))
        s = max(min(p) - r, -max(p) - r)      # > 0: this axis separates; the sign does not depend on the axis' length
        worst = s if worst is None or s > worst else worst
    return worst <= 0, worst == 0


def sphere_box_exact(sphere, box):
    """(overlap, touching) of the sphere surface (centre, radius) [4] and the closed box [6], exactly: the distances from the centre to the
    box range over [dmin, dmax], and the surface meets the box iff dmin <= radius <= dmax."""
    z = _integers(list(sphere) + list(box))
    c, r, lo, hi = z[0:3], z[3], z[4:7], z[7:10]
    dmin2 = sum(max(lo[k] - c[k], c[k] - hi[k], 0) ** 2 for k in range(3))
    dmax2 = sum(max(abs(c[k] - lo[k]), abs(hi[k] - c[k])) ** 2 for k in range(3))
    over = dmin2 <= r * r <= dmax2
    return over, over and (dmin2 == r * r or dmax2 == r * r)


# ---- reference 2: the binary64 gap (numpy), every box against every primitive ----
def tri_gap64(tri, boxes):
    """The largest of the 13 axes' normalised separations of every box [nb, 6] against every triangle [nt, 3, 3], in binary64: [nb, nt];
    <= 0 where they overlap.  Axes of zero length are skipped."""
    tri, boxes = np.asarray(tri, np.float64), np.asarray(boxes, np.float64)
    c, h = 0.5 * (boxes[:, :3] + boxes[:, 3:]), 0.5 * (boxes[:, 3:] - boxes[:, :3])
    u = tri[None, :, :, :] - c[:, None, None, :]                             # [nb, nt, 3 vertices, 3]
    f = np.roll(tri, -1, axis=1) - tri                                       # [nt, 3 edges, 3]
    eye = np.eye(3)
    axes = [np.broadcast_to(eye[a], (len(tri), 3)) for a in range(3)]
    axes += [np.cross(eye[e], f[:, j]) for e in range(3) for j in range(3)]
    axes.append(np.cross(f[:, 0], f[:, 1]))
    gap = np.full((len(boxes), len(tri)), -np.inf)
    for a in axes:
        ln = np.linalg.norm(a, axis=1)
        ok = ln > 0
        a = a / np.where(ok, ln, 1.0)[:, None]
        p = (u * a[None, :, None, :]).sum(axis=3)                            # [nb, nt, 3]
        r = (h[:, None, :] * np.abs(a)[None, :, :]).sum(axis=2)
        s = np.maximum(p.min(axis=2) - r, -p.max(axis=2) - r)
        gap = np.where(ok[None, :], np.maximum(gap, s), gap)
    return gap


def all_pairs_gap64(geo, boxes):
    """(gap [nb, ns + nq + nt], scale [nb, ns + nq + nt], usable [ns + nq + nt]) in the queries' numbering: gap <= 0 where box and
    primitive overlap (sphere: max(dmin - r, r - dmax); quad: the lesser of its two triangles' gaps), scale the largest |coordinate| of
    the pair, usable False for zero-area triangles."""
    b = np.asarray(boxes, np.float64)
    nb = len(b)
    cols, scales = [], []
    for i in range(geo.ns):
        c, r = geo.centre[i], geo.radius[i]
        dmin = np.linalg.norm(np.maximum(np.maximum(b[:, :3] - c, c - b[:, 3:]), 0.0), axis=1)
        dmax = np.linalg.norm(np.maximum(np.abs(c - b[:, :3]), np.abs(b[:, 3:] - c)), axis=1)
        cols.append(np.maximum(dmin - r, r - dmax)); scales.append(np.full(nb, np.abs(c).max() + r))
    for i in range(geo.nq):
        k = [geo.anchor[i] + a1 * geo.E1[i] + a2 * geo.E2[i] for a1, a2 in ((0, 0), (1, 0), (1, 1), (0, 1))]
        g = tri_gap64(np.array([[k[0], k[1], k[2]], [k[0], k[2], k[3]]]), b)
        cols.append(g.min(axis=1)); scales.append(np.full(nb, np.abs(np.array(k)).max()))
    gap = np.zeros((nb, geo.ns + geo.nq + geo.nt))
    scale = np.zeros_like(gap)
    if cols:
        gap[:, :geo.ns + geo.nq] = np.stack(cols, axis=1); scale[:, :geo.ns + geo.nq] = np.stack(scales, axis=1)
    usable = np.ones(gap.shape[1], bool)
    if geo.nt:
        first = geo.ns + geo.nq
        gap[:, first:] = tri_gap64(geo.tri, b)
        scale[:, first:] = np.abs(geo.tri).max(axis=(1, 2))[None, :]
        usable[first:] = np.linalg.norm(np.cross(geo.tri[:, 1] - geo.tri[:, 0], geo.tri[:, 2] - geo.tri[:, 0]), axis=1) > 0
    scale = np.maximum(scale, np.abs(b).max(axis=1)[:, None])
    return gap, scale, usable


def membership(prims, offsets, n_prims):
    """A CSR list as a bool matrix [n boxes, n_prims]."""
    m = np.zeros((len(offsets) - 1, n_prims), bool)
    rows = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    m[rows, prims] = True
    return m
