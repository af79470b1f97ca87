"""The sphere sweep queries of the CPU mirror (tests/sweepsim/sweepsim.cpp, a library of its own beside libhostsim.so): the walk through
the kernel's per-sweep code, the definition itself as a loop over every primitive record, and the per-primitive time of contact on
explicit inputs; the sweep sets the sweep tests share; and a binary64 first contact (numpy) that shares no code with the mirror."""
import ctypes as C
import os
import subprocess

import numpy as np

from box_helpers import scene_extent
from common import M, REPO, _f32, _ptr, hostsim_handle, hostsim_lib
from point_helpers import Geometry, point_case, sphere_dist64, tri_dist64      # noqa: F401  (Geometry: for the tests)
from query_helpers import same_bits     # noqa: F401  (for the tests)

SWEEP_DTYPE = np.dtype([("t", np.float32), ("prim", np.int32), ("mat", np.int32), ("u", np.float32), ("v", np.float32), ("p", np.float32, (3,))])
SWEEP_CLOSEST, SWEEP_ANY = 0, 1                           # MOPTIX_SWEEP_*, spelled out here apart from the package's definition
MODES = dict(closest=SWEEP_CLOSEST, any=SWEEP_ANY)
KINDS = dict(tri=0, sphere=1, quad=2)

_DIR = os.path.join(REPO, "tests", "sweepsim")
_sweepsim = None


def _lib():
    """tests/sweepsim/libsweepsim.so (built here if it is missing, as common.hostsim_lib builds its library) with the signatures of its
    entries.  They take the handles of common.HostsimHandle."""
    global _sweepsim
    if _sweepsim is None:
        hostsim_lib()
        path = os.path.join(_DIR, "libsweepsim.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _DIR, "-s"])
        L = C.CDLL(path)
        vp, f32p = C.c_void_p, C.POINTER(C.c_float)
        L.sweepsim_query.argtypes, L.sweepsim_query.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int, vp], C.c_int
        L.sweepsim_brute.argtypes, L.sweepsim_brute.restype = [vp, f32p, C.c_int64, C.c_int, vp], C.c_int
        L.sweepsim_stack_depth.argtypes, L.sweepsim_stack_depth.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int], C.c_int
        L.sweepsim_toi.argtypes, L.sweepsim_toi.restype = [C.c_int, f32p, f32p, C.c_int64, vp], C.c_int
        _sweepsim = L
    return _sweepsim


def _sweeps(sweeps):
    return _f32(np.asarray(sweeps, np.float32).reshape(-1, 8))


def _out(n, mode):
    return np.zeros(n, SWEEP_DTYPE if mode == "closest" else np.int32)


def sweepsim(hs, sweeps, mode="closest", node_format=64, leaf_size=4):
    """moptix_query_sweeps on the CPU, by the walk: a SWEEP_DTYPE record array ("closest") or an int32 array ("any").  hs: a scene, or a
    built one."""
    sim = hostsim_handle(hs, leaf_size)
    s = _sweeps(sweeps)
    out = _out(len(s), mode)
    assert _lib().sweepsim_query(sim._h, int(node_format), _ptr(s), len(s), MODES[mode], out.ctypes.data) == 0
    return out


def sweepbrute(hs, sweeps, mode="closest", leaf_size=4):
    """The same from the definition: every primitive record through its time of contact, no tree."""
    sim = hostsim_handle(hs, leaf_size)
    s = _sweeps(sweeps)
    out = _out(len(s), mode)
    assert _lib().sweepsim_brute(sim._h, _ptr(s), len(s), MODES[mode], out.ctypes.data) == 0
    return out


def sweep_stack_depth(hs, sweeps, mode="closest", node_format=64, leaf_size=4):
    """Most stack entries the walk of any of the sweeps holds."""
    sim = hostsim_handle(hs, leaf_size)
    s = _sweeps(sweeps)
    d = _lib().sweepsim_stack_depth(sim._h, int(node_format), _ptr(s), len(s), MODES[mode])
    assert d >= 0
    return d


def sweep_toi(kind, prims, sweeps):
    """The mirror's time of contact of `kind` ("tri": 9 floats, the record's p0, e0 = p1 - p0, e1 = p0 - p2; "sphere": centre and radius;
    "quad": the record's v1, v2, anchor) pair by pair: a SWEEP_DTYPE array with prim 0 where there is a contact in [0, tmax], else the
    miss record."""
    p, s = _f32(np.asarray(prims, np.float32).reshape(len(sweeps), -1)), _sweeps(sweeps)
    assert len(p) == len(s)
    out = np.zeros(len(s), SWEEP_DTYPE)
    assert _lib().sweepsim_toi(KINDS[kind], _ptr(p), _ptr(s), len(s), out.ctypes.data) == 0
    return out


def tri_records(tri):
    """Triangles [n, 3, 3] as the device records hold them: p0, e0 = p1 - p0, e1 = p0 - p2, in binary32 (pt_refit.h)."""
    t = np.asarray(tri, np.float32).reshape(-1, 3, 3)
    return np.ascontiguousarray(np.concatenate([t[:, 0], t[:, 1] - t[:, 0], t[:, 0] - t[:, 2]], axis=1), np.float32)


def centre32(sweeps, t):
    """c(t) = o + d * t as the definition computes it: one binary32 product and one sum per component."""
    s = np.asarray(sweeps, np.float32)
    return (s[:, 0:3] + (s[:, 3:6] * np.asarray(t, np.float32)[:, None]).astype(np.float32)).astype(np.float32)


def make_sweeps(o, d, radius, tmax):
    n = len(o)
    col = lambda x: np.broadcast_to(np.asarray(x, np.float64).reshape(-1, 1) if np.ndim(x) else np.float64(x), (n, 1))
    return np.ascontiguousarray(np.concatenate([np.asarray(o, np.float64), np.asarray(d, np.float64), col(radius), col(tmax)], axis=1), np.float32)


# ---- the sweep sets ----
def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _features(geo, rng, n):
    """n points at which a contact is a vertex or an edge contact (alternating): vertices and edge midpoints of random triangles; of the
    quads' corners and edges where there is no mesh; random surface points of the spheres where there is neither."""
    if geo.nt:
        t = geo.tri[rng.integers(0, geo.nt, n)]
    elif geo.nq:
        i = rng.integers(0, geo.nq, n)
        c = [geo.anchor[i] + a * geo.E1[i] + b * geo.E2[i] for a, b in ((0, 0), (1, 0), (1, 1))]
        t = np.stack(c, axis=1)
    else:
        return geo.surface_points(rng, n)
    k = rng.integers(0, 3, n)
    a, b = t[np.arange(n), k], t[np.arange(n), (k + 1) % 3]
    return np.where((np.arange(n) % 2 == 0)[:, None], a, 0.5 * (a + b))


def _parallel(geo, rng, n, diag, radius):
    """n sweeps that pass a face (a sphere where there is none) tangentially, at radius x (1 -+ 1e-3): alternately just inside (a contact
    with that primitive) and just outside (none with it).  (o, d) with |d| = 1."""
    off = radius * np.where(np.arange(n) % 2 == 0, 1.0 - 1e-3, 1.0 + 1e-3)
    if geo.nt or geo.nq:
        if geo.nt:
            t = geo.tri
            area = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
            t = t[area > 0][rng.integers(0, int((area > 0).sum()), n)]
        else:
            i = rng.integers(0, geo.nq, n)
            t = np.stack([geo.anchor[i], geo.anchor[i] + geo.E1[i], geo.anchor[i] + geo.E1[i] + geo.E2[i]], axis=1)
        nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        e = t[:, 1] - t[:, 0]
        size = np.linalg.norm(e, axis=1, keepdims=True)
        e = e / size
        g = t.mean(axis=1)
        return g + nrm * off[:, None] - e * (2.0 * size + 2.0 * radius[:, None] + 0.01 * diag), e
    i = rng.integers(0, geo.ns, n)
    nrm = _unit(rng, n)
    e = np.cross(nrm, _unit(rng, n)); e /= np.linalg.norm(e, axis=1, keepdims=True)
    R = geo.radius[i][:, None]
    return geo.centre[i] + nrm * (R + off[:, None]) - e * (2.0 * R + 2.0 * radius[:, None]), e


def invalid_sweeps(base):
    """Sweeps that are misses by definition, one defect each, on top of the valid sweep `base`."""
    base = np.asarray(base, np.float32)
    rows = []
    for k in range(8):
        for bad in (np.nan, np.inf, -np.inf):
            r = base.copy(); r[k] = bad; rows.append(r)
    r = base.copy(); r[3:6] = 0.0; rows.append(r)
    r = base.copy(); r[3:6] = -0.0; rows.append(r)
    for k in (6, 7):
        for bad in (0.0, -0.0, -1.0):
            r = base.copy(); r[k] = bad; rows.append(r)
    return np.ascontiguousarray(np.array(rows, np.float32))


def base_sweeps(geo, lo, hi, seed=23):
    """The sweeps of a scene before their tmax variants, float32 [n, 8], and the slices of the parts:
      uniform   768: origins uniform in the box lo .. hi, uniform directions with |d| log-uniform in [0.25, 4], radii log-uniform from
                0.1 % to 10 % of the box diagonal, a path length uniform in 0.1 .. 2 diagonals
      touching  256: origins within radius of a random surface point
      aimed     512: the centre line passes through a vertex or an edge midpoint (_features) from 0.2 .. 1 diagonals away
      parallel  256: tangential passes of a face at radius x (1 -+ 1e-3) (_parallel)
      invalid   one defect each (invalid_sweeps)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    diag = max(float(np.linalg.norm(hi - lo)), 1e-30)

    def speed(n):
        return 2.0 ** rng.uniform(-2.0, 2.0, (n, 1))

    def radii(n):
        return diag * 10.0 ** rng.uniform(-3.0, -1.0, n)
    parts, rows, first = {}, [], 0

    def add(name, s):
        nonlocal first
        parts[name] = slice(first, first + len(s)); first += len(s); rows.append(s)
    n = 768
    v = speed(n)
    add("uniform", make_sweeps(rng.uniform(lo, hi, (n, 3)), _unit(rng, n) * v, radii(n), diag * rng.uniform(0.1, 2.0, (n, 1)) / v))
    n = 256
    r, v = radii(n), speed(n)
    add("touching", make_sweeps(geo.surface_points(rng, n) + _unit(rng, n) * (r * rng.uniform(0.0, 0.999, n))[:, None], _unit(rng, n) * v, r, diag / v))
    n = 512
    r, v = radii(n), speed(n)
    f, back, far = _features(geo, rng, n), _unit(rng, n), diag * rng.uniform(0.2, 1.0, (n, 1))
    add("aimed", make_sweeps(f + back * far, -back * v, r, 2.0 * far / v))
    n = 256
    r, v = radii(n), speed(n)
    o, e = _parallel(geo, rng, n, diag, r)
    add("parallel", make_sweeps(o, e * v, r, 2.0 * diag / v))
    add("invalid", invalid_sweeps(rows[0][0]))
    return np.ascontiguousarray(np.concatenate(rows), np.float32), parts


def with_tmax_variants(base, t, prim):
    """[base; base with tmax = 0.5 t; base with tmax = 2 t], the variants of the rows that hit at t > 0 only."""
    hit = (prim >= 0) & (t > 0)
    half, twice = base[hit].copy(), base[hit].copy()
    half[:, 7] = (np.float32(0.5) * t[hit]).astype(np.float32)
    twice[:, 7] = (np.float32(2.0) * t[hit]).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([base, half, twice]), np.float32)


def valid_sweeps(sweeps):
    s = np.asarray(sweeps, np.float32).reshape(-1, 8)
    return np.isfinite(s).all(axis=1) & (s[:, 3:6] != 0).any(axis=1) & (s[:, 6] > 0) & (s[:, 7] > 0)


def contact_class(geo, hits, tol=1e-6):
    """Where the contact point of each hit lies on its primitive: 0 face interior, 1 edge, 2 vertex, -1 a miss or a sphere (which has
    neither).  From the record's u, v: a triangle's barycentrics (edges u = 0, v = 0, u + v = 1), a quad's coordinates (edges at 0 and 1)."""
    u, v, prim = hits["u"].astype(np.float64), hits["v"].astype(np.float64), hits["prim"]
    tri = prim >= geo.ns + geo.nq
    quad = (prim >= geo.ns) & ~tri
    on = np.where(tri, (u <= tol).astype(int) + (v <= tol).astype(int) + (np.abs(1.0 - u - v) <= tol).astype(int),
                  ((u <= tol) | (u >= 1 - tol)).astype(int) + ((v <= tol) | (v >= 1 - tol)).astype(int))
    return np.where(tri | quad, np.minimum(on, 2), -1)


class SweepCase:
    """A scene of the point tests (point_helpers.point_case: the scene, its geometry, its box, its leaf-4 mirror handle) with its sweep set
    -- base_sweeps and their tmax variants from the leaf-4 walk of the 64-byte nodes -- and that walk's answers, computed once and only
    read afterwards."""

    def __init__(self, name):
        self.name = name
        self.pc = point_case(name)
        self.geo = self.pc.geo
        base, self.parts = base_sweeps(self.geo, self.pc.lo, self.pc.hi)
        w = sweepsim(self.pc.sim, base)
        self.sweeps = with_tmax_variants(base, w["t"], w["prim"])
        self.n_base = len(base)
        self.hits = sweepsim(self.pc.sim, self.sweeps)
        self.anyone = sweepsim(self.pc.sim, self.sweeps, "any")
        alo, ahi = scene_extent(self.geo)
        self.S = float((ahi - alo).max())                 # the scene's largest extent, every primitive counted

    def check_classes(self):
        """Every class the set is for occurs in it: hits, misses, t == 0 starts, and -- where the scene has triangles or quads, the
        primitives that have them -- contacts on a face interior, on an edge and at a vertex."""
        h, ok = self.hits, valid_sweeps(self.sweeps)
        assert (h["prim"][ok] >= 0).sum() > 100 and (h["prim"][ok] < 0).sum() > 100, self.name
        assert ((h["prim"] >= 0) & (h["t"] == 0)).sum() > 100, self.name
        assert (h["prim"][~ok] == -1).all() and (~ok).sum() >= 30
        half = slice(self.n_base, self.n_base + (len(self.sweeps) - self.n_base) // 2)
        assert (h["prim"][half] < 0).sum() > 100, self.name                      # tmax = 0.5 t ends before the contact
        if self.geo.nt or self.geo.nq:
            k = contact_class(self.geo, h)[(h["prim"] >= 0) & (h["t"] > 0)]
            assert (k == 0).sum() > 20 and (k == 1).sum() > 20 and (k == 2).sum() > 20, (self.name, [(k == c).sum() for c in range(3)])


_made = {}


def sweep_case(name):
    if name not in _made:
        _made[name] = SweepCase(name)
    return _made[name]


# ---- the binary64 reference: first contact of the swept sphere by a loop over every primitive, numpy, no code of the mirror's ----
def _roots64(A, B, Cc):
    """The lesser root of A t^2 + 2 B t + Cc = 0 where it is real and A > 0, else inf."""
    disc = B * B - A * Cc
    ok = (A > 0) & (disc >= 0)
    return np.where(ok, (-B - np.sqrt(np.where(ok, disc, 0.0))) / np.where(ok, A, 1.0), np.inf)


def tri_toi64(o, d, R, t):
    """First contact times in [0, inf] of the sphere of radius R (scalar) from o along d (both [3]) with triangles t [m, 3, 3]: 0 where
    it starts within R, else the least of the offset face, the three edge cylinders and the three vertex spheres."""
    m = len(t)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    best = np.full(m, np.inf)
    dd = float(d @ d)
    # face
    n = np.cross(b - a, c - a)
    ln = np.linalg.norm(n, axis=1)
    okn = ln > 0
    n = n / np.where(okn, ln, 1.0)[:, None]
    h = ((o - a) * n).sum(axis=1)
    g = n @ d
    side = np.where(h >= 0, 1.0, -1.0)
    appr = okn & (side * g < 0) & (np.abs(h) > R)
    tf = np.where(appr, (np.abs(h) - R) / np.where(appr, -side * g, 1.0), np.inf)
    p = o + d * np.where(appr, tf, 0.0)[:, None] - n * (side * R)[:, None]
    inside = np.ones(m, bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(v - u, p - u) * n).sum(axis=1) >= 0
    best = np.where(appr & inside, tf, best)
    # edges
    for u, v in ((a, b), (b, c), (c, a)):
        e = v - u
        ee = (e * e).sum(axis=1)
        oke = ee > 0
        ee1 = np.where(oke, ee, 1.0)
        w = o - u
        de, we = e @ d, (w * e).sum(axis=1)
        te = _roots64(dd - de * de / ee1, w @ d - we * de / ee1, (w * w).sum(axis=1) - we * we / ee1 - R * R)
        fin = np.isfinite(te)
        s = (we + de * np.where(fin, te, 0.0)) / ee1
        te = np.where(oke & fin & (te >= 0) & (s >= 0) & (s <= 1), te, np.inf)
        best = np.minimum(best, te)
    # vertices
    for u in (a, b, c):
        w = o - u
        tv = _roots64(np.full(m, dd), w @ d, (w * w).sum(axis=1) - R * R)
        best = np.minimum(best, np.where(tv >= 0, tv, np.inf))
    start = tri_dist64(np.broadcast_to(o, (m, 3)), t)[0] <= R
    return np.where(start, 0.0, best)


def sphere_toi64(o, d, R, centre, rad):
    """The same against sphere surfaces centre [m, 3], rad [m]."""
    w = o - centre
    dd = float(d @ d)
    l = np.linalg.norm(w, axis=1)
    out_t = _roots64(np.full(len(w), dd), w @ d, l * l - (rad + R) ** 2)
    out_t = np.where(out_t >= 0, out_t, np.inf)
    B, Cc = w @ d, l * l - (rad - R) ** 2
    disc = B * B - dd * Cc
    in_t = np.where((rad - R > 0) & (disc >= 0), (-B + np.sqrt(np.maximum(disc, 0.0))) / dd, np.inf)
    t = np.where(l > rad, out_t, in_t)
    return np.where(np.abs(l - rad) <= R, 0.0, t)


def first_contact64(geo, sweeps, radius):
    """t64(R): the binary64 brute-force first contact of every sweep at the radii `radius` [n] (tmax where there is none).  Triangles whose
    bounding sphere the swept sphere cannot reach are left out, which changes no minimum."""
    s = np.asarray(sweeps, np.float64)
    out = s[:, 7].copy()
    quads = []
    for k in range(geo.nq):
        c = [geo.anchor[k] + a * geo.E1[k] + b * geo.E2[k] for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))]
        quads += [[c[0], c[1], c[2]], [c[0], c[2], c[3]]]
    quads = np.array(quads).reshape(-1, 3, 3)
    if geo.nt:
        cen = geo.tri.mean(axis=1)
        rad = np.linalg.norm(geo.tri - cen[:, None, :], axis=2).max(axis=1)
    for i in range(len(s)):
        o, d, R, tmax = s[i, 0:3], s[i, 3:6], float(radius[i]), s[i, 7]
        best = np.inf
        if geo.ns:
            best = min(best, sphere_toi64(o, d, R, geo.centre, geo.radius).min())
        if len(quads):
            best = min(best, tri_toi64(o, d, R, quads).min())
        if geo.nt:
            w = cen - o
            tt = np.clip((w @ d) / (d @ d), 0.0, tmax)
            near = np.linalg.norm(w - tt[:, None] * d, axis=1) <= (R + rad) * (1 + 1e-9) + 1e-12 * np.abs(o).max()
            if near.any():
                best = min(best, tri_toi64(o, d, R, geo.tri[near]).min())
        if best <= tmax:
            out[i] = best
    return out


def prim_dist64_at(geo, q, prim):
    """Binary64 distance from q[i] to primitive prim[i] (>= 0): spheres by their surface, quads as their two triangles."""
    q = np.asarray(q, np.float64)
    out = np.zeros(len(q))
    s = prim < geo.ns
    if s.any():
        out[s] = sphere_dist64(q[s], geo.centre[prim[s]], geo.radius[prim[s]])
    k = (prim >= geo.ns) & (prim < geo.ns + geo.nq)
    if k.any():
        i = prim[k] - geo.ns
        c = [geo.anchor[i] + a * geo.E1[i] + b * geo.E2[i] for a, b in ((0, 0), (1, 0), (1, 1), (0, 1))]
        out[k] = np.minimum(tri_dist64(q[k], np.stack([c[0], c[1], c[2]], axis=1))[0], tri_dist64(q[k], np.stack([c[0], c[2], c[3]], axis=1))[0])
    t = prim >= geo.ns + geo.nq
    if t.any():
        out[t] = tri_dist64(q[t], geo.tri[prim[t] - geo.ns - geo.nq])[0]
    return out


def bracket_misses(geo, sweeps, hits, S, eps):
    """The rows of the valid sweeps that miss the binary64 checks at this eps, as (residual rows, bracket rows):
      residual   | dist64(c(t), prim) - radius | <= eps S at every contact with t > 0; dist64 <= radius + eps S at a start in contact (t = 0),
                 which has no first touch to measure
      bracket    t64(radius + eps S) - eps S / |d| <= t <= t64(radius - eps S) + eps S / |d|  (a miss reports t = tmax, as t64 does)"""
    s = np.asarray(sweeps, np.float64)
    t, prim = hits["t"].astype(np.float64), hits["prim"]
    r, dn = s[:, 6], np.linalg.norm(s[:, 3:6], axis=1)
    hit = prim >= 0
    dist = np.zeros(len(s))
    dist[hit] = prim_dist64_at(geo, s[hit, 0:3] + s[hit, 3:6] * t[hit, None], prim[hit])
    bad_res = hit & np.where(t > 0, np.abs(dist - r) > eps * S, dist > r + eps * S)
    lo = first_contact64(geo, s, r + eps * S) - eps * S / dn
    hi = first_contact64(geo, s, np.maximum(r - eps * S, 0.0)) + eps * S / dn
    return np.where(bad_res)[0], np.where((t < lo) | (t > hi))[0]


# ---- exact cases: integer and power-of-two coordinates, every intermediate of the definition exact, t representable ----
def exact_mesh_scene():
    """Five faces alone in a scene: 0 and 1 the same triangle (0,0,0) (4,0,0) (0,4,0); 2 a small one far away; 3 three collinear vertices
    on y = 20; 4 three coincident vertices at (7, 40, 7)."""
    from common import MovedScene
    from sign_helpers import _mesh_only
    t = [[0, 0, 0, 4, 0, 0, 0, 4, 0]] * 2 + [[100, 100, 100, 101, 100, 100, 100, 101, 100], [0, 20, 0, 2, 20, 0, 4, 20, 0], [7, 40, 7] * 3]
    return _mesh_only(MovedScene(M.HostScene("file:coffee", 64, 36), np.array(t, np.float32), new_faces=True))


def _rec(t, prim, mat, u, v, p):
    r = np.zeros(1, SWEEP_DTYPE)
    r["t"], r["prim"], r["mat"], r["u"], r["v"], r["p"] = t, prim, mat, u, v, p
    return r


def exact_mesh_cases():
    """(names, sweeps [k, 8], expected records [k]) on exact_mesh_scene, radius 2 and |d| = 2 throughout."""
    below3 = np.nextafter(np.float32(3.0), np.float32(0.0))
    miss = lambda tmax: _rec(tmax, -1, -1, 0, 0, (0, 0, 0))
    face = _rec(3, 0, 0, 0.25, 0.25, (1, 1, 0))
    rows = [("face head-on; of two coincident triangles the lower id", [1, 1, 8, 0, 0, -2, 2, 16], face),
            ("vertex straight on", [12, 0, 0, -2, 0, 0, 2, 16], _rec(3, 0, 0, 1, 0, (4, 0, 0))),
            ("starts in contact", [1, 1, 1, 0, 0, 2, 2, 16], _rec(0, 0, 0, 0.25, 0.25, (1, 1, 0))),
            ("ends exactly at contact", [1, 1, 8, 0, 0, -2, 2, 3], face),
            ("ends an ulp before contact", [1, 1, 8, 0, 0, -2, 2, below3], miss(below3)),
            ("zero-area triangle: the edge", [1, 20, 8, 0, 0, -2, 2, 16], _rec(3, 3, 0, 0.5, 0, (1, 20, 0))),
            ("three coincident vertices: the vertex", [7, 40, 15, 0, 0, -2, 2, 16], _rec(3, 4, 0, 0, 0, (7, 40, 7)))]
    return [r[0] for r in rows], np.array([r[1] for r in rows], np.float32), np.concatenate([r[2] for r in rows])


def exact_sphere_scene():
    """The scene "spheres" with sphere i moved to (16 i, 64, 0), radius 2: (scene, the sphere table for moptix_update_spheres)."""
    from common import MovedScene
    hs = M.HostScene("spheres", 64, 36)
    n = hs.sizes.nSpheres
    sph = (M._capi.SphereParams * n)()
    for i in range(n):
        sph[i] = hs.flat()["spheres"][i]
        sph[i].center.x, sph[i].center.y, sph[i].center.z, sph[i].radius = 16.0 * i, 64.0, 0.0, 2.0
    return MovedScene(hs, spheres=sph), sph


def exact_sphere_case(hs):
    """A sphere primitive head-on: (sweeps [1, 8], expected record [1])."""
    mat = int(np.asarray(hs.flat()["sphereMat"])[0])
    return np.array([[0, 64, 16, 0, 0, -2, 2, 16]], np.float32), _rec(6, 0, mat, 0, 0, (0, 64, 2))
