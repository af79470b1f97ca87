"""The oriented box queries of the CPU mirror (tests/obbsim/obbsim.cpp, a library of its own beside libhostsim.so): the walk through the
kernel's per-box code and the definition itself as a loop over every primitive record; the query sets the oriented box tests share; and a
binary64 separating-axis gap in the box's own frame, from the scene's original vertices mapped by the query's own sixteen floats (numpy),
which shares no code with the mirror.  The exact rational reference is box_helpers' on the world box of a signed-permutation frame."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

from box_helpers import BOX_ANY, BOX_COUNT, MODES, csr, membership, scene_extent      # noqa: F401  (for the tests)
from common import REPO, _f32, _ptr, hostsim_handle, hostsim_lib
from point_helpers import Geometry      # noqa: F401  (for the tests)
from query_helpers import same_bits     # noqa: F401  (for the tests)

ORTHO = 2.0 ** -10                                        # kObbOrtho, spelled out here apart from the header's definition

_DIR = os.path.join(REPO, "tests", "obbsim")
_obbsim = None


def _lib():
    """tests/obbsim/libobbsim.so (built here if it is missing, as common.hostsim_lib builds its library) with the signatures of its
    entries.  They take the handles of common.HostsimHandle."""
    global _obbsim
    if _obbsim is None:
        hostsim_lib()
        path = os.path.join(_DIR, "libobbsim.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _DIR, "-s"])
        L = C.CDLL(path)
        vp, f32p, i32p, i64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        L.obbsim_query.argtypes, L.obbsim_query.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int, i32p], C.c_int
        L.obbsim_list.argtypes, L.obbsim_list.restype = [vp, C.c_int, f32p, C.c_int64, i64p, i32p, i32p], C.c_int
        L.obbsim_brute.argtypes, L.obbsim_brute.restype = [vp, f32p, C.c_int64, C.c_int, i32p], C.c_int
        L.obbsim_brute_list.argtypes, L.obbsim_brute_list.restype = [vp, f32p, C.c_int64, i64p, i32p, i32p], C.c_int
        L.obbsim_stack_depth.argtypes, L.obbsim_stack_depth.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int], C.c_int
        L.obbsim_work.argtypes, L.obbsim_work.restype = [vp, C.c_int, f32p, C.c_int64, i64p, i64p], C.c_int
        for name in ("obbsim_tri", "obbsim_sphere", "obbsim_quad"):
            getattr(L, name).argtypes, getattr(L, name).restype = [f32p, f32p, C.c_int64, i32p], C.c_int
        _obbsim = L
    return _obbsim


def _obbs(obbs):
    return _f32(np.asarray(obbs, np.float32).reshape(-1, 16))


def obbsim(hs, obbs, mode="any", node_format=64, leaf_size=4):
    """moptix_query_obbs on the CPU, by the walk: int32 per box.  hs: a scene, or a built one."""
    sim = hostsim_handle(hs, leaf_size)
    b = _obbs(obbs)
    out = np.zeros(len(b), np.int32)
    assert _lib().obbsim_query(sim._h, int(node_format), _ptr(b), len(b), MODES[mode], _ptr(out, C.c_int32)) == 0
    return out


def obbbrute(hs, obbs, mode="any", leaf_size=4):
    """The same from the definition: every primitive record through its predicate, no tree."""
    sim = hostsim_handle(hs, leaf_size)
    b = _obbs(obbs)
    out = np.zeros(len(b), np.int32)
    assert _lib().obbsim_brute(sim._h, _ptr(b), len(b), MODES[mode], _ptr(out, C.c_int32)) == 0
    return out


def _list(entry, sim, b, offsets, fill):
    offsets = np.ascontiguousarray(offsets, np.int64)
    prims = np.full(int(offsets[-1]) if len(offsets) else 0, fill, np.int32)
    counts = np.zeros(len(b), np.int32)
    keep = np.zeros(1, np.int32) if len(prims) == 0 else prims      # a valid address for an empty list
    assert entry(sim, _ptr(b), len(b), _ptr(offsets, C.c_int64), _ptr(keep, C.c_int32), _ptr(counts, C.c_int32)) == 0
    return prims, counts


def obbsim_list(hs, obbs, offsets, node_format=64, leaf_size=4, fill=-7):
    """moptix_query_obbs_list on the CPU, by the walk: (prims, counts); prims starts out as `fill` throughout."""
    sim = hostsim_handle(hs, leaf_size)
    L = _lib()
    return _list(lambda s, *a: L.obbsim_list(s._h, int(node_format), *a), sim, _obbs(obbs), offsets, fill)


def obbbrute_list(hs, obbs, offsets, leaf_size=4, fill=-7):
    """The same from the definition, the ids sorted by the library's sort."""
    sim = hostsim_handle(hs, leaf_size)
    L = _lib()
    return _list(lambda s, *a: L.obbsim_brute_list(s._h, *a), sim, _obbs(obbs), offsets, fill)


def obb_stack_depth(hs, obbs, mode="count", node_format=64, leaf_size=4):
    """Most stack entries the walk of any of the boxes holds."""
    sim = hostsim_handle(hs, leaf_size)
    b = _obbs(obbs)
    d = _lib().obbsim_stack_depth(sim._h, int(node_format), _ptr(b), len(b), MODES[mode])
    assert d >= 0
    return d


def obb_work(hs, obbs, node_format=64, leaf_size=4):
    """(node steps, triangles tested) of the count walk, int64 per box."""
    sim = hostsim_handle(hs, leaf_size)
    b = _obbs(obbs)
    steps, tested = np.zeros(len(b), np.int64), np.zeros(len(b), np.int64)
    assert _lib().obbsim_work(sim._h, int(node_format), _ptr(b), len(b), _ptr(steps, C.c_int64), _ptr(tested, C.c_int64)) == 0
    return steps, tested


def predicate(kind, prims, obbs):
    """The mirror's predicate `kind` ("tri": 9 floats, three vertices; "sphere": centre and radius; "quad": the record's v1, v2, anchor)
    pair by pair: prims [n, 9 or 4], obbs [n, 16] -> bool [n]."""
    p, b = _f32(prims), _obbs(obbs)
    assert len(p) == len(b)
    out = np.zeros(len(b), np.int32)
    assert getattr(_lib(), "obbsim_" + kind)(_ptr(p), _ptr(b), len(b), _ptr(out, C.c_int32)) == 0
    return out != 0


# ---- building boxes ----
def pack(centre, half, axes):
    """(n, 16) float32 rows from centres [n, 3], half-extents [n, 3] and axes [n, 3, 3] (axes[i, j] = box axis j as a world direction),
    written out here apart from the package's oriented_boxes (which takes the transpose, a local-to-world matrix)."""
    n = len(centre)
    out = np.zeros((n, 16), np.float32)
    out[:, 0:3], out[:, 3:6], out[:, 6:15] = centre, half, np.asarray(axes).reshape(n, 9)
    return out


def random_rotations(rng, n):
    """n rotation matrices uniform over SO(3) (from unit quaternions), binary64; rows are the box axes."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def axis_rotation(axis, angle):
    """The rotation by `angle` about world axis 0, 1 or 2, binary64."""
    c, s = np.cos(angle), np.sin(angle)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


def signed_permutations():
    """All 48 signed permutation matrices [48, 3, 3]: row j is +-e_sigma(j)."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3))
            for j in range(3):
                m[j, perm[j]] = signs[j]
            out.append(m)
    return np.array(out)


def frame_from(direction):
    """An orthonormal frame [3, 3] whose axis 0 is `direction` (normalised), binary64."""
    a0 = np.asarray(direction, np.float64)
    a0 = a0 / np.linalg.norm(a0)
    t = np.eye(3)[int(np.argmin(np.abs(a0)))]
    a1 = np.cross(a0, t); a1 /= np.linalg.norm(a1)
    return np.stack([a0, a1, np.cross(a0, a1)])


DIAGONALS = [np.array(d, np.float64) for d in ((1, 1, 1), (1, -1, 1), (-1, 1, 1), (1, 1, -1), (1, 1, 0), (1, 0, -1), (0, 1, 1), (1, -1, 0))]


def beam_set(geo, lo, hi, rng, n=128):
    """n thin beams on diagonals: half of them 100:1, half 1000:1; the long half-extent 5 % to 30 % of the scene's diagonal; centred on
    surface points."""
    diag = max(float(np.linalg.norm(np.asarray(hi, np.float64) - np.asarray(lo, np.float64))), 1e-30)
    c = geo.surface_points(rng, n)
    long_half = diag * rng.uniform(0.05, 0.30, n)
    ratio = np.where(np.arange(n) % 2 == 0, 100.0, 1000.0)
    h = np.stack([long_half, long_half / ratio, long_half / ratio], axis=1)
    axes = np.array([frame_from(DIAGONALS[i % len(DIAGONALS)]) for i in range(n)])
    return pack(c, h, axes)


def obb_sets(geo, lo, hi, seed=30):
    """The oriented boxes of a scene as one float32 [n, 16] array (about 1,500) and the slices of its parts:
      random    512 boxes centred uniformly in the box lo .. hi enlarged by a quarter of its size on each side and 256 centred on surface
                points, uniform random rotations, half-extents diag x 10^k per axis, k uniform in [log10(0.0005), log10(0.15)] (extents
                of 0.1 % to 30 % of the scene)
      beams     beam_set: 128 thin beams, 100:1 and 1000:1, on diagonals
      tilted    96 boxes on surface points rotated about a world axis by 1e-4 rad or by exactly 45 degrees
      permuted  96: all 48 signed permutations as axes, at two sizes, on surface points
      flat      96 boxes on surface points with one, two and three zero half-extents, random rotations
      touching  200 boxes one of whose faces is placed on a surface point, a mesh vertex where the scene has triangles:
                c = v - a0 h0 - t1 a1 h1 - t2 a2 h2 with |t| < 1
      far       32 boxes centred 1e4 scene diagonals away: 16 small ones, and 16 beams long enough to reach back to the scene
      special   the box holding the whole scene (random rotation), then the invalid ones: a NaN and an inf in the centre, a NaN in an
                axis, an inf half-extent, a negative half-extent, an axis of length 1.01, two axes 0.01 off orthogonal"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    diag = max(float(np.linalg.norm(hi - lo)), 1e-30)
    size = np.maximum(hi - lo, 1e-3 * diag)
    ext = lambda n: diag * 10.0 ** rng.uniform(np.log10(0.0005), np.log10(0.15), (n, 3))
    parts, rows = {}, []

    def add(name, block):
        first = sum(len(r) for r in rows)
        rows.append(block); parts[name] = slice(first, first + len(block))

    c = np.concatenate([rng.uniform(lo - 0.25 * size, hi + 0.25 * size, (512, 3)), geo.surface_points(rng, 256)])
    add("random", pack(c, ext(768), random_rotations(rng, 768)))
    add("beams", beam_set(geo, lo, hi, rng))
    angles = np.where(np.arange(96) % 2 == 0, 1e-4, np.pi / 4)
    add("tilted", pack(geo.surface_points(rng, 96), ext(96), np.array([axis_rotation(i % 3, angles[i]) for i in range(96)])))
    sp = signed_permutations()
    add("permuted", pack(geo.surface_points(rng, 96), np.concatenate([ext(48), 0.02 * ext(48)]), np.concatenate([sp, sp])))
    h = ext(96)
    for i in range(96):
        h[i, rng.permutation(3)[:1 + i % 3]] = 0.0
    add("flat", pack(geo.surface_points(rng, 96), h, random_rotations(rng, 96)))
    if geo.nt:
        v = geo.tri.reshape(-1, 3)[rng.integers(0, 3 * geo.nt, 200)].astype(np.float32).astype(np.float64)
    else:
        v = geo.surface_points(rng, 200)
    a, h, t = random_rotations(rng, 200), ext(200), rng.uniform(-1.0, 1.0, (200, 2))
    a[::4] = sp[rng.integers(0, 48, 50)]
    c = v - a[:, 0] * h[:, 0:1] - t[:, 0:1] * a[:, 1] * h[:, 1:2] - t[:, 1:2] * a[:, 2] * h[:, 2:3]
    add("touching", pack(c, h, a))
    d = random_rotations(rng, 32)[:, 0]
    mid = 0.5 * (lo + hi)
    c = mid + 1e4 * diag * d
    h = np.concatenate([ext(16), np.stack([1e4 * diag * rng.uniform(0.999, 1.001, 16), diag * rng.uniform(0.01, 0.1, 16), diag * rng.uniform(0.01, 0.1, 16)], axis=1)])
    a = np.concatenate([random_rotations(rng, 16), np.array([frame_from(d[i]) for i in range(16, 32)])])
    add("far", pack(c, h, a))
    alo, ahi = scene_extent(geo)
    whole = pack([0.5 * (alo + ahi)], [np.full(3, 0.51 * max(float(np.linalg.norm(ahi - alo)), 1e-30))], random_rotations(rng, 1))
    bad = np.repeat(whole, 7, axis=0)
    bad[0, 1] = np.nan; bad[1, 2] = np.inf; bad[2, 10] = np.nan; bad[3, 4] = np.inf; bad[4, 5] = -bad[4, 5]
    bad[5, 6:9] *= np.float32(1.01)
    bad[6, 9:12] += np.float32(0.01) * bad[6, 6:9]
    add("special", np.concatenate([whole, bad]))
    obbs = np.ascontiguousarray(np.concatenate(rows), np.float32)
    parts["whole"] = parts["special"].start
    parts["invalid"] = slice(parts["special"].start + 1, parts["special"].stop)
    return obbs, parts


def valid_obbs(obbs):
    """The header's rule, in binary64 on the binary32 values (none of the tests' boxes is near a threshold)."""
    b = np.asarray(obbs, np.float32).reshape(-1, 16).astype(np.float64)
    a = b[:, 6:15].reshape(-1, 3, 3)
    with np.errstate(invalid="ignore"):
        gram = np.einsum("nik,njk->nij", a, a)
        ok = np.isfinite(b[:, :15]).all(axis=1) & (b[:, 3:6] >= 0).all(axis=1)
        return ok & (np.abs(gram - np.eye(3)) <= ORTHO).all(axis=(1, 2))


def world_aabb(obbs):
    """The enclosing axis-aligned boxes [n, 6] of valid oriented boxes, binary64: c -+ E, E_k = sum_j |a_j.k| h_j."""
    b = np.asarray(obbs, np.float64).reshape(-1, 16)
    e = np.einsum("njk,nj->nk", np.abs(b[:, 6:15].reshape(-1, 3, 3)), b[:, 3:6])
    return np.concatenate([b[:, 0:3] - e, b[:, 0:3] + e], axis=1)


# ---- the binary64 gap in the box's own frame, every box against every primitive ----
def _local(obbs, p):
    """Points p [..., 3] (broadcast against the boxes' leading axis) in the frames of the boxes [nb, 16]: A (p - c), binary64, from the
    query's own floats."""
    b = np.asarray(obbs, np.float64)
    return np.einsum("njk,n...k->n...j", b[:, 6:15].reshape(-1, 3, 3), p - b[:, 0:3].reshape((-1,) + (1,) * (p.ndim - 2) + (3,)))


def tri_gap64(tri, obbs, chunk=64):
    """The largest of the 13 axes' normalised separations of every box [nb, 16] against every triangle [nt, 3, 3] in the box's frame, in
    binary64: [nb, nt]; <= 0 where they overlap.  Axes of zero length are skipped."""
    tri, obbs = np.asarray(tri, np.float64), np.asarray(obbs, np.float64)
    out = np.zeros((len(obbs), len(tri)))
    eye = np.eye(3)
    for first in range(0, len(obbs), chunk):
        b = obbs[first:first + chunk]
        h = b[:, None, 3:6]                                                  # [nb, 1, 3]
        u = _local(b, tri[None])                                             # [nb, nt, 3 vertices, 3]
        f = np.roll(u, -1, axis=2) - u                                       # [nb, nt, 3 edges, 3]
        axes = [np.broadcast_to(eye[a], u.shape[:2] + (3,)) for a in range(3)]
        axes += [np.cross(eye[e], f[:, :, j]) for e in range(3) for j in range(3)]
        axes.append(np.cross(f[:, :, 0], f[:, :, 1]))
        gap = np.full(u.shape[:2], -np.inf)
        for a in axes:
            ln = np.linalg.norm(a, axis=2)
            ok = ln > 0
            a = a / np.where(ok, ln, 1.0)[:, :, None]
            p = (u * a[:, :, None, :]).sum(axis=3)                           # [nb, nt, 3]
            r = (h * np.abs(a)).sum(axis=2)
            s = np.maximum(p.min(axis=2) - r, -p.max(axis=2) - r)
            gap = np.where(ok, np.maximum(gap, s), gap)
        out[first:first + chunk] = gap
    return out


def all_pairs_gap64(geo, obbs):
    """(gap [nb, ns + nq + nt], scale [nb, ns + nq + nt], usable [ns + nq + nt]) in the queries' numbering: gap <= 0 where box and
    primitive overlap (sphere: max(dmin - r, r - dmax) in the box's frame; quad: the lesser of its two triangles' gaps), scale the largest
    |coordinate| of the pair -- of the primitive and of the box's enclosing world box --, usable False for zero-area triangles."""
    b = np.asarray(obbs, np.float64).reshape(-1, 16)
    nb = len(b)
    h = b[:, 3:6]
    cols, scales = [], []
    for i in range(geo.ns):
        m, r = _local(b, geo.centre[i][None]), geo.radius[i]
        dmin = np.linalg.norm(np.maximum(np.abs(m) - h, 0.0), axis=1)
        dmax = np.linalg.norm(np.abs(m) + h, axis=1)
        cols.append(np.maximum(dmin - r, r - dmax)); scales.append(np.full(nb, np.abs(geo.centre[i]).max() + r))
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
    scale = np.maximum(scale, np.abs(world_aabb(b)).max(axis=1)[:, None])
    return gap, scale, usable


def padded_boxes_meeting(tri, extent, aabbs):
    """For every axis-aligned box [nb, 6]: how many triangles [nt, 3, 3] (binary32 vertices) have their padded box -- the builder's, pad =
    1e-5 x extent + 1e-6 |v| per plane -- meeting it.  int64 [nb]."""
    t = np.asarray(tri, np.float32).astype(np.float64)
    tlo, thi = t.min(axis=1), t.max(axis=1)
    tlo, thi = tlo - (1e-5 * extent + 1e-6 * np.abs(tlo)), thi + (1e-5 * extent + 1e-6 * np.abs(thi))
    out = np.zeros(len(aabbs), np.int64)
    for i, q in enumerate(np.asarray(aabbs, np.float64)):
        out[i] = int(((tlo <= q[3:]).all(axis=1) & (thi >= q[:3]).all(axis=1)).sum())
    return out
