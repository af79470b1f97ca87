"""Adversarial deformations for the in-place refit (csrc/refitkernel.hip, api_refit.hip, pt_refit.h) and for everything that walks a refitted
tree: deterministic functions fp0 [n, 9] float32 -> fp [n, 9] float32 on the adversarial meshes of lbvh_cases.py, the ray set of a
(case, deformation) pair, the pairs and trees the GPU tests run, and a numpy evaluation of the tree's surface-area cost from its definition
in include/moptix.h.  Every value is finite and every seed is fixed.

The deformations keep the number of faces and know nothing of the tree: a refit keeps the topology the builder chose for fp0, so the boxes
of `shuffle`, `reverse` and `swap_halves` grow towards the scene box and a walk visits most of the tree; the collapses make boxes of no
extent; `explode`, `shrink` and `offset` move the magnitudes, and with them the padding and the 64-byte nodes' grids, by many binades."""
import numpy as np

import lbvh_cases
from common import MovedScene
from query_helpers import make_rays
from refit_helpers import strip_scene

N_RAYS = 1024
HIT_SHARE = 8                                  # the loop over all triangles hits with at least one ray in HIT_SHARE
OFFSET_DIR = np.array([1.0, -1.0, 1.0])
SLAB_REACH = 3e19                              # the coordinates up to which a ray with a zero direction component is walked rightly


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32).reshape(-1, 9))


def _v(fp0):
    return np.asarray(fp0, np.float32).astype(np.float64).reshape(-1, 3, 3)


def centroid(fp0):
    """The mean of all corners, rounded to binary32."""
    return _v(fp0).reshape(-1, 3).mean(axis=0).astype(np.float32).astype(np.float64)


def areas(fp):
    """Twice the area of every face of the binary32 positions, in binary64: 0.0 exactly where two corners coincide."""
    v = _v(fp)
    return np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)


def collapse_point(fp0):
    """Every vertex moves to the centroid: every box is one point, every triangle has zero area."""
    return _f32(np.broadcast_to(centroid(fp0), _v(fp0).shape))


def _flatten(axis):
    def f(fp0):
        v = _v(fp0)
        v[:, :, axis] = centroid(fp0)[axis]
        return _f32(v)
    f.__doc__ = "Coordinate %d of every vertex set to the centroid's: every box is flat on that axis." % axis
    return f


flatten_x, flatten_y, flatten_z = _flatten(0), _flatten(1), _flatten(2)


def _scale(s):
    def f(fp0):
        c = centroid(fp0)
        return _f32(c + (_v(fp0) - c) * s)
    f.__doc__ = "Scaled about the centroid by %g." % s
    return f


explode = _scale(1e6)


def shrink_factor(fp0):
    """The factor of `shrink`: 1e-6, or the next power of ten above it at which a tenth of the faces of non-zero area keep one.  The scaled
    scene lies within s x its size of the centroid, and a centroid far from the origin quantises it: `mixed` (centroid near -1200 on x, an
    ulp of 1.2e-4 there) keeps 108 faces of 6,696 at 1e-6, one or two ulps wide, which a binary32 ray cannot be aimed at: its ray set hit
    with 108 rays of 1,024.  At 1e-5 half of its cloud keeps its triangles (its log-spaced cluster, smaller than that ulp as it is,
    collapses at any factor below 1).  The geometric chains lose their small triangles at any factor and keep a fifth at 1e-6."""
    v, c, keep = _v(fp0), centroid(fp0), areas(fp0) > 0
    for k in range(-6, 0):
        if 10 * int((areas(_f32(c + (v - c) * 10.0 ** k))[keep] > 0).sum()) >= int(keep.sum()):
            return 10.0 ** k
    raise AssertionError("no factor keeps a tenth of the areas")


def shrink(fp0):
    """Scaled about the centroid by shrink_factor (1e-6 where the centroid's magnitude allows it)."""
    c = centroid(fp0)
    return _f32(c + (_v(fp0) - c) * shrink_factor(fp0))


def offset_magnitude(fp0):
    """The translation of `offset`: m x (1, -1, 1) with m a sixteenth of the largest power of two at which every face of non-zero area
    keeps a non-zero area in binary32.  At the largest one itself the smallest triangles are a few units in the last place wide and a
    binary32 ray cannot be aimed at them (no ray of the set hit anything there); four more bits leave them their shape roughly."""
    v, keep = _v(fp0), areas(fp0) > 0
    for k in range(40, -60, -1):
        if (areas(_f32(v + 2.0 ** k * OFFSET_DIR))[keep] > 0).all():
            return 2.0 ** (k - 4)
    raise AssertionError("no translation keeps the areas")


def offset(fp0):
    """A translation far from the origin (offset_magnitude): quantised corners, relative padding far from the origin."""
    return _f32(_v(fp0) + offset_magnitude(fp0) * OFFSET_DIR)


def shuffle(fp0):
    """Face k takes the positions of face perm[k]."""
    return np.ascontiguousarray(np.asarray(fp0, np.float32)[np.random.default_rng(201).permutation(len(fp0))])


def reverse(fp0):
    """Face k takes the positions of face n - 1 - k."""
    return np.ascontiguousarray(np.asarray(fp0, np.float32)[::-1])


def swap_halves(fp0):
    """The two halves of the face array exchange positions: face k takes those of face (k + ceil(n / 2)) mod n."""
    n = len(fp0)
    return np.ascontiguousarray(np.roll(np.asarray(fp0, np.float32), -((n + 1) // 2), axis=0))


def _outlier(d):
    def f(fp0):
        v = _v(fp0)
        v[len(v) // 2, :, 0] += d
        return _f32(v)
    return f


outlier, outlier_wide = _outlier(1e9), _outlier(3e10)
outlier.__doc__ = "The middle face sent 1e9 away along x: within the reach of the 64-byte nodes' grid (pt_lbvh.h kNode64MaxStep x 255)."
outlier_wide.__doc__ = "The middle face sent 3e10 away along x: some node is wider than the grid reaches, the 64-byte form has to go."


def to_points(fp0):
    """Every third face becomes three equal vertices."""
    v = _v(fp0)
    v[::3, 1] = v[::3, 0]; v[::3, 2] = v[::3, 0]
    return _f32(v)


def to_slivers(fp0):
    """Every third face gets two equal vertices."""
    v = _v(fp0)
    v[::3, 2] = v[::3, 1]
    return _f32(v)


DEFORMATIONS = dict(collapse_point=collapse_point, flatten_x=flatten_x, flatten_y=flatten_y, flatten_z=flatten_z, explode=explode, shrink=shrink,
                    offset=offset, shuffle=shuffle, reverse=reverse, swap_halves=swap_halves, outlier=outlier, outlier_wide=outlier_wide,
                    to_points=to_points, to_slivers=to_slivers)
DEFORMATION_NAMES = tuple(DEFORMATIONS)
FEW = ("shuffle", "collapse_point", "explode", "to_points")                 # what the cases outside EVERY run on the GPU
STRIP = "strip_3"                                                           # refit_helpers.strip_scene(3): the root is a leaf
BASE_CASES = ("counts_9", "counts_257", "counts_2049", "duplicates", "degenerate", "geometric", "geometric_wide", "mixed", "big_first_1_300", STRIP)
EVERY = ("counts_257", "geometric", "mixed")                                # the cases that run every deformation on the GPU
ALL_TREES = "counts_257"                                                    # the case that runs every leaf size and both builders
CPU_PAIRS = tuple((c, d) for c in BASE_CASES for d in DEFORMATION_NAMES)
GPU_PAIRS = tuple((c, d) for c in BASE_CASES for d in (DEFORMATION_NAMES if c in EVERY else FEW))
# (case, deformation, leaf size, builder) of the GPU file
GPU_RUNS = tuple((c, d, leaf, b) for c, d in GPU_PAIRS for leaf, b in ([(l, b) for l in lbvh_cases.LEAVES for b in lbvh_cases.BUILDERS]
                                                                         if c == ALL_TREES else [(4, 1)]))

_base, _moved, _rays = {}, {}, {}


def base_scene(name):
    """The case before the move, in coffee's frame, materials and lights (made once: the tests only read it)."""
    if name not in _base:
        _base[name] = strip_scene(3) if name == STRIP else lbvh_cases.case_scene(name)
    return _base[name]


def base_faces(name):
    return base_scene(name).face_arrays()[0]


def moved_faces(name, deformation):
    """fp [n, 9] float32 of the pair, made once and only read."""
    key = (name, deformation)
    if key not in _moved:
        fp = DEFORMATIONS[deformation](base_faces(name))
        assert fp.dtype == np.float32 and fp.shape == base_faces(name).shape and np.isfinite(fp).all()
        fp.setflags(write=False)
        _moved[key] = fp
    return _moved[key]


def moved_scene(name, deformation):
    """A scene of the moved faces that knows no tree and no refit: what the oracle and the *brute helpers are handed."""
    return MovedScene(base_scene(name), moved_faces(name, deformation))


def rays_of(fp, n=N_RAYS, seed=6):
    """The ray set of moved faces, [n, 8] float32 (o, d, tmin = 0, tmax), made as lbvh_cases.case_rays makes a case's: five eighths aimed at
    a random point inside a random triangle (one of non-zero area where there is one) -- every other one from outside the scene's box, the
    others from a few triangle sizes away, so that the small triangles of a scene of many scales are met too; three sixteenths with
    uniform origins in the scene's box and uniform directions; three sixteenths parallel to an axis with exact zeros in the direction,
    half of them through a triangle's box centre.
    The axis-parallel part is made while the coordinates stay below SLAB_REACH.  The slab test takes a zero direction component as
    +-1e-19 so that plane / d stays finite, which it does up to there -- "beyond every scene whose box areas are finite floats"
    (pt_path.h kSlabMinDir).  A scene past it is outside what the walk is defined on for such rays: its share goes
    to the aimed rays.  (`explode` takes geometric_wide to 1e24; no other pair comes near.)"""
    v = _v(fp)
    rng = np.random.default_rng(seed)
    lo, hi = v.min(axis=1), v.max(axis=1)
    cen, size = 0.5 * (lo + hi), np.maximum((hi - lo).max(axis=1), 1e-30)
    slo, shi = lo.min(axis=0), hi.max(axis=0)
    diag = max(float(np.linalg.norm(shi - slo)), 1e-3 * float(np.abs(v).max()), 1e-30)
    nu = 3 * n // 16
    nx = 3 * n // 16 if float(np.abs(v).max()) < SLAB_REACH else 0
    na = n - nu - nx

    def unit(k):
        d = rng.normal(size=(k, 3)); return d / np.linalg.norm(d, axis=1, keepdims=True)
    # aimed
    solid = np.nonzero(areas(fp) > 0)[0]
    pool = solid if len(solid) else np.arange(len(v))
    f = pool[rng.integers(0, len(pool), na)]
    a, b = rng.uniform(0.1, 0.9, na), rng.uniform(0.1, 0.9, na)
    flip = a + b > 1
    a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
    target = v[f, 0] + a[:, None] * (v[f, 1] - v[f, 0]) + b[:, None] * (v[f, 2] - v[f, 0])
    d = unit(na)
    dist = np.where(np.arange(na) % 2 == 0, 2.0 * diag, 4.0 * size[f])
    aimed = make_rays(target - dist[:, None] * d, d, tmin=0.0)
    # uniform
    ext = np.maximum(shi - slo, 1e-3 * diag)
    uni = make_rays(rng.uniform(slo - 0.1 * ext, shi + 0.1 * ext, (nu, 3)), unit(nu), tmin=0.0)
    # axis-parallel
    f = rng.integers(0, len(v), nx)
    ax = rng.integers(0, 3, nx); sgn = rng.choice([-1.0, 1.0], nx)
    d = np.zeros((nx, 3)); d[np.arange(nx), ax] = sgn
    jit = rng.uniform(-0.5, 0.5, (nx, 3)) * size[f][:, None] * (np.arange(nx) % 2)[:, None]
    dist = np.where(np.arange(nx) % 4 < 2, 2.0 * diag, 4.0 * size[f])
    org = cen[f] + jit
    org[np.arange(nx), ax] = cen[f][np.arange(nx), ax] - sgn * dist
    axial = make_rays(org, d, tmin=0.0)
    rays = np.ascontiguousarray(np.concatenate([aimed, uni, axial]))
    assert rays.shape == (n, 8) and np.isfinite(rays).all()
    return rays


def pair_rays(name, deformation):
    key = (name, deformation)
    if key not in _rays:
        _rays[key] = rays_of(moved_faces(name, deformation))
        _rays[key].setflags(write=False)
    return _rays[key]


def sah_cost(nodes):
    """include/moptix.h sahCost from read-back nodes ([m, 32] words, Node128), in numpy binary64: the sum over every child slot in use of
    every node of surface area(child box) x (1 for a node child, the triangle count for a leaf child), divided by the surface area of the
    union of the root's child boxes; 0 for a tree without nodes.  (Half areas on both sides: the factor cancels.)"""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 32)
    if len(nodes) == 0:
        return 0.0
    box = nodes.view(np.float32)[:, 0:24].reshape(-1, 6, 4).astype(np.float64)
    refs = nodes[:, 24:28].view(np.int32).astype(np.int64)
    used = refs != lbvh_cases.K_EMPTY_REF

    def half_area(lo, hi):
        e = hi - lo
        return e[..., 0] * e[..., 1] + e[..., 1] * e[..., 2] + e[..., 2] * e[..., 0]
    lo, hi = np.moveaxis(box[:, 0:3], 1, 2), np.moveaxis(box[:, 3:6], 1, 2)      # [m, child, axis]
    weight = np.where(refs < 0, ((~refs) & 7) + 1, 1).astype(np.float64)
    total = float((half_area(lo, hi) * weight)[used].sum())
    root = half_area(lo[0][used[0]].min(axis=0), hi[0][used[0]].max(axis=0))
    return total / float(root) if root > 0 else 0.0


def leaf_interior_range(built, n):
    """Faces a .. b - 1 of the middle half whose first face is not the first record of its leaf and whose last face is not the last of its."""
    prim = built["tris"][:, 7].view(np.int32)
    slot = np.empty(n, np.int64); slot[prim] = np.arange(n)
    first, last = np.zeros(n, bool), np.zeros(n, bool)
    refs = built["nodes"][:, 24:28].view(np.int32).reshape(-1)
    for r in refs[(refs < 0)]:
        f, c = (~int(r)) >> 3, ((~int(r)) & 7) + 1
        first[f] = True; last[f + c - 1] = True
    a = next(f for f in range(n // 4, n) if not first[slot[f]])
    b = next(f for f in range(3 * n // 4, a, -1) if not last[slot[f]]) + 1
    assert 0 < a < b - 1 < n - 1
    return a, b
