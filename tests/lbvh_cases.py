"""Adversarial geometry for the BVH builder (csrc/lbvh.hip, pt_lbvh.h) and the kernels that walk its trees: deterministic face arrays, the
ray set of a case, and a structure check of a built tree that shares no code with the builder or its mirror.

Every generator returns a float32 [n, 9] array (p0 p1 p2 per face) from a fixed numpy seed; case_scene() puts it into coffee's frame,
materials and lights as refit_helpers.strip_scene does.  The coffee camera sits at (0, 0.18, 0.52) and looks along -z; the cases that are
rendered (duplicates, geometric, plane_y) are laid out so that they fill a good part of that view as they are."""
import numpy as np

from common import M, MovedScene
from query_helpers import make_rays

LEAVES, BUILDERS = (1, 4, 8), (0, 1)
K_EMPTY_REF = 0x7ffffffe                       # pt_types.h kEmptyRef
COUNTS = (1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 2047, 2048, 2049, 2050)      # 1, 2, 3, leaf and leaf + 1 of every leaf size, block and kWideCount boundaries
BIG_FIRST = ((1, 300), (299, 1), (2, 0), (0, 300))


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32).reshape(-1, 9))


def _cloud(rng, n, lo, hi, size):
    """n triangles of about `size` with uniform positions in the box lo .. hi."""
    c = rng.uniform(lo, hi, (n, 1, 3))
    return _f32(c + rng.uniform(-size, size, (n, 3, 3)))


def duplicates():
    """One triangle 100 times: the keys differ in the face index only, every SAH extent is 0, every hit is a 100-fold tie (rule D5)."""
    return _f32(np.tile([[-0.6, -0.15, -0.5, 0.6, -0.15, -0.45, 0.0, 0.55, -0.55]], (100, 1)))


def concentric():
    """300 similar triangles whose bounds share the centre (0, 0, 0) exactly: coinciding centroids with different boxes.  The scales span a
    factor below 7, so every one is a 'large' triangle (pt_lbvh.h tri_is_big: 1/49 > 1/64 of the scene box's area) and no root split is forced."""
    base = np.array([[-1, -1, 0], [1, -1, 0.5], [0, 1, -0.5]], np.float64)      # bounds -1..1, -1..1, -0.5..0.5; the plane misses the centre
    s = np.random.default_rng(101).permutation(0.1 * (1.0 + 5.9 * np.arange(300) / 299.0)).astype(np.float32).astype(np.float64)
    return _f32(s[:, None, None] * base[None])


def plane(axis):
    """A 40 x 40 grid of triangles, one per cell (1.4 cells wide and long, corners jittered), in the plane <axis> = 0.0625: one flat axis at
    every level, flat leaf boxes."""
    rng = np.random.default_rng(102 + axis)
    i, j = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
    u0 = -2.0 + 0.1 * (i.reshape(-1, 1) + np.array([0.0, 1.4, 0.0])) + rng.uniform(-0.01, 0.01, (1600, 3))      # the two in-plane coordinates of the corners
    v0 = -4.0 + 0.11 * (j.reshape(-1, 1) + np.array([0.0, 0.0, 1.4])) + rng.uniform(-0.01, 0.01, (1600, 3))
    p = np.full((1600, 3, 3), 0.0625)
    p[:, :, (axis + 2) % 3] = u0                 # plane_y: u = x in -2 .. 2, v = z in -4 .. 0.4 (under the coffee camera)
    p[:, :, (axis + 1) % 3] = v0
    return _f32(p)


def line():
    """257 triangles whose box centres lie on one line parallel to x (y and z centres exactly 0.5 and -0.25: dyadic extents): two flat axes."""
    rng = np.random.default_rng(105)
    n = 257
    cx = rng.uniform(-1.0, 1.0, n)
    hy = rng.integers(1, 64, n) / 1024.0; hz = rng.integers(1, 64, n) / 1024.0
    p = np.zeros((n, 3, 3))
    p[:, :, 0] = cx[:, None] + np.array([-0.01, 0.01, 0.0])
    p[:, :, 1] = 0.5 + hy[:, None] * np.array([-1.0, -1.0, 1.0])
    p[:, :, 2] = -0.25 + hz[:, None] * np.array([-1.0, 1.0, 0.0])
    return _f32(p)


def geometric(x0=1e-8, r=1.3, n=150):
    """Box centres at (0, 0, -x0 r^k), sizes in proportion: a binned sweep peels a few triangles off the far end per level (very unbalanced
    splits, a deep tree).  Each triangle faces the coffee camera; the far ones fill its view.  x0 = 1e-8: span 1e9, a 64-byte form exists."""
    x = x0 * r ** np.arange(n, dtype=np.float64)
    base = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0]], np.float64)            # bounds centred on 0 in x and y, flat in z
    p = x[:, None, None] * base[None]
    p[:, :, 2] = -x[:, None]
    return _f32(p)


def geometric_wide():
    """The same over a span of 1e18: wider than the 64-byte nodes' grid (pt_lbvh.h kNode64MaxStep), so the tree has the 128-byte form only."""
    return geometric(x0=10.0)


def degenerate():
    """500 small triangles in a unit cloud; every 5th and every 7th has two equal vertices, every 35th three: zero-area triangles in real leaves."""
    fp = _cloud(np.random.default_rng(106), 500, (-0.5, 0.0, -1.0), (0.5, 1.0, 0.0), 0.03).reshape(-1, 3, 3)
    k = np.arange(500)
    two = (k % 5 == 0) | (k % 7 == 0)
    fp[two, 1] = fp[two, 0]
    fp[k % 35 == 0, 2] = fp[k % 35 == 0, 0]
    return _f32(fp)


def offset():
    """800 triangles of size 0.05 around (1e6, -1e6, 1e6), where a float32 step is 0.0625: quantised corners, relative padding far from the origin."""
    rng = np.random.default_rng(107)
    c = np.array([1e6, -1e6, 1e6]) + rng.uniform(-2.0, 2.0, (800, 1, 3))
    return _f32(c + rng.uniform(-0.05, 0.05, (800, 3, 3)))


def big_first(b, s):
    """b triangles that span the scene (faces 0 .. b-1) and s small ones: the forced root split of the 'large triangles first' rule."""
    rng = np.random.default_rng(108 + 1000 * b + s)
    corners = np.array([[-1, 0, -1], [1, 0, 1], [-1, 1, 1], [1, 1, -1]], np.float64)
    big = np.stack([corners[rng.permutation(4)[:3]] + rng.uniform(-0.02, 0.02, (3, 3)) for _ in range(b)]) if b else np.zeros((0, 3, 3))
    small = _cloud(rng, s, (-1.0, 0.0, -1.0), (1.0, 1.0, 1.0), 0.01).reshape(-1, 3, 3) if s else np.zeros((0, 3, 3))
    return _f32(np.concatenate([big, small]))


def counts(n):
    """A jittered cloud of n triangles."""
    return _cloud(np.random.default_rng(109 + n), n, (-1.0, 0.0, -1.0), (1.0, 1.0, 1.0), 0.02)


def mixed():
    """6,696 triangles.  2,600 log-spaced over 1e-6 .. 1e-3 on x; 15 single triangles, five per axis at 2e-3 x 17^k, k = 1 .. 5 (the last at
    2.8e3); and a uniform cloud of 4,081 next to them.  While an outlier is left, the log-spaced cluster and the lower outliers share one bin
    of sixteen on every axis (17 > 16), so a level takes exactly one outlier off the cluster's node: that node keeps more than kWideCount
    triangles for fifteen levels, while the cloud doubles its nodes per level past kWideTasks.  (2,600 log-spaced triangles alone lose a
    sixteenth of their span, 350 triangles, per level, and are below 2,048 after two.)"""
    rng = np.random.default_rng(110)
    x = 10.0 ** np.linspace(-6.0, -3.0, 2600)
    cl = np.zeros((2600, 3, 3)); cl[:, :, 0] = x[:, None]
    cl = cl + x[:, None, None] * rng.uniform(-0.2, 0.2, (2600, 3, 3))
    out = np.zeros((15, 3, 3))
    for a in range(3):
        for k in range(1, 6):
            out[5 * a + k - 1, :, a] = 2e-3 * 17.0 ** k
    out = out + 1e-4 * rng.uniform(-1.0, 1.0, (15, 3, 3))
    cloud = _cloud(rng, 4081, (-3000.0, 0.0, 0.0), (-1000.0, 1400.0, 1400.0), 5.0).reshape(-1, 3, 3)
    return _f32(np.concatenate([cl, out, cloud]))


CASES = {"duplicates": duplicates, "concentric": concentric, "plane_x": lambda: plane(0), "plane_y": lambda: plane(1), "plane_z": lambda: plane(2),
         "line": line, "geometric": geometric, "geometric_wide": geometric_wide, "degenerate": degenerate, "offset": offset, "mixed": mixed}
CASES.update({"big_first_%d_%d" % bs: (lambda bs=bs: big_first(*bs)) for bs in BIG_FIRST})
CASES.update({"counts_%d" % n: (lambda n=n: counts(n)) for n in COUNTS})
CASE_NAMES = tuple(CASES)
RENDER_CASES = ("duplicates", "geometric", "plane_y")
PLANE_AXIS = {"plane_x": 0, "plane_y": 1, "plane_z": 2}

_scenes = {}


def case_faces(name):
    return CASES[name]()


def case_scene(name, width=64, height=36):
    """The case as a scene in coffee's frame, materials and lights (made once per size: the tests only read it)."""
    key = (name, width, height)
    if key not in _scenes:
        _scenes[key] = MovedScene(M.HostScene("file:coffee", width, height), case_faces(name), new_faces=True)
    return _scenes[key]


def case_rays(name, n=2048, seed=5):
    """The case's ray set, [n, 8] float32 (o, d, tmin, tmax): half aimed at the box centres of random triangles (every other one from outside
    the scene's box, the others from a few triangle sizes away, so that the small triangles of a scene of many scales are met too; tmin 0),
    a quarter with uniform origins in the scene's box and uniform directions, a quarter parallel to an axis with exact zeros in the
    direction.  Half of the axis-parallel rays pass exactly through a triangle's box centre: in the plane_* cases, with the axis in the
    plane, they lie in the plane."""
    fp = case_faces(name).astype(np.float64).reshape(-1, 3, 3)
    rng = np.random.default_rng(seed)
    lo, hi = fp.min(axis=1), fp.max(axis=1)
    cen, size = 0.5 * (lo + hi), np.maximum((hi - lo).max(axis=1), 1e-30)
    slo, shi = lo.min(axis=0), hi.max(axis=0)
    diag = max(float(np.linalg.norm(shi - slo)), 1e-3)
    na, nu = n // 2, n // 4
    nx = n - na - nu

    def unit(k):
        d = rng.normal(size=(k, 3)); return d / np.linalg.norm(d, axis=1, keepdims=True)
    # aimed
    f = rng.integers(0, len(fp), na)
    d = unit(na)
    dist = np.where(np.arange(na) % 2 == 0, 2.0 * diag, 4.0 * size[f])
    aimed = make_rays(cen[f] - dist[:, None] * d, d, tmin=0.0)
    # uniform
    ext = np.maximum(shi - slo, 1e-3 * diag)
    uni = make_rays(rng.uniform(slo - 0.1 * ext, shi + 0.1 * ext, (nu, 3)), unit(nu))
    # axis-parallel
    f = rng.integers(0, len(fp), nx)
    ax = rng.integers(0, 3, nx); sgn = rng.choice([-1.0, 1.0], nx)
    d = np.zeros((nx, 3)); d[np.arange(nx), ax] = sgn
    jit = rng.uniform(-0.5, 0.5, (nx, 3)) * size[f][:, None] * (np.arange(nx) % 2)[:, None]
    dist = np.where(np.arange(nx) % 4 < 2, 2.0 * diag, 4.0 * size[f])
    org = cen[f] + jit
    org[np.arange(nx), ax] = cen[f][np.arange(nx), ax] - sgn * dist
    axial = make_rays(org, d)
    return np.ascontiguousarray(np.concatenate([aimed, uni, axial]))


def middle_split_levels(n):
    """Node counts per level when every range splits in the middle (left half (count + 1) / 2) until single triangles are left."""
    out, ranges = [], [n]
    while ranges:
        out.append(len(ranges))
        ranges = [c for r in ranges for c in ((r + 1) // 2, r // 2) if c > 1]
    return out


def tree_structure_errors(nodes, tris, prim, root, leaf_size, n_faces):
    """Is this a tree over exactly these triangles?  Plain numpy on the arrays a context or the mirror reads out: nodes [m, 32] words
    (Node128: 24 box floats, refs in words 24..27, count in word 28), tris [n, 12] words (Tri48: word 7 = prim), prim [n], root = node
    index or leaf reference.  A reference >= 0 is a node; < 0 is a leaf, ~ref = first << 3 | count - 1; 0x7ffffffe is empty.
    Counts the violations of: prim is a permutation of 0 .. n-1 and equals the records' prim word; every node is reached exactly once from
    the root; every triangle slot lies in exactly one leaf reference; every leaf count is in 1 .. leaf_size; every child reference is in
    range; a node's count equals its number of non-empty references, which come first, and the others are the empty reference.
    Returns (errors, depth in wide levels)."""
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 32); tris = np.ascontiguousarray(tris, np.uint32).reshape(-1, 12)
    prim = np.asarray(prim).reshape(-1)
    n, m = int(n_faces), len(nodes)
    bad = 0
    bad += int(len(prim) != n) + int(len(tris) != n)
    if len(prim) == n:
        bad += int(not np.array_equal(np.sort(prim), np.arange(n)))
    if len(prim) == len(tris):
        bad += int(not np.array_equal(tris[:, 7].view(np.int32), prim))
    refs = nodes[:, 24:28].view(np.int32); count = nodes[:, 28].view(np.int32)
    seen_node = np.zeros(m, np.int64); seen_tri = np.zeros(n, np.int64)
    depth = 0

    def leaf(ref):
        nonlocal bad
        first, cnt = (~ref) >> 3, ((~ref) & 7) + 1
        bad += int(not 1 <= cnt <= leaf_size)
        if first < 0 or first + cnt > n:
            bad += 1
        else:
            seen_tri[first:first + cnt] += 1

    root = int(root)
    if root == K_EMPTY_REF:
        bad += int(n != 0)
    elif root < 0:
        leaf(root)
        bad += int(m != 0)
    else:
        stack = [(root, 1)]
        while stack:
            r, d = stack.pop()
            if not 0 <= r < m:
                bad += 1; continue
            seen_node[r] += 1
            if seen_node[r] > 1:
                continue                                           # counted below; do not walk a cycle
            depth = max(depth, d)
            c = int(count[r])
            if not 2 <= c <= 4:
                bad += 1; c = max(0, min(c, 4))
            for k in range(4):
                ref = int(refs[r, k])
                if k >= c:
                    bad += int(ref != K_EMPTY_REF)
                elif ref == K_EMPTY_REF:
                    bad += 1
                elif ref >= 0:
                    stack.append((ref, d + 1))
                else:
                    leaf(ref)
    bad += int((seen_node != 1).sum()) + int((seen_tri != 1).sum())
    return bad, depth
