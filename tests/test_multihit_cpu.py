"""Multi-hit ray queries without a GPU: the CPU mirror of the multi-hit kernel (tests/hostsim/multihitsim.cpp: pt_multihit.h compiled for the
host, on the host mirror of the builder's tree) against the definition -- a loop over every primitive record, sorted by (t, prim) -- against
the closest and occlusion queries, against a chain of the oracle's closest hits, and against answers known from the geometry."""
import os
import re

import numpy as np
import pytest

from common import M, HostsimHandle, MovedScene, REPO, oracle_scene
from lbvh_cases import case_faces
from multihit_helpers import COUNT_ALL, HIT_DTYPE, KS, axis_rays, is_miss_record, multibrute, multisim, same_bits, scene_and_rays
from query_helpers import SCENES, invalid_rays, querysim
from sign_helpers import CLOSED_OUTWARD, _mesh_only, sign_case, signsim

K = M._capi


class Case:
    """A scene of query_helpers.SCENES with its ray set, built once; the definition's answer at K = 64 with and without COUNT_ALL, and the
    mirror's answers as the tests ask for them -- each computed once and only read afterwards."""

    def __init__(self, kind, iarg):
        self.kind = kind
        self.hs, self.rays = scene_and_rays(kind, iarg)
        self.sim = HostsimHandle(self.hs, 4)
        self.brute64 = {a: multibrute(self.sim, self.rays, 64, a) for a in (False, True)}
        self.size = self.brute64[True][1]                  # |H| per ray
        self._mirror = {}

    def mirror(self, k, count_all=False, fmt=64):
        key = (k, count_all, fmt)
        if key not in self._mirror:
            self._mirror[key] = multisim(self.sim, self.rays, k, count_all, node_format=fmt)
        return self._mirror[key]

    def brute(self, k, count_all=False):
        """The definition's answer at K = k from its answer at 64: the first k records and the count cut at k."""
        h, c = self.brute64[count_all]
        return np.ascontiguousarray(h[:, :k]), (c if count_all else np.minimum(c, k).astype(np.int32))


@pytest.fixture(scope="module", params=SCENES, ids=[s[0].replace("file:", "") for s in SCENES])
def case(request):
    return Case(*request.param)


def faces_scene(fp):
    """The faces alone in coffee's frame, materials and lights, without coffee's quads: prim = face id."""
    return _mesh_only(MovedScene(M.HostScene("file:coffee", 64, 36), fp, new_faces=True))


# ---- 1: the mirror is the definition ----
def test_mirror_equals_the_loop_over_every_primitive(case):
    n = len(case.rays)
    assert n == (4096 if case.kind == "file:coffee" else 2048)
    assert (case.size <= 64).all()                         # so the answer at 64 holds all of H, and brute() is the definition at every K
    truncated = padded = False
    for k in KS:
        truncated |= bool((case.size > k).any()); padded |= bool(((case.size > 0) & (case.size < k)).any())
        for count_all in (False, True):
            want = multibrute(case.sim, case.rays, k, count_all) if k in (1, 64) else case.brute(k, count_all)
            if k == 1:
                assert same_bits(want[0], case.brute(1, count_all)[0]) and same_bits(want[1], case.brute(1, count_all)[1])      # brute() cuts rightly
            for fmt in (64, 128):
                hits, counts = case.mirror(k, count_all, fmt)
                assert hits.shape == (n, k) and hits.dtype == HIT_DTYPE
                assert same_bits(counts, want[1]), (k, count_all, fmt, np.where(counts != want[1])[0][:8])
                assert same_bits(hits, want[0]), (k, count_all, fmt)
    assert truncated and padded


# ---- 2: record 0 is the closest query, counts > 0 the occlusion query ----
def test_record_0_is_the_closest_query(case):
    for fmt in (64, 128):
        closest, occluded = querysim(case.sim, case.rays, "closest", node_format=fmt), querysim(case.sim, case.rays, "any", node_format=fmt)
        assert (occluded == 1).sum() > 100
        for k in (1, 4, 64):
            for count_all in (False, True):
                hits, counts = case.mirror(k, count_all, fmt)
                assert same_bits(np.ascontiguousarray(hits[:, 0]), closest), (k, count_all, fmt)
                assert np.array_equal(counts > 0, occluded == 1)


# ---- 3: order and prefix ----
def test_records_ascend_and_smaller_k_is_a_prefix(case):
    h8, c8 = case.mirror(8)
    n = len(case.rays)
    for k in (8, 64):
        h, c = case.mirror(k)
        t, prim = h["t"], h["prim"]
        live = np.arange(k)[None, 1:] < c[:, None]         # record j and j - 1 both within the count
        up = (t[:, 1:] > t[:, :-1]) | ((t[:, 1:] == t[:, :-1]) & (prim[:, 1:] > prim[:, :-1]))
        two_roots = (t[:, 1:] > t[:, :-1]) & (prim[:, 1:] == prim[:, :-1])      # the same prim twice: a sphere, at two different t
        assert (up | ~live).all() and live.sum() > 0
        assert (prim[:, 1:][two_roots & live] < case.hs.sizes.nSpheres).all()
        assert is_miss_record(h, case.rays[:, 7])[np.arange(k)[None, :] >= c[:, None]].all()
        assert (prim[np.arange(k)[None, :] < c[:, None]] >= 0).all()
    for small, big in ((2, 8), (4, 8), (8, 64), (64, 64)):
        hs_, cs = case.mirror(small)
        hb, cb = case.mirror(big)
        assert same_bits(hs_, np.ascontiguousarray(hb[:, :small])) and np.array_equal(cs, np.minimum(cb, small))
    for k in KS:
        h, c = case.mirror(k)
        ha, ca = case.mirror(k, True)
        assert same_bits(h, ha) and (ca >= c).all() and np.array_equal(np.minimum(ca, k), c)
    assert len(c8) == n


# ---- 4: a chain of the oracle's closest hits ----
def test_each_record_is_the_oracles_next_closest_hit(case):
    h, c = case.mirror(8)
    osc = oracle_scene(case.hs)
    checked = 0
    for j in range(7):
        rows = np.where(c > j + 1)[0]
        if not len(rows):
            continue
        later = h["t"][rows, j + 1:] > h["t"][rows, j][:, None]
        later &= (np.arange(j + 1, 8)[None, :] < c[rows, None])
        has = later.any(axis=1)
        rows, m = rows[has], j + 1 + later[has].argmax(axis=1)      # the first later record with a larger t
        chain = case.rays[rows].copy(); chain[:, 6] = h["t"][rows, j]
        op, ot = osc.closest_hits(chain)
        assert np.array_equal(op, h["prim"][rows, m]), j
        assert ot.astype(np.float32).tobytes() == h["t"][rows, m].tobytes(), j
        checked += len(rows)
    assert checked > 50


# ---- 5: exact ties ----
def test_coincident_triangles_are_consecutive_records_in_prim_order():
    sim = HostsimHandle(faces_scene(case_faces("duplicates")), 4)      # one triangle 100 times
    rays = axis_rays([[0.0, 0.1, 1.0], [0.1, 0.0, 1.0], [0.0, 0.1, -2.0], [5.0, 0.1, 1.0]], 2, -1.0)
    rays[2, 5] = 1.0                                                   # from behind, along +z
    for fmt in (64, 128):
        h, c = multisim(sim, rays, 64, True, node_format=fmt)
        assert c.tolist() == [100, 100, 100, 0]
        for i in range(3):
            assert (h["t"][i] == h["t"][i, 0]).all() and np.array_equal(h["prim"][i], np.arange(64))
        assert is_miss_record(h[3:], rays[3:, 7]).all()
        h8, c8 = multisim(sim, rays, 8, False, node_format=fmt)
        assert c8.tolist() == [8, 8, 8, 0] and same_bits(h8, np.ascontiguousarray(h[:, :8]))
        assert same_bits(h, multibrute(sim, rays, 64, True)[0])


def test_concentric_layers_are_all_counted_in_order():
    fp = case_faces("concentric")                                      # 300 similar triangles about the origin, each over (x, y) = (0, 0)
    sim = HostsimHandle(faces_scene(fp), 4)
    z0 = fp.reshape(-1, 3, 3).astype(np.float64)
    rays = axis_rays([[0.0, 0.0, 5.0], [0.0, 0.0, -5.0]], 2, -1.0)
    rays[1, 5] = 1.0
    # the layer the z axis meets in triangle i: z at (0, 0) of its plane, from the vertices in binary64; 300 different heights
    n = np.cross(z0[:, 1] - z0[:, 0], z0[:, 2] - z0[:, 0])
    zc = (n * z0[:, 0]).sum(axis=1) / n[:, 2]
    assert len(np.unique(zc)) == 300
    for fmt in (64, 128):
        for r, order in ((0, np.argsort(-zc)), (1, np.argsort(zc))):
            h, c = multisim(sim, rays[r:r + 1], 64, True, node_format=fmt)
            assert c[0] == 300
            assert np.array_equal(h["prim"][0], order[:64]) and (np.diff(h["t"][0]) > 0).all()
        assert multisim(sim, rays, 0, True, node_format=fmt)[1].tolist() == [300, 300]
        assert multisim(sim, rays, 64, False, node_format=fmt)[1].tolist() == [64, 64]


def test_coplanar_overlapping_triangles_all_count():
    fp = case_faces("plane_y")                                         # a grid of overlapping triangles in the plane y = 0.0625
    sim = HostsimHandle(faces_scene(fp), 4)
    t = fp.reshape(-1, 3, 3).astype(np.float64)[:, :, [0, 2]]
    g = np.stack(np.meshgrid(np.linspace(-1.9, 1.9, 24), np.linspace(-3.9, 0.2, 24), indexing="ij"), axis=-1).reshape(-1, 2)
    # barycentrics of every point in every triangle's (x, z) projection, binary64; keep the points that are well off every edge
    a, e1, e2 = t[None, :, 0], t[None, :, 1] - t[None, :, 0], t[None, :, 2] - t[None, :, 0]
    det = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
    d = g[:, None, :] - a
    u = (d[..., 0] * e2[..., 1] - d[..., 1] * e2[..., 0]) / det
    v = (e1[..., 0] * d[..., 1] - e1[..., 1] * d[..., 0]) / det
    edge = np.minimum(np.minimum(u, v), 1.0 - u - v)
    clear = (np.abs(edge) > 1e-3).all(axis=1)
    layers = (edge > 0).sum(axis=1)[clear]
    assert clear.sum() > 300 and layers.max() >= 2 and (layers == 0).sum() < clear.sum()
    org = np.stack([g[clear, 0], np.full(clear.sum(), 1.0), g[clear, 1]], axis=1)
    rays = axis_rays(org, 1, -1.0)
    for fmt in (64, 128):
        h, c = multisim(sim, rays, 8, True, node_format=fmt)
        assert np.array_equal(c, layers)
        for i in np.where(layers >= 2)[0][:50]:
            k = layers[i]
            key = list(zip(h["t"][i, :k].tolist(), h["prim"][i, :k].tolist()))
            assert key == sorted(key) and len(set(key)) == k and abs(h["t"][i, 0] - 0.9375) < 1e-5 and abs(h["t"][i, k - 1] - 0.9375) < 1e-5


# ---- 6: analytic known answers ----
def test_spheres_known_answers():
    hs = M.HostScene("spheres", 64, 36)                                # three spheres of radius 0.5 at z = -1, x = 0, 1, -1: they touch
    rays = np.array([[0, 0, 1, 0, 0, -1, 0, 1e27],                     # through sphere 0 from outside
                     [0, 0, -1, 0, 0, -1, 0, 1e27],                    # from its centre
                     [-3, 0, -1, 1, 0, 0, 0, 1e27],                    # through all three along x: the exit of one is the entry of the next
                     [0.5, 0, 1, 0, 0, -1, 0, 1e27]], np.float32)      # tangent to spheres 0 and 1 where they touch
    for fmt in (64, 128):
        h, c = multisim(hs, rays, 8, True, node_format=fmt)
        assert c.tolist() == [2, 1, 6, 2]
        assert h["prim"][0, :2].tolist() == [0, 0] and h["t"][0, :2].tolist() == [1.5, 2.5]
        assert h["ng"][0, 0].tolist() == [0, 0, 1] and h["ng"][0, 1].tolist() == [0, 0, -1]      # the exit's normal points along the ray
        assert h["prim"][1, 0] == 0 and h["t"][1, 0] == 0.5 and h["ng"][1, 0].tolist() == [0, 0, -1]
        assert list(zip(h["t"][2, :6].tolist(), h["prim"][2, :6].tolist())) == [(1.5, 2), (2.5, 0), (2.5, 2), (3.5, 0), (3.5, 1), (4.5, 1)]
        assert list(zip(h["t"][3, :2].tolist(), h["prim"][3, :2].tolist())) == [(2.0, 0), (2.0, 1)]      # t1 == t2: one pair per sphere
        assert (h["mat"][np.arange(8)[None, :] < c[:, None]] >= 0).all()
        assert is_miss_record(h, rays[:, 7])[np.arange(8)[None, :] >= c[:, None]].all()


def test_cornell_box_known_answers():
    hs = M.HostScene("cornell_quads", 64, 36)      # the box 0 .. 555: floor 0, ceiling 1, back wall 2, walls x = 555 and x = 0 (3, 4), light 5 at y = 554, short box top 6 at y = 165
    rays = np.array([[278, -10, 250, 0, 1, 0, 0, 1e27],                # up, beside both boxes, under the light: floor, light, ceiling
                     [-10, 400, 100, 1, 0, 0, 0, 1e27],                # across, above the boxes: the two side walls
                     [278, 400, -10, 0, 0, 1, 0, 1e27],                # in through the open front: the back wall
                     [186, 600, 169, 0, -1, 0, 0, 1e27],               # down through the short box: ceiling, its top, floor
                     [278, -10, 250, 0, 1, 0, 0, 500]], np.float32)    # the first ray, cut below the light
    h, c = multisim(hs, rays, 4, True)
    assert c.tolist() == [3, 2, 1, 3, 1]
    assert h["prim"][0, :3].tolist() == [0, 5, 1] and h["t"][0, :3].tolist() == [10, 564, 565]
    assert h["prim"][1, :2].tolist() == [4, 3] and h["t"][1, :2].tolist() == [10, 565]
    assert h["prim"][2, 0] == 2 and h["t"][2, 0] == 565
    assert h["prim"][3, :3].tolist() == [1, 6, 0] and h["t"][3, :3].tolist() == [45, 435, 600]
    assert h["prim"][4].tolist() == [0, -1, -1, -1] and h["t"][4].tolist() == [10, 500, 500, 500]


# ---- 7: parity as an inside test ----
@pytest.mark.parametrize("name", CLOSED_OUTWARD)
def test_crossing_parity_is_the_sign(name):
    """A fixed point set (the uniform and the near-surface points of the sign tests) with a fixed direction per point: a point is inside a
    closed mesh exactly when its ray crosses the surface an odd number of times.  The definition's loop satisfies that on this set, and
    the mirror gives the loop's counts."""
    sc = sign_case(name)
    pts = sc.pts[:2048]
    d = np.random.default_rng(21).normal(size=(len(pts), 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays = np.ascontiguousarray(np.concatenate([pts, d, np.zeros((len(pts), 1), np.float32), np.full((len(pts), 1), 1e27, np.float32)], axis=1))
    inside = signsim(sc.sim, sc.q[:2048])["dist"] < 0
    assert 50 < inside.sum() < len(pts) - 50
    brute = multibrute(sc.sim, rays, 0, True)[1]
    assert np.array_equal(brute & 1, inside.astype(np.int32))
    for fmt in (64, 128):
        assert np.array_equal(multisim(sc.sim, rays, 0, True, node_format=fmt)[1], brute)
        assert np.array_equal(multisim(sc.sim, rays, 4, True, node_format=fmt)[1], brute)


# ---- 8, 9, 10: invalid rays, negative tmin, the empty batch ----
def test_invalid_rays_have_no_hits():
    hs = M.HostScene("file:coffee", 64, 36)
    sim = HostsimHandle(hs, 4)
    bad, base = invalid_rays()
    assert multisim(sim, base[None, :], 4)[1][0] > 0                   # the ray every defect is planted in does hit
    for fmt in (64, 128):
        for count_all in (False, True):
            h, c = multisim(sim, bad, 4, count_all, node_format=fmt)
            assert not c.any() and is_miss_record(h, bad[:, 7]).all()
            assert same_bits(h, multibrute(sim, bad, 4, count_all)[0])
        assert not multisim(sim, bad, 0, True, node_format=fmt)[1].any()


def test_negative_tmin_is_walked_as_zero(case):
    neg = case.rays.copy(); neg[:, 6] = -1.0
    zero = case.rays.copy(); zero[:, 6] = 0.0
    minus0 = case.rays.copy(); minus0[:, 6] = -0.0
    for count_all in (False, True):
        want = multisim(case.sim, zero, 4, count_all)
        for r in (neg, minus0):
            got = multisim(case.sim, r, 4, count_all)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        assert (want[0]["t"][np.arange(4)[None, :] < np.minimum(want[1], 4)[:, None]] > 0).all()
    assert same_bits(want[0], multibrute(case.sim, neg, 4, True)[0])


def test_empty_batch():
    hs = M.HostScene("spheres", 64, 36)
    for count_all in (False, True):
        h, c = multisim(hs, np.zeros((0, 8), np.float32), 4, count_all)
        assert h.shape == (0, 4) and len(c) == 0
    assert len(multisim(hs, np.zeros((0, 8), np.float32), 0, True)[1]) == 0


# ---- 11: the surface ----
def test_symbols_and_host_side_argument_checks():
    names = {"moptix_query_rays_multi", "moptix_query_rays_multi_device"}
    header = open(os.path.join(REPO, "include", "moptix.h")).read()
    assert names <= set(re.findall(r"\bint (moptix_[a-z0-9_]+)\s*\(", header)) and "MOPTIX_MULTI_COUNT_ALL = 1" in header
    assert names <= set(K.DEVICE_SYMBOLS) and K.MULTI_COUNT_ALL == COUNT_ALL == 1
    lib = K.device_lib()
    assert all(hasattr(lib, n) for n in names)
    assert "query_rays_multi" in dir(M.Context)
    rays, counts = np.zeros((4, 8), np.float32), np.zeros(4, np.int32)
    assert lib.moptix_query_rays_multi(None, rays.ctypes.data_as(lib.moptix_query_rays_multi.argtypes[1]), 4, 4, 0, None,
                                       counts.ctypes.data_as(lib.moptix_query_rays_multi.argtypes[6])) == K.ERR_INVALID
    assert lib.moptix_query_rays_multi_device(None, None, 0, 4, 0, None, None) == K.ERR_INVALID
    blank = object.__new__(M.Context)                                  # max_hits is refused before the context is looked at
    for k, count_all in ((0, False), (-1, True), (65, False), (65, True)):
        with pytest.raises(ValueError):
            M.Context.query_rays_multi(blank, rays, max_hits=k, count_all=count_all)
