"""K-nearest point queries without a GPU: the CPU mirror of the K-nearest kernel (tests/pointmultisim/pointmultisim.cpp: pt_pointmulti.h compiled for
the host, on the host mirror of the builder's tree) against the definition -- a loop over every primitive record, ordered by (d2, prim) --
against the closest and "any" point queries, against a binary64 distance to every primitive, and against answers known from the geometry."""
import os
import re

import numpy as np
import pytest

from common import M, HostsimHandle, REPO, hostsim_bvh
from point_helpers import INF, Geometry, point_case, pointsim, scene_box, with_max
from pointmulti_helpers import (COUNT_ALL, KS, POINT_DTYPE, SmallCase, all_pairs_dist64, duplicates_scene, gpu_point_set, is_miss_record,
                                multi_stack_depth, pointmultibrute, pointmultikeys, pointmultisim, same_bits)
from query_helpers import SCENES
from sign_helpers import mesh_scene, spheres_and_cube
from test_point_cpu import TOL_ALL, TOL_BOX

K = M._capi
NAMES = [k for k, _ in SCENES] + ["case:" + n for n in ("duplicates", "concentric", "plane_y", "degenerate", "offset", "mixed")]
IDS = [n.replace("file:", "").replace("case:", "") for n in NAMES]
COFFEE = "file:coffee"


class Case:
    """A scene of the point tests (point_helpers.point_case) with its three query sets, and per set the definition's answer at K = 64 with
    COUNT_ALL, from which its answer at every K follows (the first K records, the count cut at K): computed once, only read afterwards.
    On coffee the loop over 168,196 primitives runs on the `special` slice plus every eighth point of the other two."""

    def __init__(self, name):
        self.name = name
        self.pc = point_case(name)
        self.sets = self.pc.sets(walked=True)              # the same bytes as sets() (test_point_cpu.py), without coffee's minute of loop
        n = len(self.pc.pts)
        a = self.pc.parts["special"].start
        self.idx = np.concatenate([np.arange(0, a, 8), np.arange(a, n)]) if name == COFFEE else np.arange(n)
        self.n_prims = self.pc.geo.ns + self.pc.geo.nq + self.pc.geo.nt
        self._brute = {}

    def rows(self, set_name, q):
        """The rows of a set the definition runs on."""
        return np.arange(len(q)) if set_name == "invalid" else self.idx

    def brute(self, set_name, k, count_all=False):
        if set_name not in self._brute:
            q = dict(self.sets)[set_name]
            self._brute[set_name] = pointmultibrute(self.pc.sim, q[self.rows(set_name, q)], 64, True)
        h, size = self._brute[set_name]
        return np.ascontiguousarray(h[:, :k]), (size if count_all else np.minimum(size, k).astype(np.int32))

    def size(self, set_name):
        """|S| per query of rows(set_name)."""
        return self.brute(set_name, 64, True)[1]


_made = {}


def case_of(name):
    if name not in _made:
        _made[name] = Case(name)
    return _made[name]


# ---- 1: the mirror is the definition ----
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("leaf", [1, 4, 8])
@pytest.mark.parametrize("name", NAMES, ids=IDS)
def test_mirror_equals_the_loop_over_every_primitive(name, leaf, fmt):
    """pointmultisim_query's bytes are pointmultisim_brute's, whole buffers: every set, K in 1, 2, 4, 8, 64 with and without COUNT_ALL, and K = 0
    with it.  On coffee the definition covers Case.idx, and the walk of this tree is compared with the leaf-4 walk of the 64-byte nodes
    on the full set besides.  One thinning, coffee alone: with COUNT_ALL and no limit the walk cannot prune anything and is itself a loop over
    all 168,196 primitives per point, so that combination runs on every 97th row of Case.idx."""
    c = case_of(name)
    sim = HostsimHandle(c.pc.hs, leaf)
    try:
        for set_name, q in c.sets:
            rows = c.rows(set_name, q)
            for k in (0,) + KS:
                for count_all in ((True,) if k == 0 else (False, True)):
                    thin = name == COFFEE and set_name == "inf" and count_all
                    sel = slice(None, None, 97) if thin else slice(None)
                    pts = q[rows[sel]] if thin else q
                    hits, counts = pointmultisim(sim, pts, k, count_all, node_format=fmt)
                    assert hits.shape == (len(pts), k) and hits.dtype == POINT_DTYPE and counts.dtype == np.int32
                    want_h, want_c = c.brute(set_name, k, count_all)
                    got_h, got_c = (hits, counts) if thin else (hits[rows], counts[rows])
                    assert same_bits(got_c, want_c[sel]), (set_name, k, count_all, np.where(got_c != want_c[sel])[0][:8])
                    assert same_bits(got_h, want_h[sel]), (set_name, k, count_all)
                    if name == COFFEE and (leaf, fmt) != (4, 64) and not thin:
                        ref_h, ref_c = pointmultisim(c.pc.sim, q, k, count_all)
                        assert same_bits(counts, ref_c) and same_bits(hits, ref_h), (set_name, k, count_all)
    finally:
        sim.close()


@pytest.mark.parametrize("name", [n for n in NAMES if n != COFFEE], ids=[i for i in IDS if i != "coffee"])
def test_the_definition_at_k_is_a_prefix_of_the_definition_at_64(name):
    """What Case.brute rests on, shown by calling the loop itself at K = 1, 4 and 0."""
    c = case_of(name)
    for set_name, q in c.sets:
        for k, count_all in ((1, False), (1, True), (4, False), (0, True)):
            h, n = pointmultibrute(c.pc.sim, q, k, count_all)
            want_h, want_n = c.brute(set_name, k, count_all)
            assert same_bits(h, want_h) and same_bits(n, want_n), (set_name, k, count_all)


# ---- 2: truncation and padding both run ----
@pytest.mark.parametrize("name", NAMES, ids=IDS)
def test_sets_truncate_and_pad(name):
    """|S| per query set.  With maxDist = inf |S| is the number of primitives for every query, so one set cannot both truncate and pad at one K;
    a scene's sets together must: at K = 4 and, where the scene has more than 64 primitives, at K = 64, some query has |S| > K and some
    0 < |S| < K.  The shortened set's even half ends at half the nearest distance: |S| = 0."""
    c = case_of(name)
    size = {s: c.size(s) for s, _ in c.sets}
    print("pointmulti |S| %-16s %s" % (name, "  ".join("%s: n=%d zero=%d 1..3=%d 4..63=%d 64+=%d max=%d" % (
        s, len(v), (v == 0).sum(), ((v > 0) & (v < 4)).sum(), ((v >= 4) & (v < 64)).sum(), (v >= 64).sum(), v.max()) for s, v in size.items())))
    assert (size["inf"] == c.n_prims).all() and not size["invalid"].any()
    assert not size["shortened"][c.rows("shortened", None) % 2 == 0].any()
    every = np.concatenate(list(size.values()))
    for k in (4, 64):
        assert ((every > 0) & (every < k)).any(), k
        assert (every > k).any() or (k == 64 and c.n_prims <= 64), k
    assert ((size["shortened"] > 0) & (size["shortened"] < 4)).sum() > 100      # padding at K = 4 on every scene's shortened set


# ---- 3: record 0 is the closest query, counts > 0 the "any" query; order, padding, prefix ----
@pytest.mark.parametrize("name", NAMES, ids=IDS)
def test_consistency_with_the_point_queries(name):
    """Record 0 is the closest query and counts > 0 the "any" query; miss records behind the count; dist never falls; K = 4 is a prefix of
    K = 64.  The order at a tie is read from the walk's own keys (pointmultikeys), not from dist: dist = sqrt(d2), and the square root
    sends neighbouring d2 to one dist, so "at equal dist bits the prim ascends" is false where two d2 one ulp apart belong to primitives in
    descending id order (10 such pairs at K = 4 on coffee's inf set).  What holds, and is asserted: the keys ascend strictly by (d2, prim),
    a record's dist is the correctly rounded sqrt of its key's d2, and at equal dist bits the prim ascends unless d2 does."""
    c = case_of(name)
    for set_name, q in c.sets:
        full, full_closest, full_any = q, pointsim(c.pc.sim, q, "closest"), pointsim(c.pc.sim, q, "any")
        full64 = pointmultisim(c.pc.sim, q, 64)
        for k in (1, 4, 64):
            for count_all in (False, True):
                # coffee without a limit under COUNT_ALL, the unpruned loop over every primitive: the thinning of test_mirror_equals_the_loop_...
                rows = c.idx[::97] if name == COFFEE and set_name == "inf" and count_all else slice(None)
                q, closest, anyone = full[rows], full_closest[rows], full_any[rows]
                h64, c64 = np.ascontiguousarray(full64[0][rows]), full64[1][rows]
                h, n = (h64, c64) if (k, count_all) == (64, False) else pointmultisim(c.pc.sim, q, k, count_all)
                assert same_bits(np.ascontiguousarray(h[:, 0]), closest), (set_name, k, count_all)
                assert np.array_equal(n > 0, anyone == 1), (set_name, k, count_all)
                kept = np.minimum(n, k)
                live = np.arange(k)[None, :] < kept[:, None]
                assert is_miss_record(h, q[:, 3])[~live].all() and (h["prim"][live] >= 0).all() and (h["mat"][live] >= 0).all()
                if k > 1:
                    both = live[:, 1:]                     # record j and j - 1 both within the count
                    d, prim = h["dist"], h["prim"]
                    assert (d[:, 1:] >= d[:, :-1])[both].all(), (set_name, k)
                    d2, kprim, kn = pointmultikeys(c.pc.sim, q, k, count_all)
                    assert np.array_equal(kn, n) and np.array_equal(kprim, prim) and same_bits(np.sqrt(d2)[live], d[live])
                    assert ((d2[:, 1:] > d2[:, :-1]) | ((d2[:, 1:] == d2[:, :-1]) & (prim[:, 1:] > prim[:, :-1])))[both].all(), (set_name, k)
                    same = both & (d[:, 1:].view(np.uint32) == d[:, :-1].view(np.uint32))
                    assert ((prim[:, 1:] > prim[:, :-1]) | (d2[:, 1:] > d2[:, :-1]))[same].all(), (set_name, k, int(same.sum()))
                if k == 4 and not count_all:
                    assert same_bits(h, np.ascontiguousarray(h64[:, :4])) and np.array_equal(n, np.minimum(c64, 4))
        if set_name == "shortened":
            assert (full64[1][0::2] == 0).all() and (full64[1][1::2] > 0).sum() > 1000


# ---- 4: exact ties ----
def test_coincident_triangles_are_consecutive_records_in_prim_order():
    """One triangle 100 times (prim = face id: the scene has nothing else): 64 records of one distance, prims 0 .. 63 in order."""
    hs = duplicates_scene()
    q = with_max(point_case("case:duplicates").pts)
    assert hs.sizes.nSpheres == 0 and hs.sizes.nQuads == 0
    for leaf in (1, 4, 8):
        sim = HostsimHandle(hs, leaf)
        try:
            for fmt in (64, 128):
                h, n = pointmultisim(sim, q, 64, True, node_format=fmt)
                assert (n == 100).all()
                assert (h["prim"] == np.arange(64)[None, :]).all()
                assert (h["dist"].view(np.uint32) == h["dist"].view(np.uint32)[:, :1]).all()
                h1, n1 = pointmultisim(sim, q, 1, False, node_format=fmt)
                assert (n1 == 1).all() and (h1["prim"] == 0).all() and same_bits(h1, np.ascontiguousarray(h[:, :1]))
                assert (pointmultisim(sim, q, 64, False, node_format=fmt)[1] == 64).all()
                assert (pointmultisim(sim, q, 0, True, node_format=fmt)[1] == 100).all()
            assert same_bits(h, pointmultibrute(sim, q, 64, True)[0])
        finally:
            sim.close()


# ---- 5: an independent binary64 computation ----
def _small(which):
    if which == "torus":
        hs = mesh_scene("torus")
        sc = SmallCase(hs, *Geometry(hs).box())
    else:
        hs = spheres_and_cube()[0]
        sc = SmallCase(hs, *scene_box(hs))
    return sc


@pytest.mark.parametrize("which", ["torus", "spheres_and_cube"])
def test_distance_ranks_against_binary64(which):
    """dist[j] against the j-th smallest of the binary64 distances from the point to EVERY primitive, and the COUNT_ALL count between the
    numbers of binary64 distances below maxDist -+ the tolerance.  If every binary32 distance is within tol of its binary64 one, so is
    every order statistic.  The tolerance is the point tests' (test_point_cpu.py).  Primitive ids are not compared: on shared vertices and
    edges several primitives are at one distance."""
    sc = _small(which)
    tol = np.minimum(TOL_BOX * sc.scale_box, TOL_ALL * sc.scale_all)
    d64 = np.sort(all_pairs_dist64(sc.geo, sc.pts), axis=1)
    n_prims = d64.shape[1]
    assert len(sc.pts) == 512 and n_prims == sc.geo.ns + sc.geo.nq + sc.geo.nt
    nearest = d64[:, 0].astype(np.float32)
    diag = np.float32(np.linalg.norm(np.ptp(sc.pts, axis=0)))
    worst, partial = 0.0, 0
    for label, md in (("inf", INF), ("2 x nearest", np.float32(2.0) * nearest), ("diag / 4", np.float32(0.25) * diag)):
        q = with_max(sc.pts, md)
        for k in (4, 64):
            h, n = pointmultisim(sc.hs, q, k, True)
            kept = np.minimum(n, k)
            live = np.arange(k)[None, :] < kept[:, None]
            kk = min(k, n_prims)
            err = np.abs(h["dist"][:, :kk].astype(np.float64) - d64[:, :kk])
            worst = max(worst, float((err / tol[:, None])[live[:, :kk]].max()) if live.any() else 0.0)
            assert (err <= tol[:, None])[live[:, :kk]].all(), (label, k, worst)
            lim = q[:, 3].astype(np.float64)[:, None]
            assert ((d64 < lim - tol[:, None]).sum(axis=1) <= n).all() and (n <= (d64 < lim + tol[:, None]).sum(axis=1)).all(), (label, k)
            assert same_bits(pointmultisim(sc.hs, q, k, False)[0], h)
        partial += int(((n > 0) & (n < n_prims)).sum())
    assert partial > 100                                   # queries whose maxDist cuts through the scene, so that the count bounds bite
    print("pointmulti64 %-18s %d points x %d primitives: worst |dist - d64| / tol %.3g" % (which, len(sc.pts), n_prims, worst))


# ---- 6: the stack ----
def test_stack_depth_on_coffee():
    """The GPU tests' points on coffee: the walk holds more than the 16 entries a lane keeps in LDS, so the kernel's overflow columns are in
    use there, and never more than the tree's bound, three pushes per level and one."""
    pc = point_case(COFFEE)
    sets = dict(pc.sets(walked=True))
    sel = gpu_point_set(pc)
    depth = hostsim_bvh(pc.sim)[4]
    for fmt in (64, 128):
        for k, count_all, q in ((1, False, sets["inf"][sel]), (64, False, sets["inf"][sel]), (4, True, sets["shortened"][sel]),
                                (0, True, sets["inf"][sel][::61])):
            d = multi_stack_depth(pc.sim, q, k, count_all, node_format=fmt)
            assert 16 < d <= 3 * depth + 1, (fmt, k, count_all, d, depth)


# ---- 7: invalid queries, the empty batch ----
def test_invalid_queries_have_empty_near_sets():
    pc = point_case(COFFEE)
    bad = dict(pc.sets(walked=True))["invalid"]
    for fmt in (64, 128):
        for count_all in (False, True):
            h, n = pointmultisim(pc.sim, bad, 4, count_all, node_format=fmt)
            assert not n.any() and is_miss_record(h, bad[:, 3]).all()      # the given maxDist's bits, NaN payload and -0 included
        assert not pointmultisim(pc.sim, bad, 0, True, node_format=fmt)[1].any()
    ok = bad[0].copy(); ok[:3] = pc.pts[pc.parts["near"].start]; ok[3] = INF
    assert pointmultisim(pc.sim, ok[None], 4)[1][0] == 4                    # +inf is "no limit", not a defect


def test_empty_batch():
    hs = M.HostScene("spheres", 64, 36)
    for count_all in (False, True):
        h, n = pointmultisim(hs, np.zeros((0, 4), np.float32), 4, count_all)
        assert h.shape == (0, 4) and len(n) == 0
    assert len(pointmultisim(hs, np.zeros((0, 4), np.float32), 0, True)[1]) == 0


# ---- 8: the surface ----
def test_symbols_and_host_side_argument_checks():
    names = {"moptix_query_points_multi", "moptix_query_points_multi_device"}
    header = open(os.path.join(REPO, "include", "moptix.h")).read()
    assert names <= set(re.findall(r"\bint (moptix_[a-z0-9_]+)\s*\(", header)) and "MOPTIX_POINT_MULTI_COUNT_ALL = 1" in header
    assert names <= set(K.DEVICE_SYMBOLS) and K.POINT_MULTI_COUNT_ALL == COUNT_ALL == 1 and K.POINT_MULTI_MAX_NEAR == 64
    lib = K.device_lib()
    assert all(hasattr(lib, n) for n in names)
    assert "query_points_multi" in dir(M.Context)
    pts, counts = np.zeros((4, 4), np.float32), np.zeros(4, np.int32)
    assert lib.moptix_query_points_multi(None, pts.ctypes.data_as(lib.moptix_query_points_multi.argtypes[1]), 4, 4, 0, None,
                                         counts.ctypes.data_as(lib.moptix_query_points_multi.argtypes[6])) == K.ERR_INVALID
    assert lib.moptix_query_points_multi_device(None, None, 0, 4, 0, None, None) == K.ERR_INVALID
    blank = object.__new__(M.Context)                                  # max_near is refused before the context is looked at
    for k, count_all in ((0, False), (-1, True), (65, False), (65, True)):
        with pytest.raises(ValueError):
            M.Context.query_points_multi(blank, pts, max_near=k, count_all=count_all)
