"""Segment queries without a GPU: the CPU mirror of the segment kernel (tests/segmentsim/segmentsim.cpp: pt_segment.h compiled for the
host, on the host mirror of the builder's tree) against the definition -- a loop over every primitive record through its distance
function -- against the point and ray mirrors where the three contracts meet, against a binary64 distance from the scenes' original
vertices, and against answers known from the geometry."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import lbvh_cases
from common import M, REPO, HostsimHandle, MovedScene
from point_helpers import pointsim
from query_helpers import SCENES, make_rays, querysim
from refit_helpers import RefitSim, moved_faces
from segment_helpers import (SEGMENT_DTYPE, exact_mesh_cases, exact_mesh_scene, crossing_slack, invalid_segments, make_segments, same_bits,
                             scene_dist64, seg_sphere_dist64, seg_tri_dist64, segment_case, segment_dist, segment_stack_depth, segmentbrute,
                             segmentsim, tri_records, valid_segments)

K = M._capi
SCENE_NAMES = [k for k, _ in SCENES]
NAMES = SCENE_NAMES + ["case:" + n for n in lbvh_cases.CASE_NAMES]
ids = lambda names: [n.replace("file:", "").replace("case:", "") for n in names]
COFFEE = "file:coffee"
# The largest |dist - dist64| / (the scene's largest extent) of the mirror on the four scenes' sets at maxDist = inf, over every row
# whose crossing slack is finite (test_against_the_binary64_distance prints them; profiles/r34_segment.txt section 3): coffee 4.5e-8,
# spheres 1.0e-7, cornell_quads 7.8e-8, random_spheres 1.6e-8.  EPS is 4 x the largest: the margin the sweep, box and point queries took over their measured values; it covers
# other seeds, not other arithmetic.
EPS = 4 * 1.0e-7

_brute = {}


def _rows(c):
    """The rows the loop over every primitive runs on: all, on coffee (168,196 primitives) every fourth."""
    n = len(c.segments)
    return np.arange(0, n, 4) if c.name == COFFEE else np.arange(n)


def _definition(c):
    if c.name not in _brute:
        rows = _rows(c)
        _brute[c.name] = segmentbrute(c.pc.sim, c.segments[rows])
        assert same_bits(segmentbrute(c.pc.sim, c.segments[rows], "any"), (_brute[c.name]["prim"] >= 0).astype(np.int32))
    return _brute[c.name]


def _not_quad(geo, prim):
    """A sphere, a triangle or a miss."""
    return (prim < geo.ns) | (prim >= geo.ns + geo.nq)


# ---- 1: the walk is the definition ----
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("leaf", [1, 4])
@pytest.mark.parametrize("name", NAMES, ids=ids(NAMES))
def test_walk_equals_the_loop_over_every_primitive(name, leaf, fmt):
    """segmentsim_query's bytes are segmentsim_brute's, whole records; "any" is prim >= 0 of closest.  Every segment of the set is
    compared on every scene but coffee: there the loop over 168,196 primitives runs on every fourth segment only (the sweeps'
    precedent), and the walk of this tree is compared with the leaf-4 walk of the 64-byte nodes on the full set besides."""
    c = segment_case(name)
    want = _definition(c)
    sim = HostsimHandle(c.pc.hs, leaf)
    try:
        got, anyone = segmentsim(sim, c.segments, "closest", fmt), segmentsim(sim, c.segments, "any", fmt)
        assert got.dtype == SEGMENT_DTYPE and anyone.dtype == np.int32
        rows = _rows(c)
        assert same_bits(got[rows], want), np.where((got[rows]["dist"] != want["dist"]) | (got[rows]["prim"] != want["prim"]))[0][:8]
        assert same_bits(anyone, (got["prim"] >= 0).astype(np.int32))
        assert same_bits(got, c.hits) and same_bits(anyone, c.anyone)
    finally:
        sim.close()


@pytest.mark.parametrize("name", NAMES, ids=ids(NAMES))
def test_segment_sets_have_hits_and_misses(name):
    """At its finite maxDist every set holds more than 100 hits and more than 100 misses, and so does each of its parts but the
    zero-length one (256 segments) by more than 50; at maxDist = inf every valid segment hits; the invalid rows are misses with their
    maxDist; no NaN comes out of a valid row; s lies in [0, 1] and dist below maxDist."""
    c = segment_case(name)
    h, ok = c.hits, valid_segments(c.segments)
    fin = c.finite()
    assert (h["prim"][fin] >= 0).sum() > 100 and (h["prim"][fin] < 0).sum() > 100
    for part, sl in c.parts.items():
        if part != "invalid":
            hf = h[c.n_base:][sl]
            least = 50 if part == "zero" else 100 if part != "pierce" else 50
            assert (hf["prim"] >= 0).sum() > least and (hf["prim"] < 0).sum() > least, (name, part, (hf["prim"] >= 0).sum(), (hf["prim"] < 0).sum())
    assert (h["prim"][:c.n_base][ok[:c.n_base]] >= 0).all()
    bad = h[~ok]
    assert len(bad) >= 40 and (bad["prim"] == -1).all() and (bad["mat"] == -1).all() and not bad["s"].any() and not bad["p"].any() and not bad["feature"].any()
    assert same_bits(bad["dist"], c.segments[~ok][:, 6])
    for f in ("dist", "s", "p"):
        assert not np.isnan(h[f][ok]).any(), f
    hit = ok & (h["prim"] >= 0)
    assert (h["s"][hit] >= 0).all() and (h["s"][hit] <= 1).all() and (h["dist"][hit] <= c.segments[hit][:, 6]).all() and (h["dist"][hit] >= 0).all()
    miss = ok & (h["prim"] < 0)
    assert same_bits(h["dist"][miss], c.segments[miss][:, 6]) and not h["s"][miss].any() and not h["p"][miss].any() and not h["feature"][miss].any()


def test_each_feature_code_occurs():
    """On coffee (a mesh and three quads): both ends, the three edges, the crossing, and the second quad triangle's edges 7 and 8.
    6 cannot occur: the quad's diagonal is the first triangle's edge 1 (feature 3) before it is the second one's edge 0, on the same
    operands."""
    c = segment_case(COFFEE)
    h = c.hits[c.hits["prim"] >= 0]
    count = np.bincount(h["feature"], minlength=9)
    assert (count[[0, 1, 2, 3, 4, 5, 7, 8]] > 0).all() and count[6] == 0 and len(count) == 9, count
    tri = h[h["prim"] >= c.geo.ns + c.geo.nq]
    assert (np.bincount(tri["feature"], minlength=6) > 20).all() and tri["feature"].max() == 5
    s = segment_case("spheres")
    sph = s.hits[(s.hits["prim"] >= 0) & (s.hits["prim"] < s.geo.ns)]
    assert (np.bincount(sph["feature"], minlength=6)[[0, 1, 2, 5]] > 0).all() and not np.isin(sph["feature"], (3, 4)).any()


# ---- 2: where the contracts meet ----
@pytest.mark.parametrize("name", NAMES, ids=ids(NAMES))
def test_zero_length_segments_are_the_point_query(name):
    """a == b: dist, prim, mat and p are pointsim's, bit for bit, and s = 0 -- on every row where neither answer is a quad (the point
    queries measure a quad by its clamped coordinates, the segment queries by its two triangles; every scene here has quads)."""
    c = segment_case(name)
    for part in (slice(0, c.n_base), slice(c.n_base, 2 * c.n_base)):
        seg, got = c.segments[part][c.parts["zero"]], c.hits[part][c.parts["zero"]]
        assert same_bits(seg[:, 0:3], seg[:, 3:6])
        want = pointsim(c.pc.sim, np.ascontiguousarray(seg[:, [0, 1, 2, 6]]))
        rows = _not_quad(c.geo, want["prim"]) & _not_quad(c.geo, got["prim"])
        # cornell_quads is quads alone: at maxDist = inf it has no row to compare bit for bit (its misses at the finite maxDist are
        # compared), and what is asserted of it here is s = 0 and the record's form.  The point queries' clamped coordinates and the two
        # triangles are different surfaces' nearest points on its sheared blocks: no bound relates the two distances.
        assert rows.sum() > 80 or name == "cornell_quads", rows.sum()
        for f in ("dist", "prim", "mat", "p"):
            assert same_bits(got[f][rows], want[f][rows]), f
        assert not got["s"].any() and (got["feature"][got["prim"] >= c.geo.ns + c.geo.nq] == 0).all()


@pytest.mark.parametrize("name", SCENE_NAMES + ["case:mixed", "case:degenerate"], ids=ids(SCENE_NAMES + ["case:mixed", "case:degenerate"]))
def test_no_further_than_the_point_queries_at_the_ends(name):
    """dist <= min(point query at a, point query at b): exactly where the point query names a triangle (its d2 is this triangle's candidate
    0 or 1), within EPS S where it names a sphere or a quad (another formula for the same distance).  any == (prim >= 0)."""
    c = segment_case(name)
    rows = np.where(valid_segments(c.segments))[0]
    s, h = c.segments[rows], c.hits[rows]
    first = c.geo.ns + c.geo.nq
    for end in (slice(0, 3), slice(3, 6)):
        pq = pointsim(c.pc.sim, np.ascontiguousarray(np.concatenate([s[:, end], s[:, 6:7]], axis=1)))
        tri = pq["prim"] >= first
        assert tri.sum() > 100 or name in ("spheres", "cornell_quads", "random_spheres")
        assert (h["prim"][tri] >= 0).all() and (h["dist"][tri] <= pq["dist"][tri]).all()
        both = (pq["prim"] >= 0) & ~tri & (h["prim"] >= 0)
        assert (h["dist"][both].astype(np.float64) <= pq["dist"][both].astype(np.float64) + EPS * c.S).all()
    assert same_bits(c.anyone, (c.hits["prim"] >= 0).astype(np.int32))


def test_a_ray_hit_is_distance_zero():
    """On coffee's mesh alone: where the closest ray query on (a, b - a, 0, 1) reports a triangle, the segment's dist is exactly 0, and
    where it reports the ray's primitive as a crossing its s is the ray's t; its primitive is the lowest id at distance 0, the ray's or
    a lower one."""
    from sign_helpers import _mesh_only
    c = segment_case(COFFEE)
    hs = _mesh_only(MovedScene(M.HostScene(COFFEE, 64, 36)))
    sim = HostsimHandle(hs, 4)
    try:
        s = c.segments[:c.n_base][valid_segments(c.segments[:c.n_base])]
        ab = (s[:, 3:6] - s[:, 0:3]).astype(np.float32)
        rays = make_rays(s[:, 0:3], ab, 0.0, 1.0)
        for fmt in (64, 128):
            ray = querysim(sim, rays, "closest", fmt)
            got = segmentsim(sim, s, "closest", fmt)
            hit = ray["prim"] >= 0
            assert hit.sum() > 256 and (~hit).sum() > 256                     # the pierce part alone crosses 256 times
            assert (got["dist"][hit] == 0).all() and (got["prim"][hit] >= 0).all()
            assert (got["feature"][hit] == 5).mean() > 0.9                       # the rest: an earlier candidate of the winner is 0 as well
            same = hit & (got["prim"] == ray["prim"]) & (got["feature"] == 5)
            assert same.sum() > 0.5 * hit.sum()
            assert same_bits(got["s"][same], ray["t"][same])
            assert (got["prim"][hit] <= ray["prim"][hit]).all()                  # the lowest id among the crossed, not the first along the ray
            assert (got["feature"][~hit] != 5).all()                            # and nothing else makes a crossing of a triangle
    finally:
        sim.close()


# ---- 3: binary64 ----
@pytest.mark.parametrize("name", SCENE_NAMES, ids=ids(SCENE_NAMES))
def test_against_the_binary64_distance(name):
    """|dist - dist64| <= EPS S + slack on every valid segment of the set at maxDist = inf (on coffee 256 of them, evenly spaced; no row is
    left out), dist64 the exact minimum over end-face, edge-edge and crossing from the caller's vertices (segment_helpers.scene_dist64).
    slack is segment_helpers.crossing_slack: 0 unless the segment comes within the triangle test's rounding noise of the winning
    primitive's plane, there noise / sin(angle) -- chosen from binary64 geometry and the primitive's id, not from the answer.  Where the
    slack exceeds the scene (a segment in the primitive's plane: the ray queries' test divides noise by noise, pt_segment.h "Not
    covered") the answer is still one of two things: the distance within EPS S, or a crossing, dist == 0 with feature 5."""
    c = segment_case(name)
    rows = np.where(valid_segments(c.segments[:c.n_base]))[0]
    if name == COFFEE:
        rows = rows[np.linspace(0, len(rows) - 1, 256).astype(np.int64)]
    s, h = c.segments[rows], c.hits[rows]
    d64 = scene_dist64(c.geo, s, h["dist"].astype(np.float64))
    err = np.abs(h["dist"].astype(np.float64) - d64) / c.S
    slack = crossing_slack(c.geo, s, h["prim"]) / c.S
    tight, loose, free = slack == 0, (slack > 0) & (slack <= 1), slack > 1
    print(name, "largest |dist - dist64| / S: %.3g over the %d rows without slack, %.3g over the %d with a finite one (their largest slack %.3g), "
          "%.3g over the %d in a primitive's plane" % (err[tight].max(), tight.sum(), err[loose].max() if loose.any() else 0, loose.sum(),
                                                     slack[loose].max() if loose.any() else 0, err[free].max() if free.any() else 0, free.sum()))
    assert (err[~free] <= EPS + slack[~free]).all(), (rows[~free][err[~free] > EPS + slack[~free]][:8], err[~free].max())
    assert ((err[free] <= EPS) | ((h["dist"][free] == 0) & (h["feature"][free] == 5))).all()


def test_per_primitive_function_against_binary64():
    """segment_dist pair by pair on random triangles and spheres of unit size: within EPS x 8 (the size of the configuration) of
    seg_tri_dist64 / seg_sphere_dist64, s and p consistent with dist."""
    rng = np.random.default_rng(41)
    n = 4096
    tri = rng.uniform(-1, 1, (n, 3, 3)).astype(np.float32)
    a, b = rng.uniform(-2, 2, (n, 3)), rng.uniform(-2, 2, (n, 3))
    s = make_segments(a, b)
    got = segment_dist("tri", tri_records(tri), s)
    want = seg_tri_dist64(s[:, 0:3], s[:, 3:6], tri)
    assert (got["prim"] == 0).all() and (np.abs(got["dist"] - want) <= EPS * 8).all(), np.abs(got["dist"] - want).max()
    assert (np.bincount(got["feature"], minlength=6) > 20).all()
    x = s[:, 0:3].astype(np.float64) + got["s"][:, None].astype(np.float64) * (s[:, 3:6].astype(np.float64) - s[:, 0:3])
    assert (np.abs(np.linalg.norm(x - got["p"], axis=1) - got["dist"]) <= EPS * 8).all()
    cen, rad = rng.uniform(-1, 1, (n, 3)).astype(np.float32), rng.uniform(0.2, 2.5, n).astype(np.float32)
    got = segment_dist("sphere", np.concatenate([cen, rad[:, None]], axis=1), s)
    want = seg_sphere_dist64(s[:, 0:3], s[:, 3:6], cen.astype(np.float64), rad.astype(np.float64))
    assert (np.abs(got["dist"] - want) <= EPS * 8).all(), np.abs(got["dist"] - want).max()
    assert (np.bincount(got["feature"], minlength=6)[[0, 1, 2, 5]] > 20).all()
    on = np.abs(np.linalg.norm(got["p"].astype(np.float64) - cen, axis=1) - rad)
    assert (on <= EPS * 8).all()


# ---- 4 and 5: exact cases, degenerate primitives, invalid rows ----
def test_exact_cases_on_one_triangle():
    """Dyadic coordinates on the triangle (0,0,0) (4,0,0) (0,4,0): every intermediate of the definition is exact and every expected record
    is known bit for bit -- a segment above the interior and parallel to it, one crossing the interior, one beside an edge, one beyond a
    vertex, one whose second end is nearest, and one touching at maxDist exactly, which is a miss because the bound is exclusive."""
    hs = exact_mesh_scene()
    names, s, want = exact_mesh_cases()
    for leaf in (1, 4):
        for fmt in (64, 128):
            got = segmentsim(hs, s, "closest", fmt, leaf)
            for k, nm in enumerate(names):
                assert same_bits(got[k:k + 1], want[k:k + 1]), (nm, got[k], want[k])
            assert same_bits(segmentsim(hs, s, "any", fmt, leaf), (want["prim"] >= 0).astype(np.int32))
    assert same_bits(segmentbrute(hs, s), want)
    one = segment_dist("tri", np.tile(tri_records(np.array([[0, 0, 0, 4, 0, 0, 0, 4, 0]], np.float32)), (len(s), 1)), s)
    for f in ("dist", "prim", "s", "p", "feature"):
        assert same_bits(one[f], want[f]), f


def test_degenerate_triangles_give_no_nan():
    """Zero-area triangles and points against random segments, zero-length ones among them: finite records, the binary64 distance."""
    rng = np.random.default_rng(29)
    n = 1024
    a = rng.uniform(-1, 1, (n, 3)); b = rng.uniform(-1, 1, (n, 3))
    w = rng.uniform(0, 1, (n, 1))
    tri = np.stack([a, b, a + w * (b - a)], axis=1)                            # collinear
    tri[n // 2:] = a[n // 2:, None, :]                                          # coincident
    tri[::7, 2] = tri[::7, 1]                                                   # two coincident vertices
    tri = tri.astype(np.float32)
    p, q = rng.uniform(-2, 2, (n, 3)), rng.uniform(-2, 2, (n, 3))
    q[::5] = p[::5]
    s = make_segments(p, q)
    got = segment_dist("tri", tri_records(tri), s)
    for f in ("dist", "s", "p"):
        assert np.isfinite(got[f]).all(), f
    assert (got["prim"] == 0).all()
    want = seg_tri_dist64(s[:, 0:3], s[:, 3:6], tri)
    assert (np.abs(got["dist"] - want) <= EPS * 8).all(), np.abs(got["dist"] - want).max()


def test_invalid_rows_are_misses():
    base = np.array([1, 1, 2, 2, 1, 2, 8, 0], np.float32)
    s = invalid_segments(base)
    tri = tri_records(np.array([[0, 0, 0, 4, 0, 0, 0, 4, 0]], np.float32))
    got = segment_dist("tri", np.tile(tri, (len(s), 1)), s)
    assert (got["prim"] == -1).all() and same_bits(got["dist"], s[:, 6])
    assert segment_dist("tri", tri, base[None])["dist"][0] == 2
    hs = exact_mesh_scene()
    for mode in ("closest", "any"):
        got = segmentsim(hs, s, mode)
        assert (got["prim"] == -1).all() if mode == "closest" else not got.any()
    pad = np.tile(base, (3, 1)); pad[:, 7] = (np.nan, np.inf, -1.0)              # the eighth float is ignored
    assert same_bits(segmentsim(hs, pad), np.tile(segmentsim(hs, base[None]), 3))


# ---- 6: after a refit ----
def test_walk_equals_loop_after_a_refit():
    c = segment_case(COFFEE)
    fp, _ = moved_faces(c.pc.hs, 0.02)
    rs = RefitSim(c.pc.hs, 4)
    try:
        rs.update(0, fp); rs.refit()
        rows = np.arange(0, len(c.segments), 8)
        want = segmentbrute(rs._sim, c.segments[rows])
        for fmt in (64, 128):
            got = segmentsim(rs._sim, c.segments, "closest", fmt)
            assert same_bits(got[rows], want)
            assert same_bits(segmentsim(rs._sim, c.segments, "any", fmt), (got["prim"] >= 0).astype(np.int32))
        assert not same_bits(got, c.hits)                         # the move changed the answer
    finally:
        rs.close()


def test_deep_walks_exceed_the_lds_part_of_the_stack():
    """What the capped-grid GPU test relies on: on coffee the set's deepest walk holds more than the 16 entries a lane keeps in LDS."""
    c = segment_case(COFFEE)
    assert segment_stack_depth(c.pc.sim, c.segments[::8]) > 16


# ---- 7: the interface and the shipped kernel ----
def test_symbols_constants_and_record():
    for name in ("moptix_query_segments_device", "moptix_query_segments"):
        assert name in K.DEVICE_SYMBOLS and hasattr(K.device_lib(), name)
    assert (K.SEGMENT_CLOSEST, K.SEGMENT_ANY) == (0, 1)
    assert M.SEGMENT_DTYPE == SEGMENT_DTYPE and M.SEGMENT_DTYPE.itemsize == C.sizeof(K.SegmentHit) == 32
    for (name, ctype), field in zip(K.SegmentHit._fields_, M.SEGMENT_DTYPE.names):
        assert name == field and getattr(K.SegmentHit, name).offset == M.SEGMENT_DTYPE.fields[field][1]
    header = open(os.path.join(REPO, "include", "moptix.h")).read()
    assert "MOPTIX_SEGMENT_CLOSEST = 0, MOPTIX_SEGMENT_ANY = 1" in header and "moptix_segment_hit;" in header


def test_segment_kernel_resources_are_pinned():
    """The shipped code object's pt_segmentquery instantiations (tools/kernel_resources.py): no spilled registers, no scratch, the point
    kernel's 32 KB of LDS, and the registers reached -- 117 for closest and 115 for any, pinned as they are, inside the 128 of four waves per SIMD
    (profiles/r34_segment.txt section 1)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from kernel_resources import kernel_resources
    res = {k: v for k, v in kernel_resources(os.path.join(REPO, "minimaloptix_amd", "lib", "libmoptix.so")).items() if "pt_segmentquery" in k}
    assert len(res) == 4, sorted(res)
    for k, v in res.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v["group_segment_fixed_size"] == 32768, (k, v)
        mode = int(re.search(r"pt_segmentqueryILi(\d)ELb[01]E", k).group(1))
        assert v["vgpr_count"] == {0: 117, 1: 115}[mode], (k, v)
