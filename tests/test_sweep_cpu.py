"""Sphere sweep queries without a GPU: the CPU mirror of the sweep kernel (tests/sweepsim/sweepsim.cpp: pt_sweep.h compiled for the host,
on the host mirror of the builder's tree) against the definition -- a loop over every primitive record through its time of contact --
against a binary64 first contact from the scenes' original vertices, against the point mirror at the centre of contact, and against
answers known from the geometry."""
import numpy as np
import pytest

import lbvh_cases
from common import HostsimHandle
from point_helpers import pointbrute, with_max
from query_helpers import SCENES
from refit_helpers import RefitSim, moved_faces
from sweep_helpers import (SWEEP_DTYPE, bracket_misses, centre32, exact_mesh_cases, exact_mesh_scene, exact_sphere_case, exact_sphere_scene,
                           invalid_sweeps, prim_dist64_at, same_bits, sweep_case, sweep_stack_depth, sweep_toi, sweepbrute, sweepsim,
                           tri_records, valid_sweeps)

SCENE_NAMES = [k for k, _ in SCENES]
NAMES = SCENE_NAMES + ["case:" + n for n in lbvh_cases.CASE_NAMES]
ids = lambda names: [n.replace("file:", "").replace("case:", "") for n in names]
COFFEE = "file:coffee"
# The smallest eps at which the mirror passes test_against_the_binary64_first_contact's two checks, measured on the four scenes' sets
# by bisection (profiles/r28_sweep.txt section 4): spheres 1.80e-8, cornell_quads 2.54e-7, random_spheres 2.47e-8, coffee 1.14e-7 -- the
# residual decides every one of them.  EPS is 4 x the largest: the margin the box and point queries took over their measured values;
# it covers other seeds, not other arithmetic.
EPS = 4 * 2.54e-7

_brute = {}


def _rows(c):
    """The rows the loop over every primitive runs on: all, on coffee (168,196 primitives) every fourth."""
    n = len(c.sweeps)
    return np.arange(0, n, 4) if c.name == COFFEE else np.arange(n)


def _definition(c):
    if c.name not in _brute:
        rows = _rows(c)
        _brute[c.name] = sweepbrute(c.pc.sim, c.sweeps[rows])
        assert same_bits(sweepbrute(c.pc.sim, c.sweeps[rows], "any"), (_brute[c.name]["prim"] >= 0).astype(np.int32))
    return _brute[c.name]


# ---- 1: the walk is the definition ----
@pytest.mark.parametrize("fmt", [64, 128])
@pytest.mark.parametrize("leaf", [1, 4, 8])
@pytest.mark.parametrize("name", NAMES, ids=ids(NAMES))
def test_walk_equals_the_loop_over_every_primitive(name, leaf, fmt):
    """sweepsim_query's bytes are sweepsim_brute's, whole buffers, no sweep excluded; "any" is prim >= 0 of closest.  On coffee the
    definition covers every fourth sweep, and the walk of this tree is compared with the leaf-4 walk of the 64-byte nodes on the full
    set besides."""
    c = sweep_case(name)
    want = _definition(c)
    sim = HostsimHandle(c.pc.hs, leaf)
    try:
        got, anyone = sweepsim(sim, c.sweeps, "closest", fmt), sweepsim(sim, c.sweeps, "any", fmt)
        assert got.dtype == SWEEP_DTYPE and anyone.dtype == np.int32
        rows = _rows(c)
        assert same_bits(got[rows], want), np.where((got[rows]["t"] != want["t"]) | (got[rows]["prim"] != want["prim"]))[0][:8]
        assert same_bits(anyone, (got["prim"] >= 0).astype(np.int32))
        assert same_bits(got, c.hits) and same_bits(anyone, c.anyone)
    finally:
        sim.close()


@pytest.mark.parametrize("name", NAMES, ids=ids(NAMES))
def test_sweep_sets_have_every_class(name):
    """Hits, misses, starts in contact, sweeps cut short by tmax, the invalid rows as misses with their tmax -- and on the four scenes
    contacts on a face interior, on an edge and at a vertex (sweep_helpers.SweepCase.check_classes).  The meshes of lbvh_cases include
    clouds of triangles far smaller than any radius of the set, where every contact is a vertex: the three contact classes are asserted
    on the scenes, and on counts_2049 and degenerate among the cases."""
    c = sweep_case(name)
    h, ok = c.hits, valid_sweeps(c.sweeps)
    assert (h["prim"][ok] >= 0).sum() > 100 and (h["prim"][ok] < 0).sum() > 100 and ((h["prim"] >= 0) & (h["t"] == 0)).sum() > 100
    bad = c.hits[~ok]
    assert len(bad) >= 30 and (bad["prim"] == -1).all() and (bad["mat"] == -1).all() and not bad["u"].any() and not bad["p"].any()
    assert same_bits(bad["t"], c.sweeps[~ok][:, 7])
    assert not np.isnan(h["t"][ok]).any() and not np.isnan(h["p"][ok]).any() and not np.isnan(h["u"][ok]).any() and not np.isnan(h["v"][ok]).any()
    hit = ok & (h["prim"] >= 0)
    assert (h["t"][hit] >= 0).all() and (h["t"][hit] <= c.sweeps[hit][:, 7]).all()
    if name in SCENE_NAMES or name in ("case:counts_2049", "case:degenerate"):
        c.check_classes()


# ---- 2: binary64 ----
@pytest.mark.parametrize("name", SCENE_NAMES, ids=ids(SCENE_NAMES))
def test_against_the_binary64_first_contact(name):
    """sweep_helpers.bracket_misses at EPS, on every valid sweep of the set (on coffee 256 of them, evenly spaced): the residual at the
    reported contact and the bracket of t between the binary64 first contacts at radius -+ EPS S."""
    c = sweep_case(name)
    rows = np.where(valid_sweeps(c.sweeps))[0]
    if name == COFFEE:
        rows = rows[np.linspace(0, len(rows) - 1, 256).astype(np.int64)]
    res, brk = bracket_misses(c.geo, c.sweeps[rows], c.hits[rows], c.S, EPS)
    assert len(res) == 0 and len(brk) == 0, (rows[res][:8], rows[brk][:8])


# ---- 3: the contact point ----
@pytest.mark.parametrize("name", [COFFEE, "case:counts_2049", "case:degenerate", "case:mixed"], ids=ids([COFFEE, "case:counts_2049", "case:degenerate", "case:mixed"]))
def test_contact_point_is_the_point_querys(name):
    """t, u, v and p of every triangle hit are the per-primitive entry's on that triangle's record alone; where the point mirror's loop
    over every primitive names the same primitive as nearest to c(t) -- it does unless another one is exactly as near -- its u, v and p
    are the record's, bit for bit; and |c(t) - p| is within EPS S of the radius at a first touch, not beyond it at a start in contact."""
    c = sweep_case(name)
    g = c.geo
    first = g.ns + g.nq
    idx = np.where(c.hits["prim"] >= first)[0]
    if name == COFFEE:
        idx = idx[::4]
    s, h = c.sweeps[idx], c.hits[idx]
    assert len(idx) > 300
    one = sweep_toi("tri", tri_records(g.tri[h["prim"] - first]), s)
    assert (one["prim"] == 0).all()
    for f in ("t", "u", "v", "p"):
        assert same_bits(one[f], h[f]), f
    q = centre32(s, h["t"])
    near = pointbrute(c.pc.sim, with_max(q))
    # The point query names the lowest id among the NEAREST primitives, the sweep the lowest id among the FIRST touched: at a start in
    # contact those differ by definition, and on a mesh a contact on a shared edge or vertex is a tie that the two roundings may break
    # differently.  Half of the first touches is what the comparison needs to mean something; every one of those is compared.
    same = near["prim"] == h["prim"]
    print(name, "the point query names the sweep's primitive on %.3f of the first touches" % same[h["t"] > 0].mean())
    assert same[h["t"] > 0].mean() > 0.5, same[h["t"] > 0].mean()
    for f in ("u", "v", "p"):
        assert same_bits(near[f][same], h[f][same]), f
    dist = np.linalg.norm(q.astype(np.float64) - h["p"].astype(np.float64), axis=1)
    r = s[:, 6].astype(np.float64)
    touch = h["t"] > 0
    assert (np.abs(dist - r)[touch] <= EPS * c.S).all() and (dist[~touch] <= r[~touch] + EPS * c.S).all()
    assert (np.abs(dist - prim_dist64_at(g, q, h["prim"])) <= EPS * c.S).all()


# ---- 4 and 5: exact cases, degenerate primitives ----
def test_exact_cases_on_a_mesh():
    """Integer coordinates, radius 2, |d| = 2: every intermediate of the definition is exact and every expected record is known bit for
    bit -- a face head-on (and of two coincident triangles the lower id), a vertex straight on, a start in contact, an end exactly at
    contact (t == tmax counts) and an ulp before it, a zero-area triangle (its edge) and three coincident vertices (the vertex)."""
    hs = exact_mesh_scene()
    names, s, want = exact_mesh_cases()
    for leaf in (1, 4):
        for fmt in (64, 128):
            got = sweepsim(hs, s, "closest", fmt, leaf)
            for k, nm in enumerate(names):
                assert same_bits(got[k:k + 1], want[k:k + 1]), (nm, got[k], want[k])
            assert same_bits(sweepsim(hs, s, "any", fmt, leaf), (want["prim"] >= 0).astype(np.int32))
    assert same_bits(sweepbrute(hs, s), want)
    assert not np.isnan(want["t"]).any()


def test_exact_sphere_primitive_head_on():
    hs, _ = exact_sphere_scene()
    s, want = exact_sphere_case(hs)
    assert same_bits(sweepsim(hs, s), want), (sweepsim(hs, s), want)
    assert same_bits(sweepbrute(hs, s), want)
    one = sweep_toi("sphere", np.array([[0, 64, 0, 2]], np.float32), s)
    assert one["t"][0] == 6 and same_bits(one["p"], want["p"])
    inside = np.array([[0, 0, 0, 0, 0, 2, 1, 16]], np.float32)             # from the centre of a sphere of radius 8: R - radius = 7 at t = 3.5
    one = sweep_toi("sphere", np.array([[0, 0, 0, 8]], np.float32), inside)
    assert one["prim"][0] == 0 and one["t"][0] == 3.5 and same_bits(one["p"][0], np.array([0, 0, 8], np.float32))


def test_degenerate_triangles_give_no_nan():
    """Zero-area triangles and points, swept at from random directions: the per-primitive entry reports finite records, and the time of
    a hit puts the centre at the radius from the segment or point (binary64)."""
    rng = np.random.default_rng(29)
    n = 512
    a = rng.uniform(-1, 1, (n, 3)); b = rng.uniform(-1, 1, (n, 3))
    w = rng.uniform(0, 1, (n, 1))
    tri = np.stack([a, b, a + w * (b - a)], axis=1)                            # collinear
    tri[n // 2:] = a[n // 2:, None, :]                                          # coincident
    tri = tri.astype(np.float32)
    target = tri.astype(np.float64).mean(axis=1)
    back = rng.normal(size=(n, 3)); back /= np.linalg.norm(back, axis=1, keepdims=True)
    o = target + back * 4.0 + rng.normal(size=(n, 3)) * 0.05
    r = 10.0 ** rng.uniform(-2, -0.5, n)
    s = np.ascontiguousarray(np.concatenate([o, -back * 2.0, r[:, None], np.full((n, 1), 8.0)], axis=1), np.float32)
    got = sweep_toi("tri", tri_records(tri), s)
    for f in ("t", "u", "v", "p"):
        assert np.isfinite(got[f]).all(), f
    hit = got["prim"] == 0
    assert hit.sum() > n // 2 and (~hit).sum() > 10
    from point_helpers import tri_dist64
    q = s[hit, 0:3].astype(np.float64) + s[hit, 3:6].astype(np.float64) * got["t"][hit, None].astype(np.float64)
    dist = tri_dist64(q, tri[hit].astype(np.float64))[0]
    assert (np.abs(dist - s[hit, 6]) <= EPS * 8.0).all()


def test_invalid_sweeps_are_misses_on_one_primitive():
    base = np.array([1, 1, 8, 0, 0, -2, 2, 16], np.float32)
    s = invalid_sweeps(base)
    got = sweep_toi("tri", np.tile(tri_records(np.array([[0, 0, 0, 4, 0, 0, 0, 4, 0]], np.float32)), (len(s), 1)), s)
    assert (got["prim"] == -1).all() and same_bits(got["t"], s[:, 7])
    assert sweep_toi("tri", tri_records(np.array([[0, 0, 0, 4, 0, 0, 0, 4, 0]], np.float32)), base[None])["t"][0] == 3


# ---- 6: after a refit ----
def test_walk_equals_loop_after_a_refit():
    c = sweep_case(COFFEE)
    fp, _ = moved_faces(c.pc.hs, 0.02)
    rs = RefitSim(c.pc.hs, 4)
    try:
        rs.update(0, fp); rs.refit()
        rows = np.arange(0, len(c.sweeps), 8)
        for fmt in (64, 128):
            got = sweepsim(rs._sim, c.sweeps, "closest", fmt)
            assert same_bits(got[rows], sweepbrute(rs._sim, c.sweeps[rows]))
            assert same_bits(sweepsim(rs._sim, c.sweeps, "any", fmt), (got["prim"] >= 0).astype(np.int32))
        assert not same_bits(got, c.hits)                         # the move changed the answer
    finally:
        rs.close()


def test_deep_walks_exceed_the_lds_part_of_the_stack():
    """What the capped-grid GPU test relies on: on coffee the set's deepest walk holds more than the 16 entries a lane keeps in LDS."""
    c = sweep_case(COFFEE)
    assert sweep_stack_depth(c.pc.sim, c.sweeps[::8]) > 16
