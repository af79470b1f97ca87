"""Ray queries without a GPU: the CPU mirror of the query kernel (tests/hostsim/querysim.cpp: pt_query.h compiled for the host, on the host mirror
of the builder's tree) against the CPU oracle's closest hits -- every ray, exactly -- and its hit attributes against the scene's own
arrays, in numpy."""
import numpy as np
import pytest

from common import M, oracle_scene
from query_helpers import SCENES, coffee_rays, invalid_rays, querysim, same_bits, scene_and_rays, shortened

K = M._capi
# moptix_hit spelled out here, apart from the package's definition, which the helpers and the other tests use
HIT_DTYPE = np.dtype([("t", np.float32), ("prim", np.int32), ("mat", np.int32), ("u", np.float32), ("v", np.float32), ("ng", np.float32, (3,))])


@pytest.fixture(scope="module", params=SCENES, ids=[s[0].replace("file:", "") for s in SCENES])
def case(request):
    kind, iarg = request.param
    hs, rays = scene_and_rays(kind, iarg)
    op, ot = oracle_scene(hs).closest_hits(rays)
    return hs, rays, op, ot


def test_package_exports_the_hit_record():
    assert M.HIT_DTYPE == HIT_DTYPE and M.HIT_DTYPE.itemsize == 32
    assert {"moptix_query_rays", "moptix_query_rays_device"} <= set(K.DEVICE_SYMBOLS)
    lib = K.device_lib()
    assert hasattr(lib, "moptix_query_rays") and hasattr(lib, "moptix_query_rays_device")
    assert "query_rays" in dir(M.Context)


def test_closest_equals_oracle(case):
    hs, rays, op, ot = case
    h = querysim(hs, rays, "closest")
    hit = op >= 0
    if hs.kind == "file:coffee":
        assert len(rays) == 4096 and hit.sum() > 1000 and (~hit).sum() > 100
    else:
        assert len(rays) == 2048 and hit.sum() > 100
    assert np.array_equal(h["prim"], op)
    assert np.array_equal(h["t"][hit], ot[hit])
    # a miss: t = tmax, ids -1, everything else 0
    miss = h[~hit]
    assert np.array_equal(miss["t"], rays[~hit, 7]) and (miss["mat"] == -1).all()
    assert not miss["u"].any() and not miss["v"].any() and not miss["ng"].any()


def test_closest_equals_brute_force_oracle(case):
    hs, rays, op, ot = case
    sub = rays[::8]
    bp, bt = oracle_scene(hs, brute_force_tris=True).closest_hits(sub)
    h = querysim(hs, sub, "closest")
    assert np.array_equal(h["prim"], bp) and np.array_equal(h["t"][bp >= 0], bt[bp >= 0])


def test_any_equals_oracle(case):
    hs, rays, op, ot = case
    assert np.array_equal(querysim(hs, rays, "any"), (op >= 0).astype(np.int32))
    short = shortened(rays, ot, op)
    sp, st = oracle_scene(hs).closest_hits(short)
    hit, even = op >= 0, np.arange(len(rays)) % 2 == 0
    assert (sp[hit & even] == -1).all() and np.array_equal(sp[hit & ~even], op[hit & ~even])      # cut short of the hit / well behind it
    assert np.array_equal(querysim(hs, short, "any"), (sp >= 0).astype(np.int32))
    assert np.array_equal(querysim(hs, short, "closest")["prim"], sp)


def test_any_is_closest_hit_or_not(case):
    hs, rays, op, ot = case
    for fmt in (64, 128):
        assert np.array_equal(querysim(hs, rays, "any", node_format=fmt), (querysim(hs, rays, "closest", node_format=fmt)["prim"] >= 0).astype(np.int32))


def test_node_formats_give_identical_bits(case):
    hs, rays, op, ot = case
    assert same_bits(querysim(hs, rays, "closest", node_format=64), querysim(hs, rays, "closest", node_format=128))
    assert same_bits(querysim(hs, rays, "any", node_format=64), querysim(hs, rays, "any", node_format=128))


def test_attributes_against_the_scene_arrays(case):
    hs, rays, op, ot = case
    h = querysim(hs, rays, "closest")
    f = hs.flat()
    ns, nq = hs.sizes.nSpheres, hs.sizes.nQuads
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    p = o + h["t"].astype(np.float64)[:, None] * d
    ng = h["ng"].astype(np.float64)
    prim = h["prim"]
    tri = prim >= ns + nq; sph = (prim >= 0) & (prim < ns); quad = (prim >= ns) & (prim < ns + nq)
    assert tri.sum() + sph.sum() + quad.sum() == (prim >= 0).sum() > 0

    def parallel(a, b):
        c = np.abs((a * b).sum(axis=1)) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        return (c >= 1 - 1e-5).all()

    if tri.any():
        face_pos, _, _, face_mat = hs.face_arrays()
        fid = prim[tri] - ns - nq
        p0, p1, p2 = (face_pos[fid, 3 * k:3 * k + 3].astype(np.float64) for k in range(3))
        u, v = h["u"][tri].astype(np.float64), h["v"][tri].astype(np.float64)
        assert (u >= 0).all() and (v >= 0).all() and (u + v <= 1 + 1e-5).all()
        q = p0 + u[:, None] * (p1 - p0) + v[:, None] * (p2 - p0)
        assert (np.linalg.norm(q - p[tri], axis=1) <= 1e-4 * (1 + np.linalg.norm(p[tri], axis=1))).all()
        assert parallel(ng[tri], np.cross(p1 - p0, p2 - p0))
        assert np.array_equal(h["mat"][tri], np.asarray(face_mat)[fid])
    if sph.any():
        c = np.array([[s.center.x, s.center.y, s.center.z] for s in (f["spheres"][i] for i in prim[sph])], np.float64)
        assert parallel(ng[sph], p[sph] - c)
        assert np.array_equal(h["mat"][sph], np.asarray(f["sphereMat"])[prim[sph]])
        assert not h["u"][sph].any() and not h["v"][sph].any()
    if quad.any():
        qi = prim[quad] - ns
        n = np.array([[q.plane.x, q.plane.y, q.plane.z] for q in (f["quads"][i] for i in qi)], np.float64)
        assert parallel(ng[quad], n)
        assert np.array_equal(h["mat"][quad], np.asarray(f["quadMat"])[qi])
        assert not h["u"][quad].any() and not h["v"][quad].any()


def test_invalid_rays_are_misses():
    hs = M.HostScene("file:coffee", 64, 36)
    bad, base = invalid_rays()
    good = querysim(hs, base[None, :], "closest")
    assert good["prim"][0] >= 0 and querysim(hs, base[None, :], "any")[0] == 1      # the ray every defect is planted in does hit
    for fmt in (64, 128):
        h = querysim(hs, bad, "closest", node_format=fmt)
        assert (h["prim"] == -1).all() and (h["mat"] == -1).all()
        assert h["t"].tobytes() == bad[:, 7].tobytes()                               # t = the caller's tmax, whatever it is
        assert not h["u"].any() and not h["v"].any() and not h["ng"].any()
        assert not querysim(hs, bad, "any", node_format=fmt).any()


def test_negative_tmin_is_walked_as_zero(case):
    hs, rays, op, ot = case
    neg = rays.copy(); neg[:, 6] = -1.0
    zero = rays.copy(); zero[:, 6] = 0.0
    minus0 = rays.copy(); minus0[:, 6] = -0.0
    for mode in ("closest", "any"):
        want = querysim(hs, zero, mode)
        assert same_bits(querysim(hs, neg, mode), want) and same_bits(querysim(hs, minus0, mode), want)
    zp, zt = oracle_scene(hs).closest_hits(zero)
    h = querysim(hs, neg, "closest")
    assert np.array_equal(h["prim"], zp) and np.array_equal(h["t"][zp >= 0], zt[zp >= 0]) and (h["t"][zp >= 0] > 0).all()


def test_empty_batch():
    hs = M.HostScene("spheres", 64, 36)
    assert len(querysim(hs, np.zeros((0, 8), np.float32), "closest")) == 0
    assert len(querysim(hs, np.zeros((0, 8), np.float32), "any")) == 0
