"""The material cases (tests/material_cases.py) on the CPU: the mirror's three Disney functions against the oracle's, one call at a time,
and both against a binary64 restatement of the formulas written here; every case's render, per-ray and packet state machine, against the
oracle's; radiance along grazing rays against the oracle's recursive tracer.  What the GPU tests then compare the device with.

The lines that start with "material_cases:" are the measurements profiles/r25_material_cases.txt records (pytest -s shows them)."""
import ctypes as C

import numpy as np
import pytest

import material_cases as MC
from common import K, HostsimHandle, hostsim_lib, hostsim_render, oracle_scene, rmse
from oracle import oracle as O
from radiance_helpers import radiancesim

RMSE_TIGHT = 2e-6
SEEDS = MC.M.launch_seeds(4)
W, H = 96, 54
F32 = np.float32


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------

def _norm32(v):
    """Unit vectors in binary32, normalised in binary32."""
    v = np.asarray(v, F32)
    return (v / np.sqrt((v * v).sum(axis=1, dtype=F32), dtype=F32)[:, None]).astype(F32)


def _frame(rng, n):
    """n unit normals and two unit tangents each (binary64)."""
    nn = rng.normal(size=(n, 3)); nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    t = np.cross(nn, rng.normal(size=(n, 3))); t /= np.linalg.norm(t, axis=1, keepdims=True)
    return nn, t, np.cross(nn, t)


def _at(frame, sin_el, phi):
    """The direction `sin_el` above the tangent plane of the frame at azimuth phi."""
    nn, t, b = frame
    c = np.sqrt(1.0 - sin_el * sin_el)
    return nn * np.asarray(sin_el)[:, None] + (t * np.cos(phi)[:, None] + b * np.sin(phi)[:, None]) * np.asarray(c)[:, None]


SMALL = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6)


def directions(rng, n_random, n_small):
    """(N, V, L, H) float32 [n, 3], unit in binary32: n_random with V and L uniform over N's hemisphere; for each size s in SMALL,
    n_small each with N.L = s, with N.V = s, with L opposite V at that elevation (L.H = s, H next to N); all with H = normalize(L + V) as a
    path makes it -- and n_small mirror directions L = reflect(-V, N) with H = N exactly."""
    sets = []

    def add(frame, v, l, h=None):
        nn = _norm32(frame[0]); v = _norm32(v); l = _norm32(l)
        sets.append((nn, v, l, _norm32(l + v) if h is None else h))
    f = _frame(rng, n_random)
    add(f, _at(f, rng.uniform(0, 1, n_random), rng.uniform(0, 2 * np.pi, n_random)), _at(f, rng.uniform(0, 1, n_random), rng.uniform(0, 2 * np.pi, n_random)))
    for s in SMALL:
        k = n_small
        small = np.full(k, s)
        f = _frame(rng, k)
        add(f, _at(f, rng.uniform(0.05, 1, k), rng.uniform(0, 2 * np.pi, k)), _at(f, small, rng.uniform(0, 2 * np.pi, k)))      # N.L
        f = _frame(rng, k)
        add(f, _at(f, small, rng.uniform(0, 2 * np.pi, k)), _at(f, rng.uniform(0.05, 1, k), rng.uniform(0, 2 * np.pi, k)))      # N.V
        f = _frame(rng, k)
        phi = rng.uniform(0, 2 * np.pi, k)
        add(f, _at(f, small, phi), _at(f, small, phi + np.pi))                                                                    # L.H
    f = _frame(rng, n_small)
    v = _at(f, rng.uniform(0.05, 1, n_small), rng.uniform(0, 2 * np.pi, n_small))
    nn = _norm32(f[0]).astype(np.float64)
    add(f, v, 2.0 * (nn * v).sum(axis=1, keepdims=True) * nn - v, h=_norm32(f[0]))
    return tuple(np.ascontiguousarray(np.concatenate([s[i] for s in sets])) for i in range(4))


def _disney_record(m):
    """A dict of material_cases (every key) as the C ABI's material record."""
    km = K.Material()
    km.kind = K.MAT_DISNEY
    km.disney.color = K.Float3(*m["color"])
    for k in MC.PARAMS:
        setattr(km.disney, k, m[k])
    km.disney.brdfType = int(m.get("brdf", 0))
    return km


def _orc_record(km):
    """The oracle's record of a Disney material record."""
    om = O.OrcMaterial()
    om.kind = O.ORC_DISNEY
    d = km.disney
    om.color = O.f3(d.color.x, d.color.y, d.color.z)
    for k in MC.PARAMS:
        setattr(om, k, getattr(d, k))
    om.brdfType, om.refIdx = int(d.brdfType), 1.0
    return om


def _materials():
    """(label, record): every Disney material of every case as its scene holds it, then 300 vectors uniform in [0, 1]^10 with colours
    uniform in [0, 1]^3."""
    out = []
    for name in MC.CASE_NAMES:
        hs = MC.case_scene(name, W, H)
        want = MC.case_materials(name)
        recs = [MC.scene_material(hs, i) for i in range(hs.sizes.nMaterials)]
        recs = [r for r in recs if r.kind == K.MAT_DISNEY]
        assert len(recs) == len(want), name
        for i, (r, m) in enumerate(zip(recs, want)):      # the scene file said what the case says
            assert [F32(getattr(r.disney, k)) for k in MC.PARAMS] == [F32(m[k]) for k in MC.PARAMS] and r.disney.brdfType == m["brdf"], (name, i)
            assert (F32(r.disney.color.x), F32(r.disney.color.y), F32(r.disney.color.z)) == tuple(F32(c) for c in m["color"]), (name, i)
            out.append(("%s/%d" % (name, i), r))
    rng = np.random.default_rng(2024)
    for i in range(300):
        m = dict(zip(MC.PARAMS, rng.uniform(0.0, 1.0, len(MC.PARAMS)).tolist()), color=tuple(rng.uniform(0.0, 1.0, 3).tolist()))
        out.append(("random/%d" % i, _disney_record(m)))
    return out


# ---- the three implementations -------------------------------------------------------------------------------------------------------------

def _p(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


def _f3s(a):
    """A float32 [n, 3] array as ctypes float[3] values over the same memory."""
    return (O.f3 * len(a)).from_buffer(a)


def mirror_sample(km, nn, v, states):
    n = len(nn)
    st = np.ascontiguousarray(states, np.uint32).copy()
    l, h = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    assert hostsim_lib().disneysim_sample(C.byref(km), n, _p(nn), _p(v), _p(st, C.c_uint32), _p(l), _p(h)) == 0
    return l, h, st


def mirror_pdf_eval(km, nn, v, l, h):
    n = len(nn)
    pdf, ev = np.zeros(n, F32), np.zeros((n, 3), F32)
    assert hostsim_lib().disneysim_pdf(C.byref(km), n, _p(nn), _p(l), _p(h), _p(pdf)) == 0
    assert hostsim_lib().disneysim_eval(C.byref(km), n, _p(nn), _p(v), _p(l), _p(h), _p(ev)) == 0
    return pdf, ev


def oracle_sample(om, nn, v, states):
    n = len(nn)
    lib = O.lib()
    l, h = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    st = np.ascontiguousarray(states, np.uint32).copy()
    cn, cv, cl, ch = _f3s(nn), _f3s(v), _f3s(l), _f3s(h)
    seeds = st.view(np.int32)
    for i in range(n):
        s = C.c_int32(int(seeds[i]))
        lib.orc_disney_sample(C.byref(s), C.byref(om), cn[i], cv[i], cl[i], ch[i])
        seeds[i] = s.value
    return l, h, st


def oracle_pdf_eval(om, nn, v, l, h):
    n = len(nn)
    lib = O.lib()
    pdf, ev = np.zeros(n, F32), np.zeros((n, 3), F32)
    cn, cv, cl, ch, ce = _f3s(nn), _f3s(v), _f3s(l), _f3s(h), _f3s(ev)
    base = om.color
    for i in range(n):
        pdf[i] = lib.orc_disney_pdf(C.byref(om), cn[i], cl[i], cv[i], ch[i])
        lib.orc_disney_eval(C.byref(om), base, cn[i], cl[i], cv[i], ch[i], ce[i])
    return pdf, ev


def binary64_pdf_eval(km, nn, v, l, h):
    """The Disney pdf and BRDF as this renderer states them, in binary64 numpy from the binary32 inputs: written from the formulas, not
    from either C source."""
    d = km.disney
    par = {k: float(getattr(d, k)) for k in MC.PARAMS}
    nn, v, l, h = (np.asarray(a, np.float64) for a in (nn, v, l, h))
    dot = lambda a, b: (a * b).sum(axis=1)
    unit = lambda a: a / np.sqrt(dot(a, a))[:, None]
    mix = lambda a, b, t: a + t * (b - a)
    schlick = lambda u: np.clip(1.0 - u, 0.0, 1.0) ** 5

    def gtr1(c, a):
        return np.full_like(c, 1.0 / np.pi) if a >= 1.0 else (a * a - 1.0) / (np.pi * np.log(a * a) * (1.0 + (a * a - 1.0) * c * c))

    def smith(c, ag):
        return 1.0 / (c + np.sqrt(ag * ag + c * c - ag * ag * c * c))

    def smith_aniso(c, x, y, ax, ay):
        return 1.0 / (c + np.sqrt((x * ax) ** 2 + (y * ay) ** 2 + c * c))
    # pdf
    ratio_d = 0.5 * (1.0 - par["metallic"])
    alpha = max(0.001, par["roughness"])
    cc_alpha = mix(0.1, 0.001, par["clearcoatGloss"])
    c = np.abs(dot(nn, h))
    t = 1.0 + (alpha * alpha - 1.0) * c * c
    pdf_h = mix(gtr1(c, cc_alpha) * c, alpha * alpha / (np.pi * t * t) * c, 1.0 / (1.0 + par["clearcoat"]))
    with np.errstate(all="ignore"):
        pdf = ratio_d * np.abs(dot(nn, l)) / np.pi + (1.0 - ratio_d) * pdf_h / (4.0 * np.abs(dot(l, h)))
    # BRDF
    color = np.array([d.color.x, d.color.y, d.color.z], np.float64)
    cdlin = color ** float(F32(2.2))
    lum = 0.3 * cdlin[0] + 0.6 * cdlin[1] + 0.1 * cdlin[2]
    tint = cdlin / lum if lum > 0.0 else np.ones(3)
    cspec0 = mix(mix(np.ones(3), tint, par["specularTint"]) * (par["specular"] * 0.08), cdlin, par["metallic"])
    csheen = mix(np.ones(3), tint, par["sheenTint"])
    ndl, ndv, ndh, ldh = dot(nn, l), dot(nn, v), dot(nn, h), dot(l, h)
    fl, fv = schlick(ndl), schlick(ndv)
    fd90 = 0.5 + 2.0 * ldh * ldh * par["roughness"]
    fd = mix(1.0, fd90, fl) * mix(1.0, fd90, fv)
    fss90 = ldh * ldh * par["roughness"]
    fss = mix(1.0, fss90, fl) * mix(1.0, fss90, fv)
    aspect = np.sqrt(1.0 - par["anisotropic"] * 0.9)
    ax, ay = max(0.001, par["roughness"] ** 2 / aspect), max(0.001, par["roughness"] ** 2 * aspect)
    # the tangent frame of the normal: the binormal lies in the plane x-y or y-z, whichever the normal is further from
    wide = (np.abs(nn[:, 0]) > np.abs(nn[:, 2]))[:, None]
    zero = np.zeros(len(nn))
    binormal = unit(np.where(wide, np.stack([-nn[:, 1], nn[:, 0], zero], axis=1), np.stack([zero, -nn[:, 2], nn[:, 1]], axis=1)))
    x = unit(np.cross(binormal, nn))
    y = unit(np.cross(nn, x))
    with np.errstate(all="ignore"):
        ss = 1.25 * (fss * (1.0 / (ndl + ndv) - 0.5) + 0.5)
        ds = 1.0 / (np.pi * ax * ay * ((dot(h, x) / ax) ** 2 + (dot(h, y) / ay) ** 2 + ndh * ndh) ** 2)
        fh = schlick(ldh)
        fs = mix(cspec0[None, :], np.ones(3)[None, :], fh[:, None])
        gs = smith_aniso(ndl, dot(l, x), dot(l, y), ax, ay) * smith_aniso(ndv, dot(v, x), dot(v, y), ax, ay)
        dr = gtr1(ndh, cc_alpha)
        fr = mix(0.04, 1.0, fh)
        gr = smith(ndl, 0.25) * smith(ndv, 0.25)
        diffuse = (cdlin[None, :] * ((1.0 / np.pi) * mix(fd, ss, par["subsurface"]))[:, None] + csheen[None, :] * (fh * par["sheen"])[:, None]) * (1.0 - par["metallic"])
        ev = diffuse + fs * (gs * ds)[:, None] + (0.25 * par["clearcoat"] * gr * fr * dr)[:, None]
    return pdf, ev


# ---- a. the functions, one call at a time ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def function_results():
    """Per material: inputs, the mirror's and the oracle's sample / pdf / eval, and the binary64 values.  Case materials take the full
    direction set; a random material takes a set a tenth the size, drawn for it."""
    rng = np.random.default_rng(77)
    big = directions(rng, 256, 24)
    rows = []
    for label, km in _materials():
        nn, v, l, h = big if not label.startswith("random/") else directions(rng, 32, 2)
        om = _orc_record(km)
        states = rng.integers(0, 2 ** 32, len(nn), dtype=np.uint64).astype(np.uint32)
        rows.append(dict(label=label, km=km, n=len(nn), sample_m=mirror_sample(km, nn, v, states), sample_o=oracle_sample(om, nn, v, states),
                         m=mirror_pdf_eval(km, nn, v, l, h), o=oracle_pdf_eval(om, nn, v, l, h), ref=binary64_pdf_eval(km, nn, v, l, h)))
    return rows


def test_every_parameter_is_off_its_default_somewhere_and_at_both_ends():
    mats = [m for name in MC.CASE_NAMES for m in MC.case_materials(name)]
    for k in MC.PARAMS:
        vals = {F32(m[k]) for m in mats}
        assert F32(0.0) in vals and F32(1.0) in vals and len(vals - {F32(MC.DEFAULTS[k]), F32(0.0), F32(1.0)}) > 0, k
        assert all(0.0 <= x <= 1.0 for x in vals), k
    assert len(MC.case_materials(MC.TWELVE)) >= 12 and any(m["brdf"] == 1 for m in MC.case_materials(MC.GLASS))
    hs = MC.case_scene(MC.LAMBERTIAN, W, H)
    assert sum(MC.scene_material(hs, i).kind == K.MAT_LAMBERTIAN for i in range(hs.sizes.nMaterials)) == 1
    a, b = MC.case_materials("all")
    assert all(F32(a[k]) != F32(b[k]) != F32(MC.DEFAULTS[k]) != F32(a[k]) for k in MC.PARAMS)


def test_disney_sample_gives_the_oracles_directions_bit_for_bit(function_results):
    """Directions are part of the path: L, H and the RNG state afterwards are the oracle's bits, both lobes, every material."""
    n = 0
    for r in function_results:
        for a, b, what in zip(r["sample_m"], r["sample_o"], ("L", "H", "state")):
            assert a.tobytes() == b.tobytes(), (r["label"], what)
        assert np.isfinite(r["sample_m"][0]).all() and np.isfinite(r["sample_m"][1]).all(), r["label"]
        n += r["n"]
    print("material_cases: disney_sample: %d draws over %d materials, L, H and state bit-identical to the oracle's" % (n, len(function_results)))


def _rel_errors(got, ref, keep):
    got = np.asarray(got, np.float64).reshape(len(ref), -1); ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    with np.errstate(all="ignore"):
        e = np.abs(got - ref) / np.abs(ref)
    return e[keep.reshape(len(ref), -1)]


@pytest.mark.parametrize("which", ["pdf", "eval"])
def test_disney_pdf_and_eval_against_the_oracle_and_binary64(function_results, which):
    """Measured: the mirror's pdf and eval are the oracle's binary32 bits on every input, so equality is what is asserted.  The binary64
    restatement then measures what binary32 costs either of them: the mirror's worst relative error may not exceed twice the
    oracle's (trivially met while the bits are equal; the check that remains should they ever part).  Inputs whose binary64 value is 0
    or not finite are left out: under 1 % of them, and on the others the oracle's value is finite."""
    k = 0 if which == "pdf" else 1
    total = dropped = differing = 0
    worst_m = worst_o = 0.0
    for r in function_results:
        m, o, ref = r["m"][k], r["o"][k], r["ref"][k]
        keep = np.isfinite(ref) & (ref != 0.0)
        total += keep.size; dropped += int((~keep).sum())
        assert np.isfinite(o[keep]).all(), r["label"]
        differing += int((m.view(np.uint32) != o.view(np.uint32)).sum())
        em, eo = _rel_errors(m, ref, keep), _rel_errors(o, ref, keep)
        if em.size:
            worst_m, worst_o = max(worst_m, float(em.max())), max(worst_o, float(eo.max()))
    print("material_cases: disney_%s: %d values, %d differ in bits from the oracle's; worst relative error against binary64: mirror %.3g, "
          "oracle %.3g; %d left out (binary64 value 0 or not finite)" % (which, total, differing, worst_m, worst_o, dropped))
    assert dropped < 0.01 * total
    assert differing == 0
    assert worst_m <= 2.0 * worst_o


# ---- b. renders ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,tilted", [(n, False) for n in MC.CASE_NAMES] + [("all", True), ("aniso", True)])
def test_case_renders_match_the_oracle_and_each_other(name, tilted):
    """96 x 54, 4 samples, every pixel: the per-ray state machine on 128-byte nodes and the packet one on 64-byte nodes give the same bits,
    the oracle's image to RMSE 2e-6 and its four ray counts.  Two cases once more with two different normals per face (the tangent
    frame of the anisotropic terms then turns across a face)."""
    hs = MC.case_scene(name, W, H, tilted_normals=tilted)
    sim = HostsimHandle(hs)
    o, ost = oracle_scene(hs).render(SEEDS)
    a, ca = hostsim_render(sim, SEEDS, node_format=128)
    b, cb = hostsim_render(sim, SEEDS, node_format=64, packet=1)
    sim.close()
    e = rmse(a / len(SEEDS), o / len(SEEDS))
    print("material_cases: render %s%s: RMSE against the oracle %.3g, %d rays" % (name, " (tilted normals)" if tilted else "", e, ost.rays))
    assert np.isfinite(a).all() and np.isfinite(o).all() and a.max() > 0
    assert a.tobytes() == b.tobytes()
    assert e <= RMSE_TIGHT
    for c in (ca, cb):
        assert (c["primaryRays"], c["bounceRays"], c["shadowRays"], c["closestHits"]) == \
               (ost.primaryRays, ost.bounceRays, ost.shadowRays, ost.closestHits)


# ---- c. grazing rays -------------------------------------------------------------------------------------------------------------------------

def _oracle_trace(osc, rays, states):
    out = np.zeros((len(rays), 3), F32)
    o, d, res = _f3s(np.ascontiguousarray(rays[:, 0:3])), _f3s(np.ascontiguousarray(rays[:, 3:6])), _f3s(out)
    for i in range(len(rays)):
        O.lib().orc_trace_one(C.byref(osc.c), o[i], d[i], int(states[i]), res[i])
    return out


def _relative(a, b):
    """Per ray: the largest channel difference over the larger of the reference's largest channel and 1 -- relative where the clamp to
    [0, 1] hides a radiance, absolute below it."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1.0)


@pytest.mark.parametrize("name", MC.GRAZING_CASES)
def test_grazing_rays_match_the_oracles_tracer(name):
    """512 rays per elevation 1e-1 .. 1e-5 rad towards the floor, one RNG state per ray, unclamped.  Finite everywhere; clamped RMSE
    2e-6.  The unclamped relative difference is held to twice the oracle's own spread between its binary32 and binary64 Disney
    arithmetic on the same rays, per case and elevation.  Measured: the difference is at most 5.3e-7 on every set (metal1's radiances
    reach 2.6e5 there); the spread is 7.7e-6 at its smallest and of order 1 and more where the binary64 arithmetic sends a path
    elsewhere, so it bounds the difference everywhere, by a factor of 35 at the least."""
    hs = MC.case_scene(name, W, H)
    sim, osc = HostsimHandle(hs), oracle_scene(hs)
    try:
        for elevation, rays in MC.grazing_sets(hs).items():
            states = np.random.default_rng(int(1e6 * elevation) + 5).integers(0, 2 ** 31, len(rays), dtype=np.int64).astype(np.uint32)
            got = radiancesim(sim, rays, states=states[:, None], clamp=False)[:, :3]
            want = _oracle_trace(osc, rays, states.view(np.int32))
            O.set_option("disney_binary64", 1)
            try:
                want64 = _oracle_trace(osc, rays, states.view(np.int32))
            finally:
                O.set_option("disney_binary64", 0)
            assert np.isfinite(got).all() and np.isfinite(want).all()
            e = rmse(np.clip(got, 0, 1), np.clip(want, 0, 1))
            diff, spread = _relative(got, want), _relative(want64, want)
            print("material_cases: grazing %s at %g rad: clamped RMSE %.3g, largest clamped difference %.3g, largest radiance %.3g, "
                  "largest relative difference %.3g (the oracle's binary32 / binary64 spread: %.3g)" % (
                      name, elevation, e, float(np.abs(np.clip(got, 0, 1) - np.clip(want, 0, 1)).max()), float(want.max()),
                      float(diff.max()), float(spread.max())))
            assert want.any()
            assert e <= RMSE_TIGHT
            assert diff.max() <= 2.0 * spread.max()
    finally:
        sim.close()
