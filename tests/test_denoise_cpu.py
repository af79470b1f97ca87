"""The denoiser (include/moptix.h "denoiser") without a GPU: exp_ac against float64 exp, the CPU mirror of the kernels (tests/hostsim/denoisesim.cpp,
the kernels' own per-pixel code from pt_denoise.h) against an independent float64 implementation of the semantics written here from the
header's text, the filter's properties, its quality on path-traced frames, and the C ABI's host-only entry points."""
import ctypes as C

import numpy as np
import pytest

from common import M, K, hostsim_render, rmse, textured_scene
from aov_helpers import aovsim_render
from denoise_helpers import DEFAULTS, denoisesim, exp_ac, pow_int, synthetic_aovs

F = np.float64
LUM = np.array([0.2126, 0.7152, 0.0722], F)
H5 = {-2: 1 / 16, -1: 1 / 4, 0: 3 / 8, 1: 1 / 4, 2: 1 / 16}
H3 = {-1: 1 / 4, 0: 1 / 2, 1: 1 / 4}


# ---------------------------------------------------------------------------------------------
# the semantics in float64, from the header's text
# ---------------------------------------------------------------------------------------------
def _shift(a, dx, dy, fill=0):
    """out[y, x] = a[y + dy, x + dx] where that is inside the frame, else `fill`."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    if abs(dx) >= w or abs(dy) >= h:
        return out
    out[max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx)] = a[max(0, dy):h - max(0, -dy), max(0, dx):w - max(0, -dx)]
    return out


def spec_denoise(accum, aovs, n_accumulation, n_samples, iterations=5, normal_power=128, sigma_luminance=4.0, sigma_depth=1.0,
                 demodulate=False):
    c = accum.astype(F) / F(n_accumulation)
    if iterations == 0:
        return c
    hits = aovs["hits"][..., 0].astype(F)
    geo = hits > 0
    s = F(n_samples)
    nr = aovs["normal"].astype(F) / s
    ln = np.sqrt((nr * nr).sum(-1, keepdims=True))
    n = np.where(ln > 0, nr / np.where(ln > 0, ln, 1), 0)
    z = np.where(geo, aovs["depth"][..., 0].astype(F) / np.where(geo, hits, 1), 0)
    a = np.maximum(aovs["albedo"].astype(F) / s, 1e-3) if demodulate else np.ones_like(c)
    i_ = c / a
    lum = lambda x: x @ LUM
    # prepass: variance over the 3x3 window's geometry pixels, depth gradient
    l = lum(i_)
    s1, s2, cnt = np.zeros_like(l), np.zeros_like(l), np.zeros_like(l)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            m = _shift(geo, dx, dy, False)
            lq = _shift(l, dx, dy)
            s1 += np.where(m, lq, 0); s2 += np.where(m, lq * lq, 0); cnt += m
    cnt = np.maximum(cnt, 1)
    v = np.maximum(s2 / cnt - (s1 / cnt) ** 2, 0)

    def axis(dx, dy):
        lo, hi = _shift(geo, -dx, -dy, False), _shift(geo, dx, dy, False)
        zl, zh = _shift(z, -dx, -dy), _shift(z, dx, dy)
        return np.where(lo & hi, np.abs(zh - zl) / 2, np.where(lo, np.abs(z - zl), np.where(hi, np.abs(zh - z), 0)))

    g = np.maximum(axis(1, 0), axis(0, 1))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for it in range(iterations):
            step = 2 ** it
            sv, sk = np.zeros_like(v), np.zeros_like(v)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    m = _shift(geo, dx, dy, False)
                    sv += np.where(m, H3[dx] * H3[dy] * _shift(v, dx, dy), 0); sk += np.where(m, H3[dx] * H3[dy], 0)
            den_l = sigma_luminance * np.sqrt(sv / sk) + 1e-4
            lp = lum(i_)
            sw, si, svv = np.zeros_like(v), np.zeros_like(i_), np.zeros_like(v)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    m = _shift(geo, step * dx, step * dy, False)
                    iq, vq = _shift(i_, step * dx, step * dy), _shift(v, step * dx, step * dy)
                    if dx == 0 and dy == 0:
                        w = np.full_like(v, 9 / 64)
                    else:
                        nq, zq = _shift(n, step * dx, step * dy), _shift(z, step * dx, step * dy)
                        wn = np.maximum((n * nq).sum(-1), 0) ** normal_power
                        wz = np.exp(-np.abs(z - zq) / (sigma_depth * step * (abs(dx) + abs(dy)) * g + 1e-4))
                        wl = np.exp(-np.abs(lp - lum(iq)) / den_l)
                        w = H5[dx] * H5[dy] * wn * wz * wl
                    w = np.where(m, w, 0)
                    sw += w; si += w[..., None] * iq; svv += w * w * vq
            i_ = np.where(geo[..., None], si / sw[..., None], i_)
            v = np.where(geo, svv / (sw * sw), v)
    return np.where(geo[..., None], i_ * a, c)


def _rel_err(got, want):
    """max per-channel |got - want| relative to the larger of |want| and the frame's mean |want| (a channel near 0 next to bright
    ones is compared on the frame's scale)"""
    want = np.asarray(want, F)
    scale = np.maximum(np.abs(want), np.abs(want).mean())
    return float((np.abs(got.astype(F) - want) / scale).max())


def _assert_close(got, want, normal_power=DEFAULTS["normal_power"]):
    """Relative error <= 1e-5: over the frame (norm-wise), and per pixel where the normal weight allows it.  w_n = x^n has condition
    number n, so the binary32 rounding of the normalised normals (~2^-23) reaches n 2^-23 in a weight -- 1.5e-5 at n = 128 -- and the
    per-pixel bound grows with n / 8."""
    want = np.asarray(want, F)
    d = got.astype(F) - want
    assert float(np.linalg.norm(d) / np.linalg.norm(want)) <= 1e-5
    assert _rel_err(got, want) <= 1e-5 * max(1.0, normal_power / 8.0)


def _scene(kind, tmp_path, w, h):
    return textured_scene(tmp_path, w, h) if kind == "textured" else M.HostScene(kind, w, h)


def _rendered(hs, spp, first=0, base=0):
    seeds = M.launch_seeds(spp, base, first)
    accum, _ = hostsim_render(hs, seeds)
    return accum, aovsim_render(hs, seeds), spp


# ---------------------------------------------------------------------------------------------
# exp_ac and the integer power
# ---------------------------------------------------------------------------------------------
def test_exp_ac_relative_error_exact_points_and_monotone():
    x = np.linspace(-87.0, 0.0, 2_000_001).astype(np.float32)
    y = exp_ac(x)
    want = np.exp(x.astype(F))
    assert float((np.abs(y.astype(F) - want) / want).max()) <= 2.0 ** -21
    assert (np.diff(y.astype(F)) >= 0).all()
    assert exp_ac([0.0])[0] == np.float32(1.0) and exp_ac([-0.0])[0] == np.float32(1.0)
    below = exp_ac([-87.00001, -88.0, -100.0, -1e30, -np.inf])
    assert (below == 0).all() and not np.signbit(below).any()
    assert (exp_ac(np.float32([-87.0])) > 0).all()


@pytest.mark.parametrize("e", [1, 2, 3, 7, 64, 128, 255, 256])
def test_integer_power_is_the_documented_binary_exponentiation(e):
    x = np.random.RandomState(e).rand(1000).astype(np.float32)
    want = np.empty_like(x)
    for k, xv in enumerate(x):
        r, b, n = np.float32(1), xv, e
        while True:
            if n & 1:
                r = np.float32(r * b)
            n >>= 1
            if n == 0:
                break
            b = np.float32(b * b)
        want[k] = r
    assert np.array_equal(pow_int(x, e).view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------
# mirror against the semantics
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spheres", "cornell_quads", "file:coffee", "textured"])
def test_mirror_matches_the_semantics_on_rendered_frames(kind, tmp_path):
    hs = _scene(kind, tmp_path, 61, 37)
    accum, aovs, n = _rendered(hs, 4)
    assert (aovs["hits"] > 0).any()
    for demodulate in (False, True):
        _assert_close(denoisesim(accum, aovs, n, aovs["samples"], demodulate=demodulate),
                      spec_denoise(accum, aovs, n, aovs["samples"], demodulate=demodulate))


@pytest.mark.parametrize("iterations", [1, 3, 5, 8])
@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("normal_power", [1, 7, 128])
def test_mirror_matches_the_semantics_on_synthetic_fields(iterations, demodulate, normal_power):
    accum, aovs, s = synthetic_aovs(29, 43, seed=iterations * 10 + normal_power)
    kw = dict(iterations=iterations, demodulate=demodulate, normal_power=normal_power, sigma_luminance=2.5, sigma_depth=0.7)
    _assert_close(denoisesim(accum, aovs, 3.0, s, **kw), spec_denoise(accum, aovs, 3.0, s, **kw), normal_power)


# ---------------------------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_zero_iterations_return_the_beauty_mean_bits():
    accum, aovs, s = synthetic_aovs(23, 31, seed=3)
    c = accum / np.float32(3.0)
    for demodulate in (False, True):
        assert np.array_equal(_bits(denoisesim(accum, aovs, 3.0, s, iterations=0, demodulate=demodulate)), _bits(c))


def test_background_passes_through_and_influences_nothing():
    accum, aovs, s = synthetic_aovs(31, 37, seed=5, background=0.3)
    bg = aovs["hits"][..., 0] == 0
    a = denoisesim(accum, aovs, 2.0, s)
    assert np.array_equal(_bits(a[bg]), _bits(accum[bg] / np.float32(2.0)))
    other = accum.copy()
    other[bg] = np.float32(1e6)
    b = denoisesim(other, aovs, 2.0, s)
    assert np.array_equal(_bits(a[~bg]), _bits(b[~bg]))
    assert np.array_equal(_bits(b[bg]), _bits(other[bg] / np.float32(2.0)))


@pytest.mark.parametrize("demodulate", [False, True])
def test_a_constant_field_stays_constant(demodulate):
    h, w, s = 27, 33, 4
    accum = np.full((h, w, 3), 0.7, np.float32) * np.float32([1.0, 0.5, 0.25])
    _, aovs, _ = synthetic_aovs(h, w, seed=9, background=0.0, n_samples=s)
    aovs["albedo"][:] = np.float32(0.5 * s)
    out = denoisesim(accum, aovs, 1.0, s, demodulate=demodulate)
    assert float((np.abs(out.astype(F) - accum.astype(F)) / accum.astype(F)).max()) <= 1e-6


def test_a_cancelled_normal_gives_a_finite_output():
    accum, aovs, s = synthetic_aovs(17, 19, seed=11, background=0.0)
    aovs["normal"][8, 9] = 0
    out = denoisesim(accum, aovs, 1.0, s)
    assert np.isfinite(out).all()


def test_orthogonal_half_planes_do_not_bleed():
    h, w, s = 32, 40, 2
    left = np.arange(w)[None, :] < w // 2
    normal = np.where(left[..., None], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]) * np.ones((h, 1, 1))
    colour = np.where(left[..., None], [0.9, 0.1, 0.1], [0.1, 0.1, 0.9]) * np.ones((h, 1, 1))
    aovs = dict(albedo=np.full((h, w, 3), 0.8 * s, np.float32), normal=(normal * s).astype(np.float32),
                depth=np.full((h, w, 1), 3.0 * s, np.float32), hits=np.full((h, w, 1), s, np.float32))
    out = denoisesim(colour.astype(np.float32), aovs, 1.0, s, normal_power=DEFAULTS["normal_power"])
    assert float(np.abs(out - colour).max()) <= 1e-5


@pytest.mark.parametrize("h,w", [(1, 1), (1, 8), (8, 1)])
def test_tiny_frames(h, w):
    accum, aovs, s = synthetic_aovs(h, w, seed=h * 8 + w, background=0.0)
    for it in (0, 1, 5):
        got = denoisesim(accum, aovs, 2.0, s, iterations=it)
        assert np.isfinite(got).all()
        _assert_close(got, spec_denoise(accum, aovs, 2.0, s, iterations=it))


# ---------------------------------------------------------------------------------------------
# quality: 4 spp denoised against 512 spp on disjoint seeds (192x108: at 128x72 the silhouettes' partly covered pixels, which the
# filter takes for the surface, and the 5-level footprint against small features keep cornell_quads at 0.57 with any parameters)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["file:coffee", "cornell_quads"])
def test_denoised_4spp_halves_the_error(kind, record_property):
    hs = M.HostScene(kind, 192, 108)
    accum, aovs, n = _rendered(hs, 4)
    ref, _ = hostsim_render(hs, M.launch_seeds(512, 0, 1000))
    ref = ref / np.float32(512)
    noisy = accum / np.float32(n)
    den = denoisesim(accum, aovs, n, aovs["samples"])          # the defaults
    e_noisy, e_den = rmse(noisy, ref), rmse(den, ref)
    ratio = e_den / e_noisy
    record_property("rmse_ratio", ratio)
    print("%s 192x108: RMSE noisy 4 spp %.4f, denoised %.4f, ratio %.3f" % (kind, e_noisy, e_den, ratio))
    assert ratio <= 0.5


# ---------------------------------------------------------------------------------------------
# host-only entry points
# ---------------------------------------------------------------------------------------------
def test_defaults_without_a_device_and_a_null_context():
    lib = K.device_lib()
    p = K.DenoiseParams()
    assert lib.moptix_denoise_defaults(C.byref(p)) == K.MOPTIX_OK
    assert (p.iterations, p.normalPower, p.demodulate, p.sigmaLuminance, p.sigmaDepth) == (5, 128, 0, 4.0, 1.0)
    assert dict(iterations=5, normal_power=128, sigma_luminance=4.0, sigma_depth=1.0, demodulate=False) == DEFAULTS
    assert lib.moptix_denoise_defaults(None) == K.ERR_INVALID
    assert lib.moptix_denoise(None, C.byref(p), 1.0) == K.ERR_INVALID
    out = (C.c_float * 3)()
    assert lib.moptix_denoise_read(None, out) == K.ERR_INVALID
    assert lib.moptix_denoise_bind(None, None) == K.ERR_INVALID
