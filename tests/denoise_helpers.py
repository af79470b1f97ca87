"""The denoiser of the CPU mirror (tests/hostsim/denoisesim.cpp) for the denoiser tests."""
import ctypes as C

import numpy as np

from common import K, _f32, _ptr, hostsim_lib

DEFAULTS = dict(iterations=5, normal_power=128, sigma_luminance=4.0, sigma_depth=1.0, demodulate=False)


def denoisesim(accum, aovs, n_accumulation, n_samples, iterations=5, normal_power=128, sigma_luminance=4.0, sigma_depth=1.0,
               demodulate=False):
    """moptix_denoise on the CPU.  accum: (H, W, 3) sums; aovs: dict with albedo, normal (H, W, 3) and depth, hits (H, W, 1) sums, as
    aov_read / aovsim_render return them; n_samples = their sample count.  Returns (H, W, 3) float32 in the same row order."""
    accum = _f32(accum)
    h, w = accum.shape[:2]
    ins = [_f32(aovs[n]) for n in ("albedo", "normal", "depth", "hits")]
    assert ins[0].size == ins[1].size == 3 * h * w and ins[2].size == ins[3].size == h * w
    out = np.empty((h, w, 3), np.float32)
    p = K.DenoiseParams(int(iterations), int(normal_power), 1 if demodulate else 0, float(sigma_luminance), float(sigma_depth))
    rc = hostsim_lib().denoisesim_run(w, h, _ptr(accum), *[_ptr(a) for a in ins], float(n_accumulation), float(n_samples), C.byref(p), _ptr(out))
    assert rc == 0
    return out


def exp_ac(x):
    x = _f32(x).reshape(-1)
    y = np.empty_like(x)
    hostsim_lib().denoisesim_exp_ac(_ptr(x), _ptr(y), len(x))
    return y


def pow_int(x, e):
    x = _f32(x).reshape(-1)
    y = np.empty_like(x)
    hostsim_lib().denoisesim_pow_int(_ptr(x), int(e), _ptr(y), len(x))
    return y


def synthetic_aovs(h, w, seed, background=0.25, n_samples=4):
    """Random guide layers and beauty sums: piecewise normals and depths with noise, random albedo, a `background` share of pixels with
    hits = 0 (and zero depth / normal / albedo of a miss's kind).  Returns (accum, aovs, n_samples)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    region = ((xx * 3) // max(w, 1) + 3 * ((yy * 2) // max(h, 1))).astype(np.int32)
    base_n = rng.normal(size=(6, 3)); base_n[:, 2] = np.abs(base_n[:, 2]) + 0.5
    base_n /= np.linalg.norm(base_n, axis=1, keepdims=True)
    normal = base_n[region] + 0.05 * rng.normal(size=(h, w, 3))
    depth = 2.0 + region + 0.01 * xx + 0.02 * yy + 0.01 * rng.rand(h, w)
    albedo = rng.rand(6, 3)[region] * (0.6 + 0.4 * rng.rand(h, w, 1))
    colour = (0.3 + rng.rand(6, 3))[region] * albedo
    accum = colour * rng.gamma(2.0, 0.5, size=(h, w, 1)) * 8.0
    hits = np.full((h, w), float(n_samples))
    bg = rng.rand(h, w) < background
    hits[bg] = 0
    aovs = dict(albedo=(albedo * n_samples).astype(np.float32), normal=(normal * n_samples).astype(np.float32),
                depth=(depth * hits)[..., None].astype(np.float32), hits=hits[..., None].astype(np.float32))
    aovs["normal"][bg] = 0
    aovs["albedo"][bg] = np.float32(0.2 * n_samples)
    return accum.astype(np.float32), aovs, n_samples
