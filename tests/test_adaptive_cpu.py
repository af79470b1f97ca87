"""Adaptive sampling without a GPU: the defaults and the argument check, the CPU mirror of the kernels and the pass schedule
(tests/hostsim/adaptivesim.cpp) against the semantics of include/moptix.h -- the threshold-0 anchor, the prefix property, the moments -- and what
adaptive sampling buys at equal cost on the denoiser tests' scenes."""
import ctypes as C

import numpy as np
import pytest

from common import M, K, hostsim_render, rmse
from adaptive_helpers import ADAPTIVE_DEFAULTS, AdaptiveSim, check_params, hostsim_samples, prefix_pick, sequential_sums


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_bits(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = _bits(got) == _bits(want)
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:5].tolist())


@pytest.fixture(scope="module")
def small():
    """cornell_quads 64x36, 56 seeds: (samples, sequential sums)."""
    hs = M.HostScene("cornell_quads", 64, 36)
    samples = hostsim_samples(hs, M.launch_seeds(56, 3, 0))
    return samples, sequential_sums(samples)


# ---------------------------------------------------------------------------------------------
# 1 host-only entry points
# ---------------------------------------------------------------------------------------------
def test_defaults_without_a_device_and_the_argument_check():
    lib = K.device_lib()
    p = K.AdaptiveParams()
    assert lib.moptix_adaptive_defaults(C.byref(p)) == K.MOPTIX_OK
    assert (np.float32(p.threshold), p.minSamples, p.batch) == (np.float32(0.03), 16, 64)
    assert lib.moptix_adaptive_defaults(None) == K.ERR_INVALID
    d = M.Context.adaptive_defaults()                       # no context, no device
    assert d == dict(threshold=float(np.float32(0.03)), min_samples=16, batch=64)
    assert {k: float(np.float32(v)) if k == "threshold" else v for k, v in ADAPTIVE_DEFAULTS.items()} == d
    # the entry points reject a NULL context / NULL arguments before they touch a device
    st = K.AdaptiveStats()
    assert lib.moptix_render_adaptive(None, None, 0, C.byref(p), C.byref(st)) == K.ERR_INVALID
    assert lib.moptix_render_adaptive(None, None, 0, None, None) == K.ERR_INVALID
    assert lib.moptix_adaptive_clear(None) == K.ERR_INVALID
    assert lib.moptix_adaptive_read(None, None) == K.ERR_INVALID
    assert lib.moptix_adaptive_mean(None, None) == K.ERR_INVALID
    assert lib.moptix_adaptive_mean_device(None, None) == K.ERR_INVALID
    assert lib.moptix_adaptive_resolve_rgb8(None, None) == K.ERR_INVALID
    # ranges as the header documents them: threshold >= 0 and finite, minSamples >= 1, batch >= 1 -- the library's own check first (it
    # comes before the context is looked at, so it runs without a device: the error text tells which check spoke), then the mirror's,
    # which is the same function (pt_adaptive.h ad_bad_params)
    def abi(threshold, min_samples, batch):
        q = K.AdaptiveParams(float(threshold), int(min_samples), int(batch))
        assert lib.moptix_render_adaptive(None, None, 0, C.byref(q), None) == K.ERR_INVALID
        return lib.moptix_last_error(None).decode()
    for ok in ((0.0, 1, 1), (0.03, 16, 64), (1e30, 1000, 7)):
        assert abi(*ok) == "null context", ok
    for bad, word in (((-1e-6, 16, 16), "threshold"), ((float("nan"), 16, 16), "threshold"), ((float("inf"), 16, 16), "threshold"),
                      ((0.03, 0, 16), "minSamples"), ((0.03, -3, 16), "minSamples"), ((0.03, 16, 0), "batch")):
        assert word in abi(*bad), bad
    for ok in ((0.0, 1, 1), (0.03, 16, 16), (1e30, 1000, 7)):
        assert check_params(*ok) == K.MOPTIX_OK, ok
    for bad in ((-1e-6, 16, 16), (float("nan"), 16, 16), (float("inf"), 16, 16), (0.03, 0, 16), (0.03, -3, 16), (0.03, 16, 0)):
        assert check_params(*bad) == K.ERR_INVALID, bad


# ---------------------------------------------------------------------------------------------
# 2 threshold 0: the plain sequential sum
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_samples,batch", [(16, 16), (1, 1), (7, 5), (100, 3)])
def test_threshold_zero_is_the_sequential_sum(small, min_samples, batch):
    samples, sums = small
    n = len(samples)
    sim = AdaptiveSim(64, 36)
    st = sim.render(samples, threshold=0.0, min_samples=min_samples, batch=batch)
    r = sim.read()
    _assert_bits(r["accum"], sums[n])
    assert (r["count"] == n).all() and not r["converged"].any()
    first = min(min_samples, n)
    assert st == dict(passes=1 + -(-(n - first) // batch), samples_traced=64 * 36 * n, samples_uniform=64 * 36 * n,
                      active_pixels_last=64 * 36, converged_pixels=0, min_count=n, max_count=n)


# ---------------------------------------------------------------------------------------------
# 3 the prefix property, the counts a schedule allows, converged is sticky
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold,min_samples,batch", [(0.03, 16, 16), (0.1, 4, 8), (0.05, 8, 3)])
def test_every_pixel_holds_a_prefix_of_the_seed_list(small, threshold, min_samples, batch):
    samples, sums = small
    n = len(samples)
    sim = AdaptiveSim(64, 36)
    st = sim.render(samples, threshold=threshold, min_samples=min_samples, batch=batch)
    r = sim.read()
    _assert_bits(r["accum"], prefix_pick(sums, r["count"]))
    allowed = set(range(min_samples, n, batch)) | {n}
    assert set(np.unique(r["count"]).tolist()) <= allowed
    assert len(np.unique(r["count"])) >= 2, "the threshold stops no pixel or every pixel at once: the case shows nothing"
    assert st["samples_traced"] == int(r["count"].sum()) and st["min_count"] == r["count"].min() and st["max_count"] == r["count"].max()
    assert st["converged_pixels"] == int(r["converged"].sum()) and st["active_pixels_last"] == 64 * 36 - st["converged_pixels"]
    # a pixel that stopped early is converged; a converged pixel met the rule's first half
    assert (r["converged"][r["count"] < n] == 1).all() and (r["count"][r["converged"] == 1] >= min_samples).all()
    # the error buffer is e of the pixel's own moments
    cnt = r["count"].astype(np.float32)
    m = r["moments"][..., 0] / cnt
    v = np.maximum(np.float32(0), r["moments"][..., 1] / cnt - m * m)
    _assert_bits(r["error"], (np.sqrt(v / cnt) / (m + np.float32(0.01))).astype(np.float32))


def test_two_calls_continue_and_converged_is_monotone(small):
    samples, sums = small
    kw = dict(threshold=0.05, min_samples=8, batch=8)
    one = AdaptiveSim(64, 36)
    st1 = one.render(samples, **kw)
    two = AdaptiveSim(64, 36)
    two.render(samples[:24], **kw)                  # 24 = 8 + 2 * 8: a pass boundary of the joint call
    a = two.read()
    st2 = two.render(samples[24:], **kw)
    b = two.read()
    assert (b["converged"] >= a["converged"]).all() and (b["count"] >= a["count"]).all()
    want = one.read()
    for k in ("accum", "moments", "error"):
        _assert_bits(b[k], want[k], k)
    assert (b["count"] == want["count"]).all() and (b["converged"] == want["converged"]).all()
    assert {k: st2[k] for k in ("active_pixels_last", "converged_pixels", "min_count", "max_count")} == \
           {k: st1[k] for k in ("active_pixels_last", "converged_pixels", "min_count", "max_count")}
    # a call whose seeds all go to converged pixels traces nothing; clear() starts over
    two.clear()
    r = two.read()
    assert not r["accum"].any() and not r["count"].any() and not r["converged"].any() and not r["moments"].any()


# ---------------------------------------------------------------------------------------------
# 4 moments against float64
# ---------------------------------------------------------------------------------------------
def test_moments_are_the_luminance_sums_within_the_float32_summation_bound(small):
    samples, _ = small
    n = len(samples)
    sim = AdaptiveSim(64, 36)
    sim.render(samples, threshold=0.0)
    r = sim.read()
    # l in binary32 in the documented operation order; the sums in float64 of those same terms
    l = (np.float32(0.2126) * samples[..., 0] + np.float32(0.7152) * samples[..., 1]) + np.float32(0.0722) * samples[..., 2]
    assert l.dtype == np.float32
    l2 = l * l
    for got, terms in ((r["moments"][..., 0], l), (r["moments"][..., 1], l2)):
        exact = terms.astype(np.float64).sum(axis=0)
        # n - 1 sequential binary32 adds of non-negative terms: |error| <= (n - 1) u sum|term| to first order, u = 2^-24; n u sum|term| covers it
        bound = n * 2.0 ** -24 * np.abs(terms.astype(np.float64)).sum(axis=0)
        assert (np.abs(got.astype(np.float64) - exact) <= bound).all()
    mean, rgb8 = sim.mean()
    _assert_bits(mean, r["accum"] / np.float32(n))
    want8 = ((np.clip(mean, 0, 1) * np.float32(65535.0) + np.float32(0.5)).astype(np.uint32) >> 8).astype(np.uint8)[::-1]
    assert (rgb8 == want8).all()


# ---------------------------------------------------------------------------------------------
# 5 quality at equal cost (192x108, the denoiser tests' size and scenes): adaptive with a budget of 128 seeds traces S samples; uniform
# rendering with ceil(S / pixels) seeds is the opponent; both against 1,024 uniform samples on disjoint seeds.  Measured with the mirror
# at the defaults, threshold 0.03, minSamples 16, batch 64 (DESIGN.md "Adaptive sampling"; batch 16 and 32 give the same ratios to three digits):
#   cornell_quads  S / uniform 0.406, 31.5 % of the pixels at the full 128, RMSE 0.00736 against 0.01087 (52 seeds): ratio 0.677
#   coffee         S / uniform 0.858, 83.7 % at 128,                        RMSE 0.01875 against 0.02006 (110 seeds): ratio 0.935
# asserted with a margin of 10 % of the measured value, as the denoiser's quality tests are.
# ---------------------------------------------------------------------------------------------
MEASURED_RATIO = {"cornell_quads": 0.677, "file:coffee": 0.935}


@pytest.mark.parametrize("kind", ["cornell_quads", "file:coffee"])
def test_adaptive_beats_uniform_sampling_at_equal_cost(kind, record_property):
    w, h, budget = 192, 108, 128
    hs = M.HostScene(kind, w, h)
    samples = hostsim_samples(hs, M.launch_seeds(budget, 0, 0))
    ref, _ = hostsim_render(hs, M.launch_seeds(1024, 0, 5000))
    ref = ref / np.float32(1024)
    sim = AdaptiveSim(w, h)
    st = sim.render(samples, **ADAPTIVE_DEFAULTS)
    r = sim.read()
    mean, _ = sim.mean()
    s = st["samples_traced"]
    n_eq = -(-s // (w * h))
    uniform = sequential_sums(samples[:n_eq])[n_eq] / np.float32(n_eq)
    share, full = s / st["samples_uniform"], float((r["count"] == budget).mean())
    e_ad, e_un = rmse(mean, ref), rmse(uniform, ref)
    ratio = e_ad / e_un
    record_property("rmse_ratio", ratio)
    print("%s 192x108: traced %.3f of uniform, %.3f of the pixels at %d, RMSE adaptive %.5f, uniform %d seeds %.5f, ratio %.3f" % (
        kind, share, full, budget, e_ad, n_eq, e_un, ratio))
    # the inputs' condition: the threshold must stop a tenth of the work and still leave pixels that use the whole budget
    assert share <= 0.9 and full >= 0.05
    assert ratio <= 1.1 * MEASURED_RATIO[kind]
