"""The denoiser on the MI355X (denoisekernel.hip): bit for bit the CPU mirror of the kernels' code (tests/hostsim/denoisesim.cpp) on rendered and on
synthetic inputs, no effect on anything else the context holds, binding, state errors and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from common import M, K, REPO, textured_scene
from denoise_helpers import DEFAULTS, denoisesim, synthetic_aovs

pytestmark = pytest.mark.gpu

AOV_IN = ("albedo", "normal", "depth", "hits")
SETTINGS = [DEFAULTS, dict(iterations=1, normal_power=7, demodulate=True), dict(iterations=8, normal_power=1, sigma_luminance=0.5, sigma_depth=3.0),
            dict(iterations=3, normal_power=256, demodulate=True, sigma_luminance=0.0, sigma_depth=0.0), dict(iterations=0)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_bits(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = _bits(got) == _bits(want)
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same.all(axis=-1))[:5].tolist())


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0); gpu_ctx.set_partition(0, 1)
    gpu_ctx.aov_bind(None); gpu_ctx.accum_bind(None); gpu_ctx.denoise_bind(None)


def _render(ctx, hs, seeds, leaf=4, fmt=0):
    """beauty + AOVs of the same seeds; returns (accum, aovs, aov_samples) as read back"""
    ctx.set_option("leaf_size", leaf)
    ctx.set_option("node_format", fmt)
    ctx.load(hs)
    ctx.accum_clear()
    ctx.render(seeds)
    ctx.aov_clear()
    ctx.render_aovs(seeds)
    return ctx.accum_read(), ctx.aov_read(), ctx.aov_samples()


# the AOV tests' scene / size grid (tests/test_gpu_aov.py CASES) and the benchmark frame
CASES = [("spheres", 64, 36, 1, 4, 64), ("cornell_quads", 64, 36, 7, 4, 64), ("file:coffee", 64, 36, 1, 4, 64), ("file:coffee", 64, 36, 7, 1, 128),
         ("file:coffee", 61, 37, 7, 4, 128), ("file:coffee", 61, 37, 1, 1, 64), ("textured", 64, 36, 7, 4, 64), ("textured", 61, 37, 1, 1, 128),
         ("random_spheres", 61, 37, 7, 4, 64), ("file:coffee", 1920, 1080, 4, 4, 64)]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind,w,h,nseeds,leaf,fmt", CASES)
def test_gpu_denoiser_is_the_cpu_mirrors_bits_on_rendered_frames(ctx, tmp_path, kind, w, h, nseeds, leaf, fmt):
    hs = textured_scene(tmp_path, w, h) if kind == "textured" else M.HostScene(kind, w, h)
    accum, aovs, s = _render(ctx, hs, M.launch_seeds(nseeds, 5), leaf, fmt)
    assert s == nseeds and (aovs["hits"] > 0).any()
    for kw in (SETTINGS if w * h < 100000 else SETTINGS[:2]):
        _assert_bits(ctx.denoise(nseeds, **kw), denoisesim(accum, aovs, nseeds, s, **kw), kw)


def _bind_synthetic(ctx, h, w, n_samples=3):
    """A context whose accumulation buffer and AOVs are torch tensors, with aov_samples == n_samples (rendered into them, then
    overwritten); returns (fill, n_samples), fill(accum, aovs) writing host arrays into the bound tensors."""
    import torch
    dev = torch.device("cuda", 0)
    hs = M.HostScene("cornell_quads", w, h)
    ctx.load(hs)
    acc_t = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    aov_t = {n: torch.zeros((h, w, 3 if n in ("albedo", "normal") else 1), dtype=torch.float32, device=dev) for n in AOV_IN}
    torch.cuda.synchronize()
    ctx.accum_bind(acc_t.data_ptr())
    ctx.aov_bind(aov_t)
    ctx.aov_clear()
    ctx.render_aovs(M.launch_seeds(n_samples))
    assert ctx.aov_samples() == n_samples

    def fill(accum, aovs):
        acc_t.copy_(torch.from_numpy(np.ascontiguousarray(accum, np.float32)))
        for n in AOV_IN:
            aov_t[n].copy_(torch.from_numpy(np.ascontiguousarray(aovs[n], np.float32)))
        torch.cuda.synchronize()                 # the copies are on torch's stream, the library works on its own
    return fill, n_samples


def _synthetic(kind, h, w, s):
    accum, aovs, _ = synthetic_aovs(h, w, seed=h * 131 + w, background=1.0 if kind in ("all_background", "single_pixel") else 0.25, n_samples=s)
    if kind == "single_pixel":
        aovs["hits"][h // 2, w // 2] = s
        aovs["depth"][h // 2, w // 2] = 2.5 * s
        aovs["normal"][h // 2, w // 2] = np.float32([0, 0, s])
    if kind == "zero_albedo":
        aovs["albedo"][:] = 0
    return accum, aovs


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind,h,w", [("random", 37, 61), ("all_background", 37, 61), ("single_pixel", 37, 61), ("zero_albedo", 37, 61),
                                      ("random", 1, 1), ("random", 1, 8), ("random", 8, 1), ("random", 90, 160)])
def test_gpu_denoiser_is_the_cpu_mirrors_bits_on_synthetic_inputs(ctx, kind, h, w):
    fill, s = _bind_synthetic(ctx, h, w)
    accum, aovs = _synthetic(kind, h, w, s)
    fill(accum, aovs)
    for kw in SETTINGS:
        got = ctx.denoise(2.0, **kw)
        want = denoisesim(accum, aovs, 2.0, s, **kw)
        _assert_bits(got, want, (kind, kw))
        if kind == "all_background":
            _assert_bits(got, accum / np.float32(2.0))


@pytest.mark.timeout(300)
def test_denoising_changes_nothing_else(ctx):
    hs = M.HostScene("file:coffee", 160, 90)
    seeds, more = M.launch_seeds(4), M.launch_seeds(2, 0, 4)
    ctx.set_option("kernel_variant", 4)
    try:
        frames = {}
        for with_denoise in (False, True):
            ctx.load(hs)                         # new build: same depth history and node-format verdict for both runs
            ctx.accum_clear()
            ctx.kernel_time(reset=True)
            ctx.render(seeds)
            ctx.aov_clear()
            ctx.render_aovs(seeds)
            if with_denoise:
                before = (ctx.accum_read(), ctx.aov_read(), ctx.aov_samples(), ctx.kernel_time(), ctx.reduce_time(), ctx.get_option("node_format_used"))
                out = ctx.denoise(4)
                assert np.isfinite(out).all()
                after = (ctx.accum_read(), ctx.aov_read(), ctx.aov_samples(), ctx.kernel_time(), ctx.reduce_time(), ctx.get_option("node_format_used"))
                _assert_bits(after[0], before[0], "accum")
                for n in ("albedo", "normal", "depth", "hits", "primId", "matId"):
                    assert np.array_equal(_bits(after[1][n]), _bits(before[1][n])), n
                assert after[2:] == before[2:]
            ctx.render(more)
            frames[with_denoise] = (ctx.accum_read(), ctx.kernel_time()[1], ctx.get_option("node_format_used"))
        _assert_bits(frames[True][0], frames[False][0], "beauty after the denoiser")
        assert frames[True][1:] == frames[False][1:]
    finally:
        ctx.set_option("kernel_variant", -1)


@pytest.mark.timeout(300)
def test_binding_resize_and_bad_parameters(ctx):
    import torch
    hs = M.HostScene("file:coffee", 61, 37)
    _render(ctx, hs, M.launch_seeds(3))
    own = ctx.denoise(3)
    t = torch.full((37, 61, 3), 7.0, dtype=torch.float32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.denoise_bind(t)
    assert np.array_equal(_bits(ctx.denoise(3)), _bits(own))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(own))
    ctx.denoise_bind(None)
    t.fill_(7.0); torch.cuda.synchronize()
    assert np.array_equal(_bits(ctx.denoise(3)), _bits(own))
    assert (t.cpu().numpy() == 7.0).all()
    with pytest.raises(ValueError):
        ctx.denoise_bind(torch.zeros((37, 61, 2), dtype=torch.float32, device=torch.device("cuda", 0)))
    # bad parameters
    for kw in (dict(iterations=-1), dict(iterations=9), dict(normal_power=0), dict(normal_power=257), dict(sigma_luminance=float("nan")),
               dict(sigma_depth=float("inf")), dict(sigma_luminance=-1.0)):
        with pytest.raises(M.MoptixError) as e:
            ctx.denoise(3, **kw)
        assert e.value.code == K.ERR_INVALID, kw
    for n in (0.0, -1.0, float("nan")):
        with pytest.raises(M.MoptixError) as e:
            ctx.denoise(n)
        assert e.value.code == K.ERR_INVALID, n
    p = K.DenoiseParams(5, 128, 2, 4.0, 1.0)
    assert K.device_lib().moptix_denoise(ctx._h, C.byref(p), 1.0) == K.ERR_INVALID
    # a frame-size change: MOPTIX_ERR_STATE until AOVs are rendered again
    prm = hs.params
    prm.width, prm.height = 48, 30
    ctx.set_params(prm)
    for call in (lambda: ctx.denoise(3), lambda: ctx.denoise(3, iterations=0)):
        with pytest.raises(M.MoptixError) as e:
            call()
        assert e.value.code == K.ERR_STATE
    ctx.render_aovs(M.launch_seeds(1))
    assert ctx.denoise(1).shape == (30, 48, 3)


def _read_pfm(path, w, h):
    with open(path, "rb") as f:
        assert f.readline() == b"PF\n" and f.readline() == ("%d %d\n" % (w, h)).encode() and f.readline() == b"-1.0\n"
        return np.frombuffer(f.read(), np.float32).reshape(h, w, 3)


def _read_png(path):
    w, h = C.c_int32(), C.c_int32()
    L = K.host_lib()
    assert L.mohost_read_image(path.encode(), C.byref(w), C.byref(h), None, 0) == K.MOPTIX_OK, L.mohost_last_error()
    px = np.zeros((h.value, w.value, 3), np.uint8)
    assert L.mohost_read_image(path.encode(), C.byref(w), C.byref(h), px.ctypes.data_as(C.POINTER(C.c_uint8)), px.size) == K.MOPTIX_OK
    return px


@pytest.mark.timeout(300)
@pytest.mark.parametrize("iterations", [None, 3])
def test_cli_denoise_writes_what_context_denoise_computes(ctx, tmp_path, iterations):
    w, h, spp = 96, 54, 3
    exe = os.path.join(REPO, "minimaloptix_amd", "lib", "moptix_render")
    args = [exe, "--scene", "coffee", "--spp", str(spp), "--denoise", "--width", str(w), "--height", str(h), "--scenes", M.scenes_dir(),
            "--outdir", str(tmp_path), "--out", "f"]
    if iterations is not None:
        args += ["--denoise-iterations", str(iterations)]
    p = subprocess.run(args, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    got = _read_pfm(str(tmp_path / "f_denoised.pfm"), w, h)
    hs = M.HostScene("file:coffee", w, h)
    seeds = M.launch_seeds(spp)
    _render(ctx, hs, seeds)
    want = ctx.denoise(spp, iterations=5 if iterations is None else iterations)
    _assert_bits(got, want, "PFM")
    v = np.clip(want, 0.0, 1.0)
    rgb8 = (((v * np.float32(65535.0) + np.float32(0.5)).astype(np.uint32)) >> 8).astype(np.uint8)[::-1]
    assert np.array_equal(_read_png(str(tmp_path / "f_denoised.png")), rgb8)
    assert os.path.exists(tmp_path / "f.png")            # the beauty frame is still written, unchanged by the denoiser
