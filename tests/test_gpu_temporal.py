"""Temporal accumulation on the MI355X (temporalkernel.hip): output, motion vectors, history lengths and counters bit for bit the CPU
mirror of the kernels' code (tests/hostsim/temporalsim.cpp) over moving sequences and on synthetic inputs, the anchor to Context.denoise, no
effect on anything else the context holds, binding, state errors, the history's life."""
import ctypes as C

import numpy as np
import pytest

from common import M, K, textured_scene
from temporal_helpers import TEMPORAL_DEFAULTS, TemporalSim, cam_of, centres_of, copy_spheres, moved_camera, sphere_array
from denoise_helpers import synthetic_aovs

pytestmark = pytest.mark.gpu

AOV_IN = ("albedo", "normal", "depth", "hits", "primId", "matId")
SETTINGS = [dict(), dict(iterations=1, normal_power=7, demodulate=True), dict(iterations=0),
            dict(iterations=3, normal_power=256, demodulate=True, sigma_luminance=0.0, sigma_depth=0.0)]
TEMPORALS = [None, dict(alpha=0.0, alpha_moments=0.5, depth_tolerance=0.05, normal_threshold=0.9, max_history=3, variance_frames=2)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_bits(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = _bits(got) == _bits(want)
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:5].tolist())


def _assert_info(got, want, what=""):
    assert {k: v for k, v in got.items() if k != "mean_history"} == {k: v for k, v in want.items() if k != "mean_history"}, (what, got, want)
    assert np.float32(got["mean_history"]) == np.float32(want["mean_history"]), (what, got, want)


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0); gpu_ctx.set_partition(0, 1)
    gpu_ctx.aov_bind(None); gpu_ctx.accum_bind(None); gpu_ctx.denoise_bind(None)


def _frame(ctx, seeds):
    ctx.accum_clear(); ctx.render(seeds)
    ctx.aov_clear(); ctx.render_aovs(seeds)
    return ctx.accum_read(), ctx.aov_read(), ctx.aov_samples()


def _check_call(ctx, sim, accum, aovs, s, n_acc, cam, centres, temporal, kw, what):
    got = ctx.denoise_temporal(n_acc, temporal=temporal, **kw)
    want = sim.run(accum, aovs, n_acc, s, cam, centres, temporal=temporal, **kw)
    _assert_bits(got, want["out"], (what, "out"))
    r = ctx.temporal_read()
    _assert_bits(r["motion"], want["motion"], (what, "motion"))
    _assert_bits(r["history"], want["history"], (what, "history"))
    _assert_info(ctx.temporal_info(), want["info"], what)
    return want


# the AOV tests' scene / size grid (tests/test_gpu_aov.py CASES) under a camera that moves a little every frame
CASES = [("spheres", 64, 36, 1, 4, 64), ("cornell_quads", 64, 36, 7, 4, 64), ("file:coffee", 64, 36, 1, 4, 64), ("file:coffee", 64, 36, 7, 1, 128),
         ("file:coffee", 61, 37, 7, 4, 128), ("file:coffee", 61, 37, 1, 1, 64), ("textured", 64, 36, 7, 4, 64), ("textured", 61, 37, 1, 1, 128),
         ("random_spheres", 61, 37, 7, 4, 64), ("file:coffee", 480, 270, 2, 4, 64)]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind,w,h,nseeds,leaf,fmt", CASES)
def test_gpu_temporal_is_the_cpu_mirrors_bits_on_moving_sequences(ctx, tmp_path, kind, w, h, nseeds, leaf, fmt):
    hs = textured_scene(tmp_path, w, h) if kind == "textured" else M.HostScene(kind, w, h)
    ctx.set_option("leaf_size", leaf); ctx.set_option("node_format", fmt)
    ctx.load(hs)
    sph, n = sphere_array(hs)
    centres = centres_of(sph, n)
    for ti, temporal in enumerate(TEMPORALS):
        for kw in (SETTINGS if ti == 0 else SETTINGS[:2]):
            ctx.temporal_reset()
            sim = TemporalSim()
            reprojected = 0
            for k in range(5):
                # frames 0-1 move, frame 2 repeats frame 1's camera (the static shortcut), 3-4 move on
                j = k if k < 2 else k - 1
                p = moved_camera(hs.params, (0.01 * j, -0.006 * j, 0.004 * j))
                ctx.set_params(p)
                accum, aovs, s = _frame(ctx, M.launch_seeds(nseeds, 5, 50 * k))
                want = _check_call(ctx, sim, accum, aovs, s, nseeds, cam_of(p), centres, temporal, kw, (kind, kw, temporal, k))
                reprojected += want["info"]["history_pixels"]
            assert reprojected > 0 or not (aovs["hits"] > 0).any()
    ctx.set_params(hs.params)


@pytest.mark.timeout(600)
def test_gpu_temporal_is_the_cpu_mirrors_bits_on_video_frames(ctx):
    """updateVideo's steps: the spheres move, the camera orbits."""
    w, h = 160, 90
    hs = M.HostScene("random_spheres", w, h, iarg=60)
    ctx.load(hs)
    sph, n = sphere_array(hs)
    angle = C.c_float(0.0)
    sim = TemporalSim()
    moved = 0
    for k in range(5):
        K.host_lib().mohost_animate_spheres(sph, n, 0.002, C.byref(angle))
        p = K.Params.from_buffer_copy(hs.params)
        K.host_lib().mohost_video_camera(angle.value, w / h, C.byref(p.cam))
        ctx.update_spheres(0, sph, n)
        ctx.set_params(p)
        accum, aovs, s = _frame(ctx, M.launch_seeds(4, 0, 100 * k))
        want = _check_call(ctx, sim, accum, aovs, s, 4, cam_of(p), centres_of(copy_spheres(sph, n), n), None, dict(), k)
        moved += int((want["motion"] != 0).any(axis=-1).sum())
        if k > 0:
            assert want["info"]["history_pixels"] > 0.5 * want["info"]["geometry_pixels"]
    assert moved > 0


def _bind_synthetic(ctx, h, w, n_samples=3):
    import torch
    dev = torch.device("cuda", 0)
    hs = M.HostScene("cornell_quads", w, h)
    ctx.load(hs)
    acc_t = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    aov_t = {n: torch.zeros((h, w, 3 if n in ("albedo", "normal") else 1), dtype=torch.int32 if n in ("primId", "matId") else torch.float32, device=dev)
             for n in AOV_IN}
    torch.cuda.synchronize()
    ctx.accum_bind(acc_t.data_ptr())
    ctx.aov_bind(aov_t)
    ctx.aov_clear()
    ctx.render_aovs(M.launch_seeds(n_samples))
    assert ctx.aov_samples() == n_samples

    def fill(accum, aovs):
        acc_t.copy_(torch.from_numpy(np.ascontiguousarray(accum, np.float32)))
        for n in AOV_IN:
            a = np.ascontiguousarray(aovs[n], np.int32 if n in ("primId", "matId") else np.float32).reshape(aov_t[n].shape)
            aov_t[n].copy_(torch.from_numpy(a))
        torch.cuda.synchronize()                 # the copies are on torch's stream, the library works on its own
    return fill, n_samples, hs


@pytest.mark.timeout(300)
@pytest.mark.parametrize("h,w,background", [(37, 61, 0.25), (37, 61, 1.0), (1, 1, 0.0), (1, 8, 0.0), (8, 1, 0.0), (90, 160, 0.25)])
def test_gpu_temporal_is_the_cpu_mirrors_bits_on_synthetic_inputs(ctx, h, w, background):
    fill, s, hs = _bind_synthetic(ctx, h, w)
    rng = np.random.RandomState(h * 7 + w)
    for temporal in TEMPORALS:
        for kw in SETTINGS[:3]:
            ctx.temporal_reset()
            sim = TemporalSim()
            for k in range(4):
                accum, aovs, _ = synthetic_aovs(h, w, seed=h * 131 + w, background=background, n_samples=s)
                accum = (accum * (0.7 + 0.6 * rng.rand(h, w, 1))).astype(np.float32)
                geo = aovs["hits"][..., 0] > 0
                yy, xx = np.mgrid[0:h, 0:w]
                aovs["primId"] = np.where(geo, 3 + (xx % 2), -1).astype(np.int32)        # ids far outside the scene's spheres as well
                aovs["matId"] = np.where(geo, (xx * 3) // max(w, 1), -1).astype(np.int32)
                fill(accum, aovs)
                p = moved_camera(hs.params, (0.003 * k, 0.002 * k, 0.0))
                ctx.set_params(p)
                _check_call(ctx, sim, accum, aovs, s, 2.0, cam_of(p), None, temporal, kw, (kw, temporal, k))


@pytest.mark.timeout(300)
def test_first_call_is_context_denoise_and_the_history_drops(ctx):
    hs = M.HostScene("spheres", 64, 36)
    ctx.load(hs)
    accum, aovs, s = _frame(ctx, M.launch_seeds(3))
    for kw in SETTINGS:
        ctx.temporal_reset()
        _assert_bits(ctx.denoise_temporal(3, **kw), ctx.denoise(3, **kw), kw)
        assert ctx.temporal_info()["frames"] == 1 and ctx.temporal_info()["history_pixels"] == 0
    spatial = ctx.denoise(3)

    def first_frame():
        out = ctx.denoise_temporal(3)
        i = ctx.temporal_info()
        return i["frames"] == 1 and i["history_pixels"] == 0 and np.array_equal(_bits(out), _bits(spatial))
    ctx.temporal_reset()
    assert first_frame() and not first_frame()            # the second call has history
    ctx.temporal_reset()
    assert first_frame()
    ctx.denoise_temporal(3, demodulate=True)              # a change of demodulation
    assert ctx.temporal_info()["frames"] == 1
    assert first_frame()
    ctx.denoise_temporal(3, iterations=0)
    assert ctx.temporal_info()["frames"] == 2             # demodulate = 0 in effect before and after
    ctx.load(hs)                                          # moptix_clear_scene
    _frame(ctx, M.launch_seeds(3))
    assert first_frame()
    # a frame-size change: MOPTIX_ERR_STATE until AOVs are rendered again, then a first frame
    prm = K.Params.from_buffer_copy(hs.params)
    prm.width, prm.height = 48, 30
    ctx.set_params(prm)
    for call in (lambda: ctx.denoise_temporal(3), ctx.temporal_read):
        with pytest.raises(M.MoptixError) as e:
            call()
        assert e.value.code == K.ERR_STATE
    ctx.render_aovs(M.launch_seeds(1))
    assert ctx.denoise_temporal(1).shape == (30, 48, 3) and ctx.temporal_info()["frames"] == 1
    assert ctx.temporal_read()["history"].shape == (30, 48)
    # a different sphere count
    ctx.denoise_temporal(1)
    assert ctx.temporal_info()["frames"] == 2
    other = M.HostScene("cornell_quads", 48, 30)
    ctx.load(other)
    ctx.aov_clear(); ctx.render_aovs(M.launch_seeds(1))
    ctx.denoise_temporal(1)
    assert ctx.temporal_info()["frames"] == 1


@pytest.mark.timeout(300)
def test_temporal_denoising_changes_nothing_else(ctx):
    hs = M.HostScene("file:coffee", 160, 90)
    seeds, more = M.launch_seeds(4), M.launch_seeds(2, 0, 4)
    ctx.set_option("kernel_variant", 4)
    try:
        frames = {}
        for with_denoise in (False, True):
            ctx.load(hs)
            ctx.accum_clear()
            ctx.kernel_time(reset=True)
            ctx.render(seeds)
            ctx.aov_clear()
            ctx.render_aovs(seeds)
            if with_denoise:
                before = (ctx.accum_read(), ctx.aov_read(), ctx.aov_samples(), ctx.kernel_time(), ctx.reduce_time(), ctx.get_option("node_format_used"))
                for _ in range(2):
                    assert np.isfinite(ctx.denoise_temporal(4)).all()
                after = (ctx.accum_read(), ctx.aov_read(), ctx.aov_samples(), ctx.kernel_time(), ctx.reduce_time(), ctx.get_option("node_format_used"))
                _assert_bits(after[0], before[0], "accum")
                for n in AOV_IN:
                    assert np.array_equal(_bits(after[1][n]), _bits(before[1][n])), n
                assert after[2:] == before[2:]
            ctx.render(more)
            frames[with_denoise] = (ctx.accum_read(), ctx.kernel_time()[1], ctx.get_option("node_format_used"))
        _assert_bits(frames[True][0], frames[False][0], "beauty after the temporal denoiser")
        assert frames[True][1:] == frames[False][1:]
    finally:
        ctx.set_option("kernel_variant", -1)


@pytest.mark.timeout(300)
def test_binding_state_errors_and_bad_parameters(ctx):
    import torch
    with pytest.raises(M.MoptixError) as e:
        ctx.denoise_temporal(1)
    assert e.value.code == K.ERR_STATE                    # no params yet
    hs = M.HostScene("file:coffee", 61, 37)
    ctx.load(hs)
    with pytest.raises(M.MoptixError) as e:
        ctx.denoise_temporal(1)
    assert e.value.code == K.ERR_STATE                    # no AOV samples
    with pytest.raises(M.MoptixError) as e:
        ctx.temporal_read()
    assert e.value.code == K.ERR_STATE
    assert ctx.temporal_info() == dict(frames=0, geometry_pixels=0, history_pixels=0, disoccluded_pixels=0, mean_history=0.0)
    _frame(ctx, M.launch_seeds(3))
    own = ctx.denoise_temporal(3)
    t = torch.full((37, 61, 3), 7.0, dtype=torch.float32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.denoise_bind(t)
    ctx.temporal_reset()
    assert np.array_equal(_bits(ctx.denoise_temporal(3)), _bits(own))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(own))
    ctx.denoise_bind(None)
    for temporal in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha_moments=float("nan")), dict(depth_tolerance=-1.0), dict(depth_tolerance=float("inf")),
                     dict(normal_threshold=1.5), dict(normal_threshold=-2.0), dict(max_history=0), dict(variance_frames=0), dict(max_history=1 << 20)):
        with pytest.raises(M.MoptixError) as e:
            ctx.denoise_temporal(3, temporal=temporal)
        assert e.value.code == K.ERR_INVALID, temporal
    for kw in (dict(iterations=-1), dict(iterations=9), dict(normal_power=0), dict(sigma_luminance=float("nan"))):
        with pytest.raises(M.MoptixError) as e:
            ctx.denoise_temporal(3, **kw)
        assert e.value.code == K.ERR_INVALID, kw
    for n in (0.0, -1.0, float("nan")):
        with pytest.raises(M.MoptixError) as e:
            ctx.denoise_temporal(n)
        assert e.value.code == K.ERR_INVALID, n
    with pytest.raises(ValueError):
        ctx.denoise_temporal(3, temporal=dict(nonsense=1))
    assert ctx.temporal_defaults() == {k: pytest.approx(v) for k, v in TEMPORAL_DEFAULTS.items()}


def _read_pfm(path, w, h):
    with open(path, "rb") as f:
        assert f.readline() == b"PF\n" and f.readline() == ("%d %d\n" % (w, h)).encode() and f.readline() == b"-1.0\n"
        return np.frombuffer(f.read(), np.float32).reshape(h, w, 3)


@pytest.mark.timeout(300)
def test_cli_video_frames_with_temporal_denoising(ctx, tmp_path):
    """moptix_render --video-frames 2 --denoise-temporal: the files of both steps exist, step 0's denoised image is the spatial denoiser's
    (the history's first frame), step 1's is the temporal entry's second call and not the spatial denoiser's."""
    import os
    import subprocess
    from common import REPO
    w, h, spp, L = 96, 54, 3, 3
    exe = os.path.join(REPO, "minimaloptix_amd", "lib", "moptix_render")
    base = [exe, "--scene", "random_spheres_256", "--spp", str(spp), "--width", str(w), "--height", str(h), "--scenes", M.scenes_dir(),
            "--outdir", str(tmp_path), "--out", "f"]
    p = subprocess.run(base + ["--video-frames", "2", "--denoise-temporal", "--denoise-iterations", str(L)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    for name in ("f.png", "f_video0.png", "f_video1.png", "f_video0_denoised.pfm", "f_video0_denoised.png", "f_video1_denoised.pfm",
                 "f_video1_denoised.png"):
        assert os.path.exists(tmp_path / name), name
    assert not os.path.exists(tmp_path / "f_denoised.pfm")
    # the same steps through the Python interface
    hs = M.HostScene("random_spheres", w, h, iarg=256)
    ctx.load(hs)
    sph, n = sphere_array(hs)
    angle = C.c_float(0.0)
    for k in range(2):
        K.host_lib().mohost_animate_spheres(sph, n, 0.002, C.byref(angle))
        prm = K.Params.from_buffer_copy(hs.params)
        K.host_lib().mohost_video_camera(angle.value, w / h, C.byref(prm.cam))
        ctx.update_spheres(0, sph, n)
        ctx.set_params(prm)
        _frame(ctx, M.launch_seeds(spp, 0, spp * (k + 1)))           # the frame itself took the first spp seeds
        temporal = ctx.denoise_temporal(spp, iterations=L)
        spatial = ctx.denoise(spp, iterations=L)
        got = _read_pfm(str(tmp_path / ("f_video%d_denoised.pfm" % k)), w, h)
        _assert_bits(got, temporal, ("PFM", k))
        if k == 0:
            _assert_bits(got, spatial, "step 0 is a first frame")
        else:
            assert not np.array_equal(_bits(got), _bits(spatial))
            assert ctx.temporal_info()["history_pixels"] > 0
    # without the new flags the frame's own file is what it was; the flags' misuse is an error that names the reason
    q = subprocess.run(base[:-1] + ["g"], capture_output=True, text=True, timeout=240)
    assert q.returncode == 0 and open(tmp_path / "g.png", "rb").read() == open(tmp_path / "f.png", "rb").read()
    assert sorted(x for x in os.listdir(tmp_path) if x.startswith("g")) == ["g.png"]
    for extra, word in ((["--video-frames", "2", "--ranks", "2", "--rank", "0", "--comm-file", str(tmp_path / "id")], "one rank"),
                        (["--video-frames", "2", "--spawn", "2"], "one rank"), (["--denoise-temporal"], "--video-frames"),
                        (["--scene", "spheres", "--video-frames", "1"], "random_spheres_256")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr[-500:])
