"""Adaptive sampling on the MI355X (adaptivekernel.hip, api_adaptive.hip): a shortened order list renders exactly the active pixels
through the trace kernels as they are (every pixel holds the bits of a plain render of its own prefix of the seed list), threshold 0 is
moptix_render, every buffer and the stats are the CPU mirror's (tests/hostsim/adaptivesim.cpp) bit for bit, nothing else in the context changes,
state and argument errors, sub-passes under a small per-sample buffer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from common import M, K, REPO
from adaptive_helpers import AdaptiveSim

pytestmark = pytest.mark.gpu

# (scene, width, height, leaf_size, node_format, kernel_variant): the packet kernel on 64-byte and on 128-byte nodes, the queue kernel
# (what a launch this small picks for a triangle scene), and two scenes without triangles, where moptix_render plans the per-lane
# kernel (cornell_quads) or the lean queue kernel (random_spheres) -- the AOV / temporal GPU tests' scenes and sizes
CASES = [("file:coffee", 64, 36, 4, 64, 4), ("file:coffee", 61, 37, 1, 128, 4), ("file:coffee", 64, 36, 4, 0, -1),
         ("cornell_quads", 61, 37, 4, 0, -1), ("random_spheres", 64, 36, 4, 0, -1)]
USED = {("file:coffee", 4): 4, ("file:coffee", -1): 3, ("cornell_quads", -1): 3, ("random_spheres", -1): 3}
KW = dict(threshold=0.1, min_samples=8, batch=8)      # on 40 seeds: stops some pixels at 8, 16, 24, 32 and leaves others at 40 on every scene above
N_SEEDS = 40


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_bits(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = _bits(got) == _bits(want)
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:5].tolist())


def _restore(c):
    for name, v in (("leaf_size", 4), ("node_format", 0), ("kernel_variant", -1), ("tile_major", 3), ("drain_below", 64), ("sample_buffer_mb", 16384)):
        c.set_option(name, v)
    c.set_partition(0, 1)
    c.accum_bind(None)
    if c.width:
        c.adaptive_clear()      # the suite's other tests render into this context: leave no adaptive state behind


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    _restore(gpu_ctx)


@pytest.fixture
def other():
    c = M.Context(0)
    yield c
    c.close()


def _load(c, case):
    kind, w, h, leaf, fmt, variant = case
    hs = M.HostScene(kind, w, h)
    c.set_option("leaf_size", leaf); c.set_option("node_format", fmt); c.set_option("kernel_variant", variant)
    c.load(hs)
    return hs


def _snapshots(c, seeds, boundaries):
    """{count: accumulator of a plain render of seeds[:count]} at every pass boundary, the render continued from boundary to boundary."""
    c.accum_clear()
    snaps = {0: c.accum_read()}
    done = 0
    for b in boundaries:
        c.render(seeds[done:b]); done = b
        snaps[b] = c.accum_read()
    return snaps


def _pick(snaps, count):
    out = np.zeros(count.shape + (3,), np.float32)
    for k, img in snaps.items():
        out[count == k] = img[count == k]
    assert set(np.unique(count).tolist()) <= set(snaps)
    return out


# ---- 6: the hand-out mechanism ----
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-leaf%d-fmt%d-variant%d" % c)
def test_every_pixel_holds_the_bits_of_a_plain_render_of_its_prefix(ctx, other, case):
    seeds = M.launch_seeds(N_SEEDS, 2, 0)
    _load(ctx, case); _load(other, case)
    ctx.adaptive_clear()
    st = ctx.render_adaptive(seeds, **KW)
    assert ctx.get_option("kernel_variant_used") == USED[(case[0], case[5])]
    assert ctx.get_option("kernel_variant") == case[5] and ctx.get_option("tile_major") == 3      # as the caller set them
    r = ctx.adaptive_read()
    count = r["count"]
    print(case, st, dict(zip(*[x.tolist() for x in np.unique(count, return_counts=True)])))
    assert len(np.unique(count)) >= 2, "every pixel got the same number of samples: the case shows nothing"
    assert count.min() >= KW["min_samples"] and st["samples_traced"] == int(count.sum()) < st["samples_uniform"] == case[1] * case[2] * N_SEEDS
    snaps = _snapshots(other, seeds, list(range(KW["min_samples"], N_SEEDS, KW["batch"])) + [N_SEEDS])
    _assert_bits(ctx.accum_read(), _pick(snaps, count), case)


# ---- 7: threshold 0 is moptix_render ----
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-leaf%d-fmt%d-variant%d" % c)
def test_threshold_zero_is_moptix_render(ctx, other, case):
    seeds = M.launch_seeds(N_SEEDS, 5, 0)
    _load(ctx, case); _load(other, case)
    other.accum_clear(); other.render(seeds)
    want = other.accum_read()
    for drain in ((0, 64) if case[5] == 4 else (64,)):
        ctx.set_option("drain_below", drain)
        ctx.adaptive_clear()
        st = ctx.render_adaptive(seeds, threshold=0.0, min_samples=8, batch=8)
        _assert_bits(ctx.accum_read(), want, (case, drain))
        r = ctx.adaptive_read()
        assert (r["count"] == N_SEEDS).all() and not r["converged"].any()
        px = case[1] * case[2]
        assert st == dict(passes=5, samples_traced=px * N_SEEDS, samples_uniform=px * N_SEEDS, active_pixels_last=px, converged_pixels=0,
                          min_count=N_SEEDS, max_count=N_SEEDS)


# ---- 8: the CPU mirror's bits, fed with the GPU's own per-seed images ----
def _gpu_samples(c, seeds):
    out = []
    for s in seeds:
        c.accum_clear(); c.launch(int(s))
        out.append(c.accum_read())
    return np.stack(out)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-leaf%d-fmt%d-variant%d" % c)
def test_gpu_adaptive_is_the_cpu_mirrors_bits(ctx, other, case):
    kind, w, h = case[:3]
    seeds = M.launch_seeds(N_SEEDS, 9, 0)
    _load(ctx, case); _load(other, case)
    samples = _gpu_samples(other, seeds)
    sim = AdaptiveSim(w, h)
    ctx.adaptive_clear()
    # two calls (24 = 8 + 2 * 8 seeds, then the rest), other parameters in a third: the state carries over
    for part, kw in ((slice(0, 24), KW), (slice(24, 32), KW), (slice(32, N_SEEDS), dict(threshold=0.03, min_samples=4, batch=3))):
        got = ctx.render_adaptive(seeds[part], **kw)
        want = sim.render(samples[part], **kw)
        assert got == want, (case, part, got, want)
        r, m = ctx.adaptive_read(), sim.read()
        _assert_bits(ctx.accum_read(), m["accum"], (case, part, "accum"))
        _assert_bits(r["moments"], m["moments"], (case, part, "moments"))
        _assert_bits(r["error"], m["error"], (case, part, "error"))
        assert (r["count"] == m["count"]).all() and (r["converged"] == m["converged"]).all()
        mean, rgb8 = sim.mean()
        _assert_bits(ctx.adaptive_mean(), mean, (case, part, "mean"))
        assert (ctx.adaptive_resolve_rgb8() == rgb8).all()
    assert len(np.unique(sim.read()["count"])) >= 2


def test_adaptive_mean_into_a_tensor(ctx):
    import torch
    _load(ctx, CASES[2])
    ctx.adaptive_clear()
    ctx.render_adaptive(M.launch_seeds(24, 1, 0), **KW)
    t = torch.full((ctx.height, ctx.width, 3), -1.0, dtype=torch.float32, device=torch.device("cuda", 0))
    ctx.adaptive_mean_into(t)
    torch.cuda.synchronize()
    _assert_bits(t.cpu().numpy(), ctx.adaptive_mean())
    with pytest.raises(ValueError):
        ctx.adaptive_mean_into(t[:, :, :2])


# ---- 9: changes nothing else ----
def test_an_adaptive_call_changes_nothing_else(ctx, other):
    case = CASES[0]
    seeds = M.launch_seeds(16, 4, 0)
    _load(ctx, case); _load(other, case)
    ctx.set_option("tile_major", 1)
    ctx.aov_clear(); ctx.render_aovs(seeds[:4])
    ctx.accum_clear(); ctx.render(seeds[:4])
    den = ctx.denoise_temporal(4)
    aovs, tinfo, tread = ctx.aov_read(), ctx.temporal_info(), ctx.temporal_read()
    ctx.adaptive_clear()
    ctx.render_adaptive(M.launch_seeds(N_SEEDS, 2, 0), **KW)
    assert ctx.get_option("tile_major") == 1 and ctx.get_option("kernel_variant") == 4
    after = ctx.aov_read()
    for k in aovs:
        assert (aovs[k].view(np.uint32) == after[k].view(np.uint32)).all(), k
    assert ctx.aov_samples() == 4 and ctx.temporal_info() == tinfo
    t2 = ctx.temporal_read()
    _assert_bits(t2["motion"], tread["motion"]); _assert_bits(t2["history"], tread["history"])
    out = np.empty((ctx.height, ctx.width, 3), np.float32)
    ctx._chk(ctx._L.moptix_denoise_read(ctx._h, out.ctypes.data_as(C.POINTER(C.c_float))))
    _assert_bits(out, den)
    # after the clear a plain render gives the bits of a fresh context
    ctx.adaptive_clear()
    ctx.set_option("forget_history", 1)
    ctx.render(seeds)
    other.set_option("tile_major", 1)
    other.accum_clear(); other.render(seeds)
    _assert_bits(ctx.accum_read(), other.accum_read())
    assert ctx.get_option("kernel_variant_used") == other.get_option("kernel_variant_used")


# ---- 10: state and argument errors ----
def test_state_and_argument_errors(ctx):
    hs = _load(ctx, CASES[3])
    seeds = M.launch_seeds(8, 1, 0)

    def fails(code, f, *a, **kw):
        with pytest.raises(M.MoptixError) as e:
            f(*a, **kw)
        assert e.value.code == code, (e.value.code, str(e.value))

    ctx.adaptive_clear()
    for bad in (dict(threshold=-0.1), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(min_samples=0), dict(batch=0), dict(batch=-2)):
        fails(K.ERR_INVALID, ctx.render_adaptive, seeds, **bad)
    L = ctx._L
    p = K.AdaptiveParams(0.03, 16, 16)
    assert L.moptix_render_adaptive(ctx._h, None, 3, C.byref(p), None) == K.ERR_INVALID
    assert L.moptix_render_adaptive(ctx._h, None, 0, None, None) == K.ERR_INVALID
    assert L.moptix_adaptive_read(ctx._h, None) == K.ERR_INVALID
    assert L.moptix_adaptive_mean(ctx._h, None) == K.ERR_INVALID
    assert L.moptix_adaptive_mean_device(ctx._h, None) == K.ERR_INVALID
    assert L.moptix_adaptive_resolve_rgb8(ctx._h, None) == K.ERR_INVALID
    assert ctx.render_adaptive([], **KW)["passes"] == 0            # no seeds: nothing rendered, the totals of the cleared state
    assert not ctx.adaptive_read()["count"].any()
    # a tile split
    ctx.set_partition(1, 2)
    fails(K.ERR_STATE, ctx.render_adaptive, seeds, **KW)
    ctx.set_partition(0, 1)
    # plain render on adaptive state, and the reverse
    ctx.render_adaptive(seeds, **KW)
    fails(K.ERR_STATE, ctx.render, seeds)
    fails(K.ERR_STATE, ctx.launch, 1)
    fails(K.ERR_STATE, ctx.render_counted, seeds)
    ctx.render_adaptive(seeds, **KW)                               # continuing is fine
    assert ctx.adaptive_read()["count"].max() == 16
    ctx.adaptive_clear()
    ctx.render(seeds)
    fails(K.ERR_STATE, ctx.render_adaptive, seeds, **KW)
    ctx.accum_clear()                                              # drops the adaptive state with the buffer
    fails(K.ERR_STATE, ctx.adaptive_read)
    ctx.render_adaptive(seeds, **KW)
    assert ctx.adaptive_read()["count"].max() == 8
    ctx.accum_clear()
    ctx.render(seeds)                                              # allowed again
    # the collectives' device halves write samples without counts into the accumulator, too
    import torch
    ctx.adaptive_clear()
    packed = torch.zeros(ctx.packed_tile_floats(1), dtype=torch.float32, device=torch.device("cuda", 0))
    ctx.unpack_tiles(0, 1, packed.data_ptr())
    fails(K.ERR_STATE, ctx.render_adaptive, seeds, **KW)
    ctx.adaptive_clear()
    with pytest.raises(ValueError):
        ctx.adaptive_mean_into(torch.zeros((ctx.height, ctx.width, 3), dtype=torch.float32))      # a CPU tensor
    # a frame-size change drops the state
    ctx.adaptive_clear(); ctx.render_adaptive(seeds, **KW)
    p2 = K.Params.from_buffer_copy(hs.params); p2.width, p2.height = 40, 24
    ctx.set_params(p2)
    fails(K.ERR_STATE, ctx.adaptive_read)
    fails(K.ERR_STATE, ctx.adaptive_mean)
    st = ctx.render_adaptive(seeds, threshold=0.0)
    assert st["samples_traced"] == 40 * 24 * 8 and ctx.adaptive_read()["count"].shape == (24, 40)
    ctx.set_params(hs.params)


# ---- 11: sub-passes ----
def test_a_small_sample_buffer_cuts_the_passes_and_keeps_the_bits(ctx, other):
    case = ("file:coffee", 480, 270, 4, 0, -1)
    seeds = M.launch_seeds(24, 2, 0)
    _load(ctx, case); _load(other, case)
    # 480 x 270 = 129,600 pixels -> 130,560 slots x 12 bytes = 1.49 MB per seed: 4 MB hold two seeds, so a pass of 8 runs as 2 + 2 + 2 + 2
    ctx.set_option("sample_buffer_mb", 4)
    ctx.adaptive_clear()
    ctx.kernel_time(reset=True)
    st = ctx.render_adaptive(seeds, **KW)
    assert st["passes"] == 3 and ctx.kernel_time()[1] == 12
    count = ctx.adaptive_read()["count"]
    assert len(np.unique(count)) >= 2
    snaps = _snapshots(other, seeds, [8, 16, 24])
    _assert_bits(ctx.accum_read(), _pick(snaps, count))


# ---- 12: the CLI and the host ABI ----
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


@pytest.mark.timeout(600)
def test_cli_adaptive_writes_what_the_python_path_computes(ctx, tmp_path):
    import torch
    w, h, spp = 96, 54, N_SEEDS
    exe = os.path.join(REPO, "minimaloptix_amd", "lib", "moptix_render")
    base = [exe, "--scene", "coffee", "--spp", str(spp), "--width", str(w), "--height", str(h), "--scenes", M.scenes_dir(), "--outdir", str(tmp_path),
            "--adaptive", str(KW["threshold"]), "--adaptive-min", str(KW["min_samples"]), "--adaptive-batch", str(KW["batch"])]
    p = subprocess.run(base + ["--out", "f", "--aov", "--denoise"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    # the Python path
    hs = M.HostScene("file:coffee", w, h)
    seeds = M.launch_seeds(spp)
    ctx.load(hs)
    ctx.adaptive_clear()
    st = ctx.render_adaptive(seeds, **KW)
    r = ctx.adaptive_read()
    assert len(np.unique(r["count"])) >= 2
    assert np.array_equal(_read_png(str(tmp_path / "f.png")), ctx.adaptive_resolve_rgb8())
    _assert_bits(_read_pfm(str(tmp_path / "f_count.pfm"), w, h), np.repeat(r["count"].astype(np.float32)[..., None], 3, axis=2), "count")
    _assert_bits(_read_pfm(str(tmp_path / "f_error.pfm"), w, h), np.repeat(r["error"][..., None], 3, axis=2), "error")
    line = [l for l in p.stderr.splitlines() if l.startswith("adaptive:")]
    assert len(line) == 1 and ("%d passes, %d of %d samples traced" % (st["passes"], st["samples_traced"], st["samples_uniform"])) in line[0], p.stderr[-2000:]
    assert ("%d pixels active and %d converged" % (st["active_pixels_last"], st["converged_pixels"])) in line[0]
    for name in ("albedo", "normal", "depth"):
        assert os.path.exists(tmp_path / ("f_%s.pfm" % name))
    # --denoise: the per-pixel mean, bound as the accumulator of a denoise call that divides by 1
    mean = torch.zeros((h, w, 3), dtype=torch.float32, device=torch.device("cuda", 0))
    ctx.adaptive_mean_into(mean)
    ctx.accum_bind(mean.data_ptr())
    ctx.aov_clear(); ctx.render_aovs(seeds)
    want = ctx.denoise(1.0)
    ctx.accum_bind(None)
    _assert_bits(_read_pfm(str(tmp_path / "f_denoised.pfm"), w, h), want, "denoised")
    # the host ABI: the same render as arrays
    canvas = np.zeros((h, w, 3), np.uint8); count = np.zeros((h, w), np.uint32); error = np.zeros((h, w), np.float32)
    hst = K.AdaptiveStats()
    q = K.AdaptiveParams(KW["threshold"], KW["min_samples"], KW["batch"])
    rc = K.host_lib().mohost_render_scene_adaptive(0, 1, M.scenes_dir().encode(), w, h, spp, 0, C.byref(q), canvas.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                    count.ctypes.data_as(C.POINTER(C.c_uint32)), error.ctypes.data_as(C.POINTER(C.c_float)), C.byref(hst))
    assert rc == K.MOPTIX_OK, K.host_lib().mohost_last_error()
    assert hst.as_dict() == st and (count == r["count"]).all()
    _assert_bits(error, r["error"], "host ABI error")
    assert np.array_equal(canvas, _read_png(str(tmp_path / "f.png")))
    # one rank, one image
    for extra in (["--spawn", "2"], ["--ranks", "2", "--rank", "0", "--comm-file", str(tmp_path / "id")], ["--video-frames", "1"], ["--autosave"]):
        e = subprocess.run(base + ["--out", "g"] + extra, capture_output=True, text=True, timeout=60)
        assert e.returncode == 2 and "--adaptive" in e.stderr, (extra, e.returncode, e.stderr[-500:])
    bad = subprocess.run(base[:-6] + ["--adaptive", "-1", "--out", "g"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "threshold" in bad.stderr, bad.stderr[-500:]
