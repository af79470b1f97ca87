"""Per-face motion in the temporal stage on the MI355X (facemotionkernel.hip, temporalkernel.hip's k_tp_reproject<true>): output,
motion vectors, history lengths and both sets of counters bit for bit the CPU mirror of the whole call (tests/hostsim/temporalsim.cpp) on moving
and deforming meshes, over the face counts at the wave and workgroup tails, with the option off (today's bits), on static frames,
no effect on anything else the context holds, and the argument errors."""
import ctypes as C

import numpy as np
import pytest

from common import M, K
from temporal_helpers import TemporalSim, cam_of, moved_camera
from denoise_helpers import synthetic_aovs
from refit_helpers import moved_faces, strip_scene
from facemotion_helpers import first_face, translated

pytestmark = pytest.mark.gpu

AOV_IN = ("albedo", "normal", "depth", "hits", "primId", "matId")
OPTION = "temporal_face_motion"


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
    gpu_ctx.set_option(OPTION, 0)
    gpu_ctx.set_option("leaf_size", 4); gpu_ctx.set_option("node_format", 0); gpu_ctx.set_partition(0, 1)
    gpu_ctx.aov_bind(None); gpu_ctx.accum_bind(None); gpu_ctx.denoise_bind(None)


def _frame(ctx, seeds):
    ctx.accum_clear(); ctx.render(seeds)
    ctx.aov_clear(); ctx.render_aovs(seeds)
    return ctx.accum_read(), ctx.aov_read(), ctx.aov_samples()


def _check(ctx, sim, accum, aovs, s, n_acc, cam, centres, faces, ff, what, **kw):
    """One denoise_temporal call against one call of the mirror (a TemporalSim, its option on or off)."""
    got = ctx.denoise_temporal(n_acc, **kw)
    want = sim.run(accum, aovs, n_acc, s, cam, centres, face_pos=faces, first_face=ff, **kw)
    _assert_bits(got, want["out"], (what, "out"))
    r = ctx.temporal_read()
    _assert_bits(r["motion"], want["motion"], (what, "motion"))
    _assert_bits(r["history"], want["history"], (what, "history"))
    _assert_info(ctx.temporal_info(), want["info"], what)
    assert ctx.temporal_face_info() == want["face_info"], (what, ctx.temporal_face_info(), want["face_info"])
    return want


def _torch_rows(rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows, np.float32)).to("cuda:0")


def _add_spheres(ctx, centres, radius=0.06):
    """Spheres beside the loaded mesh (material 0), then the rebuild: ids are spheres, quads, triangles."""
    n = len(centres)
    sph = (K.SphereParams * n)()
    for i, c in enumerate(centres):
        sph[i] = K.SphereParams(radius, K.Float3(*[float(x) for x in c]), K.Float3(0.0, 0.0, 0.0))
    mats = np.zeros(n, np.int32)
    ctx._chk(K.device_lib().moptix_add_spheres(ctx._h, sph, mats.ctypes.data_as(C.POINTER(C.c_int32)), n))
    ctx.build_accel("Trbvh")
    return sph


# (name, node format, how the faces move, through torch tensors, camera and spheres move too)
SEQUENCES = [("rigid", 64, "rigid", False, False), ("deform_numpy", 64, "deform", False, False), ("deform_torch", 128, "deform", True, False),
             ("deform_camera_spheres", 64, "deform", False, True), ("rigid_camera_spheres_128", 128, "rigid", True, True)]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name,fmt,how,device,moving", SEQUENCES, ids=[s[0] for s in SEQUENCES])
def test_gpu_face_motion_is_the_cpu_mirrors_bits_on_coffee(ctx, name, fmt, how, device, moving):
    w, h = 64, 36
    hs = M.HostScene("file:coffee", w, h)
    ctx.set_option("node_format", fmt)
    ctx.set_option(OPTION, 1)
    ctx.load(hs)
    base = hs.face_arrays()[0].copy()
    n_sph = 0
    centres0 = np.float32([[-0.25, 0.3, -0.1], [0.3, 0.25, -0.2]])
    sph = None
    if moving:
        sph = _add_spheres(ctx, centres0)
        n_sph = len(centres0)
    ff = n_sph + int(hs.sizes.nQuads)
    sim = TemporalSim(option=1)
    sim.faces_changed()
    first, count = 20000, 60000
    moved_px = 0
    for k in range(4):
        # frame 2 repeats frame 1's faces without an update: the face pass does not run
        j = k if k < 2 else k - 1
        if how == "rigid":
            faces, lo, rows = translated(base, np.float32([0.012, 0.004, -0.006]) * np.float32(j)), 0, None
            rows = faces
        else:
            faces, rows = moved_faces(hs, 0.004 * j, first, count)
            lo = first
        if k != 2:
            ctx.update_faces(lo, _torch_rows(rows) if device else rows)
            ctx.refit_accel()
            sim.faces_changed()
        centres = None
        p = hs.params
        if moving:
            p = moved_camera(hs.params, (0.01 * k, -0.006 * k, 0.004 * k))
            ctx.set_params(p)
            centres = (centres0 + np.float32([0.01, 0.005, 0.0]) * np.float32(k)).astype(np.float32)
            for i in range(n_sph):
                sph[i].center = K.Float3(*[float(x) for x in centres[i]])
            ctx.update_spheres(0, sph, n_sph)
        accum, aovs, s = _frame(ctx, M.launch_seeds(2, 5, 50 * k))
        want = _check(ctx, sim, accum, aovs, s, 2, cam_of(p), centres, faces, ff, (name, k))
        fi = want["face_info"]
        if k == 0:
            assert fi == dict(tracked_faces=0, moved_faces=0, moved_pixels=0)
        elif k == 2:
            assert fi == dict(tracked_faces=len(base), moved_faces=0, moved_pixels=0)
        else:
            assert fi["tracked_faces"] == len(base) and 0 < fi["moved_faces"] <= (len(base) if how == "rigid" else count)
        moved_px += fi["moved_pixels"]
        if k > 0:
            assert want["info"]["history_pixels"] > 0
    assert moved_px > 0
    ctx.set_params(hs.params)


def _bind_synthetic(ctx, scene, h, w, n_samples=3):
    """The AOV and accumulation buffers bound to torch tensors that the test fills (as tests/test_gpu_temporal.py): the ids then name
    whatever faces the test wants."""
    import torch
    dev = torch.device("cuda", 0)
    prm = K.Params.from_buffer_copy(scene.params)
    prm.width, prm.height = w, h
    ctx.load(scene)
    ctx.set_params(prm)
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
    return fill, n_samples, prm


def _synthetic_sequence(ctx, n_faces, h, w, frames=3, refit=False):
    """A strip of n_faces triangles whose faces all move differently each frame; every geometry pixel names one of them (and a few a
    quad, and a few an id past the last face)."""
    scene = strip_scene(n_faces)
    ctx.set_option(OPTION, 1)
    fill, s, prm = _bind_synthetic(ctx, scene, h, w)
    base = scene.face_arrays()[0].copy()
    ff = first_face(scene)
    sim = TemporalSim(option=1)
    sim.faces_changed()
    rng = np.random.RandomState(n_faces * 31 + h * 7 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    moved = 0
    for k in range(frames):
        accum, aovs, _ = synthetic_aovs(h, w, seed=h * 131 + w, background=0.2, n_samples=s)
        accum = (accum * (0.7 + 0.6 * rng.rand(h, w, 1))).astype(np.float32)
        geo = aovs["hits"][..., 0] > 0
        ids = ff + (yy * w + xx) % (n_faces + 2) - 1           # ff - 1 (a quad), the faces, ff + n_faces (past the last face)
        aovs["primId"] = np.where(geo, ids, -1).astype(np.int32)
        aovs["matId"] = np.where(geo, 0, -1).astype(np.int32)
        fill(accum, aovs)
        faces = (base + np.float32(0.004 * k) * rng.rand(*base.shape)).astype(np.float32)
        if n_faces > 2:
            faces[1] = base[1]                                  # one face never moves
        ctx.update_faces(0, faces if k % 2 else _torch_rows(faces))
        if refit:
            ctx.refit_accel()
        sim.faces_changed()
        want = _check(ctx, sim, accum, aovs, s, 2.0, cam_of(prm), None, faces, ff, (n_faces, h, w, k), iterations=1)
        if k > 0:
            assert want["face_info"]["tracked_faces"] == n_faces
            assert want["face_info"]["moved_faces"] == n_faces - (1 if n_faces > 2 else 0)
            moved += want["face_info"]["moved_pixels"]
    return moved


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n_faces", [1, 63, 64, 65, 257])
def test_face_counts_at_the_wave_and_workgroup_tails(ctx, n_faces):
    assert _synthetic_sequence(ctx, n_faces, 36, 64) > 0


@pytest.mark.timeout(300)
@pytest.mark.parametrize("h,w", [(1, 1), (1, 8)])
def test_tiny_frames(ctx, h, w):
    _synthetic_sequence(ctx, 7, h, w, refit=True)


def _moving_coffee(ctx, option, frames=3):
    """coffee with some rows deforming every frame, the option as given; yields (k, accum, aovs, s, faces)."""
    hs = M.HostScene("file:coffee", 64, 36)
    ctx.set_option(OPTION, option)
    ctx.load(hs)
    for k in range(frames):
        faces, rows = moved_faces(hs, 0.004 * k, 20000, 60000)
        ctx.update_faces(20000, rows)
        ctx.refit_accel()
        accum, aovs, s = _frame(ctx, M.launch_seeds(2, 5, 50 * k))
        yield hs, k, accum, aovs, s, faces


@pytest.mark.timeout(300)
def test_option_off_with_moved_faces_is_todays_behaviour(ctx):
    sim = TemporalSim()
    for hs, k, accum, aovs, s, faces in _moving_coffee(ctx, 0):
        _check(ctx, sim, accum, aovs, s, 2, cam_of(hs.params), None, faces, first_face(hs), ("off", k))
        assert ctx.temporal_face_info()["tracked_faces"] == 0


@pytest.mark.timeout(300)
def test_static_frames_after_motion_cost_nothing_and_apply_no_displacement(ctx):
    sim = TemporalSim(option=1)
    for hs, k, accum, aovs, s, faces in _moving_coffee(ctx, 1):
        sim.faces_changed()
        want = _check(ctx, sim, accum, aovs, s, 2, cam_of(hs.params), None, faces, first_face(hs), ("moving", k))
    assert want["face_info"]["moved_faces"] > 0 and want["face_info"]["moved_pixels"] > 0
    for k in range(2):                                      # no update in between: the face pass does not run
        accum, aovs, s = _frame(ctx, M.launch_seeds(2, 5, 500 + 50 * k))
        want = _check(ctx, sim, accum, aovs, s, 2, cam_of(hs.params), None, faces, first_face(hs), ("static", k))
        assert want["face_info"] == dict(tracked_faces=len(faces), moved_faces=0, moved_pixels=0)
        assert (want["motion"] == 0).all()


@pytest.mark.timeout(300)
def test_face_motion_changes_nothing_else(ctx):
    hs = M.HostScene("file:coffee", 160, 90)
    seeds, more = M.launch_seeds(4), M.launch_seeds(2, 0, 4)
    rays = np.float32([[0.0, 0.18, 0.52, 0.0, 0.0, -1.0, 0.0, 1e30]])
    ctx.set_option("kernel_variant", 4)
    ctx.set_option(OPTION, 1)
    try:
        frames = {}
        for with_denoise in (False, True):
            ctx.load(hs)
            faces, rows = moved_faces(hs, 0.004, 20000, 60000)
            ctx.update_faces(20000, rows); ctx.refit_accel()
            ctx.query_rays(rays)                             # the query area exists
            ctx.accum_clear()
            ctx.kernel_time(reset=True)
            ctx.render(seeds)
            ctx.aov_clear()
            ctx.render_aovs(seeds)
            if with_denoise:
                def state():
                    return (ctx.accum_read(), ctx.aov_read(), ctx.aov_samples(), ctx.kernel_time(), ctx.reduce_time(), ctx.get_option("node_format_used"),
                            ctx.debug_buffer_addresses(), ctx.refit_info(), [a.tobytes() for a in ctx.debug_read_accel()])
                before = state()
                assert np.isfinite(ctx.denoise_temporal(4)).all()
                faces2, rows2 = moved_faces(hs, 0.008, 20000, 60000)
                ctx.update_faces(20000, rows2)               # moved, not refitted: the denoiser reads the faces, not the tree
                assert np.isfinite(ctx.denoise_temporal(4)).all()
                assert ctx.temporal_face_info()["moved_faces"] > 0
                ctx.update_faces(20000, rows)                # back, so that the tree fits again
                ctx.refit_accel()
                after = state()
                _assert_bits(after[0], before[0], "accum")
                for n in AOV_IN:
                    assert np.array_equal(_bits(after[1][n]), _bits(before[1][n])), n
                assert after[2:7] == before[2:7]
                assert {k: v for k, v in after[7].items() if k != "refitMs"} == {k: v for k, v in before[7].items() if k != "refitMs"}
                assert after[8] == before[8]
            ctx.render(more)
            frames[with_denoise] = (ctx.accum_read(), ctx.kernel_time()[1], ctx.get_option("node_format_used"))
        _assert_bits(frames[True][0], frames[False][0], "beauty after the temporal denoiser with face motion")
        assert frames[True][1:] == frames[False][1:]
    finally:
        ctx.set_option("kernel_variant", -1)


@pytest.mark.timeout(300)
def test_state_and_argument_errors(ctx):
    c = M.Context(0)                                        # a context of its own: nothing has been called on it
    try:
        assert c.temporal_face_info() == dict(tracked_faces=0, moved_faces=0, moved_pixels=0)
        assert K.device_lib().moptix_temporal_face_info(c._h, None) == K.ERR_INVALID
        for bad in (-1, 2, 64):
            with pytest.raises(M.MoptixError) as e:
                c.set_option(OPTION, bad)
            assert e.value.code == K.ERR_INVALID, bad
        assert c.get_option(OPTION) == 0
        c.set_option(OPTION, 1)
        assert c.get_option(OPTION) == 1
        hs = M.HostScene("file:coffee", 61, 37)
        c.load(hs)
        with pytest.raises(M.MoptixError) as e:
            c.denoise_temporal(1)
        assert e.value.code == K.ERR_STATE                  # no AOV samples
        assert c.temporal_face_info() == dict(tracked_faces=0, moved_faces=0, moved_pixels=0)
        _frame(c, M.launch_seeds(2))
        c.denoise_temporal(2); c.denoise_temporal(2)
        assert c.temporal_face_info() == dict(tracked_faces=len(hs.face_arrays()[0]), moved_faces=0, moved_pixels=0)
        c.set_option(OPTION, 0); c.set_option(OPTION, 1)    # drops the snapshot, not the history
        c.denoise_temporal(2)
        assert c.temporal_face_info()["tracked_faces"] == 0 and c.temporal_info()["frames"] == 3
        c.temporal_reset()
        c.denoise_temporal(2)
        assert c.temporal_face_info()["tracked_faces"] == 0 and c.temporal_info()["frames"] == 1
    finally:
        c.close()
