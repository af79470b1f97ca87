"""Per-face motion in the temporal stage (include/moptix.h, step 2 of "denoiser: temporal accumulation", option "temporal_face_motion")
without a GPU: the CPU mirror of the whole call (tests/hostsim/temporalsim.cpp with its option on, the kernels' own per-face and per-pixel code from pt_temporal.h)
against the mirror of the call without the option (the same mirror with the option off), against the camera path that the temporal tests already cover,
on a mesh of small triangles that moves fast, and on the edge cases of the snapshot's life.  Measured values: profiles/r14_face_motion.txt."""
import ctypes as C

import numpy as np
import pytest

from common import M, K, MovedScene, hostsim_render, rmse
from aov_helpers import aovsim_render
from temporal_helpers import TemporalSim, cam_of, cam_params, centres_of, copy_spheres, moved_camera, sphere_array
from facemotion_helpers import first_face, grid_mesh_scene, translated

F = np.float64


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    for n in ("out", "motion", "history", "pre"):
        assert np.array_equal(_bits(got[n]), _bits(want[n])), (what, n)
    assert got["info"] == want["info"], (what, got["info"], want["info"])


def _render(scene, seeds):
    accum, _ = hostsim_render(scene, seeds)
    return accum, aovsim_render(scene, seeds)


# ---------------------------------------------------------------------------------------------
# off or unmoved: TemporalSim's bits
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_sequence():
    """Four frames of random_spheres under updateVideo's steps (moving camera, moving spheres): (accum, aovs, camera, centres)."""
    w, h = 64, 36
    hs = M.HostScene("random_spheres", w, h, iarg=60)
    sph, n = sphere_array(hs)
    angle = C.c_float(0.0)
    frames = []
    for k in range(4):
        K.host_lib().mohost_animate_spheres(sph, n, 0.002, C.byref(angle))
        p = K.Params.from_buffer_copy(hs.params)
        K.host_lib().mohost_video_camera(angle.value, w / h, C.byref(p.cam))
        frame = copy_spheres(sph, n)
        scene = MovedScene(hs, spheres=frame, params=p)
        seeds = M.launch_seeds(2, 0, 100 * k)
        accum, aovs = _render(scene, seeds)
        frames.append((accum, aovs, cam_of(p), centres_of(frame, n)))
    return frames, n


@pytest.mark.parametrize("mode", ["on_unmoved", "off_moving"])
def test_without_a_moved_face_the_mirror_gives_temporalsims_bits(sphere_sequence, mode):
    """Moving camera, moving spheres.  on_unmoved: the option on, the faces never change (flagged as changed before every call, so the
    face pass runs and finds nine zeros per face).  off_moving: the option off while the faces move every frame."""
    frames, n = sphere_sequence
    rng = np.random.RandomState(3)
    faces = rng.rand(40, 9).astype(np.float32)
    # every pixel of some frames points at a face: ids past the spheres are faces 0 .. 39
    sim, ref = TemporalSim(option=1 if mode == "on_unmoved" else 0), TemporalSim()
    for k, (accum, aovs, cam, centres) in enumerate(frames):
        a = dict(aovs)
        a["primId"] = np.where(aovs["primId"] >= 0, aovs["primId"] + (n if k % 2 else 0), -1).astype(np.int32)
        if mode == "off_moving":
            faces = (faces + np.float32(0.01)).astype(np.float32)
        sim.faces_changed()
        got = sim.run(accum, a, 2, aovs["samples"], cam, centres, face_pos=faces, first_face=n)
        want = ref.run(accum, a, 2, aovs["samples"], cam, centres)
        _same(got, want, (mode, k))
        assert got["face_info"] == dict(tracked_faces=40 if mode == "on_unmoved" and k > 0 else 0, moved_faces=0, moved_pixels=0)
    assert want["info"]["history_pixels"] > 0


# ---------------------------------------------------------------------------------------------
# a rigid translation of the mesh equals the opposite translation of the previous camera
# ---------------------------------------------------------------------------------------------
# Measured with this test, and copied by hand here and into profiles/r14_face_motion.txt from what
#   python -m pytest tests/test_facemotion_cpu.py -s -k "rigid or tracked or quality or affine"
# prints (the lines "rigid ...", "tracking: ...", "quality ...", "affine ..."): the worst difference of a motion-vector component between run A (mesh moves)
# and run B (previous camera moves) over the pixels compared, in pixels, and the difference of the history counts over those pixels.
# The bounds are 4x the measured values: the two runs round (P - T) - o against P - (o + T), and frame 0's geometry is the mesh at
# base - T seen from o in A, the mesh at base seen from o + T in B.
MV_MEASURED = 1.14e-5
MV_BOUND = 4 * MV_MEASURED
# history: the triangle pixels that found history, A's count against B's.  They differ at the mesh's silhouette, where frame 0 is not the
# same picture in the two runs: in A the quads behind the mesh stay where they are, in B they move with it.
HISTORY_MARGIN_MEASURED = 13         # pixels, of 929 / 942 (grid, T with a z component); 6 of 1749 / 1743 on coffee
HISTORY_MARGIN = 4 * HISTORY_MARGIN_MEASURED

RIGID_CASES = [("coffee", (0.02, 0.0, 0.0)), ("coffee", (-0.01, 0.015, 0.02)), ("grid", (0.03, 0.01, 0.0)), ("grid", (0.0, -0.02, -0.05))]


def _rigid_scene(kind):
    if kind == "coffee":
        hs = M.HostScene("file:coffee", 64, 36)
        return hs, hs.face_arrays()[0].copy()
    sc = grid_mesh_scene(12, 6, -0.45, 0.45, 0.02, 0.42, -0.3)
    return sc, sc.face_arrays()[0].copy()


@pytest.mark.parametrize("kind,T", RIGID_CASES)
def test_rigid_translation_of_the_mesh_equals_a_translation_of_the_previous_camera(kind, T):
    assert MV_BOUND < 1.0 / 16
    hs, base = _rigid_scene(kind)
    T = np.float32(T)
    ff = first_face(hs)
    seeds0, seeds1 = M.launch_seeds(2, 0, 0), M.launch_seeds(2, 0, 100)
    before = translated(base, -T)
    # run A: the mesh at base - T, then at base; the camera stays
    sim_a = TemporalSim(option=1)
    s0 = MovedScene(hs, before, new_faces=(kind == "grid"))
    acc, aov = _render(s0, seeds0)
    sim_a.run(acc, aov, 2, aov["samples"], cam_of(hs.params), face_pos=before, first_face=ff)
    s1 = MovedScene(hs, base, new_faces=(kind == "grid"))
    acc1, aov1 = _render(s1, seeds1)
    sim_a.faces_changed()
    a = sim_a.run(acc1, aov1, 2, aov1["samples"], cam_of(hs.params), face_pos=base, first_face=ff)
    # run B: the mesh at base in both frames; the previous camera is translated by +T
    sim_b = TemporalSim()
    pb = moved_camera(hs.params, T)
    sb = MovedScene(hs, base, new_faces=(kind == "grid"), params=pb)
    accb, aovb = _render(sb, seeds0)
    sim_b.run(accb, aovb, 2, aovb["samples"], cam_of(pb))
    b = sim_b.run(acc1, aov1, 2, aov1["samples"], cam_of(hs.params))
    tri = aov1["primId"][..., 0] >= ff
    assert a["face_info"]["moved_faces"] == len(base) and a["face_info"]["moved_pixels"] == int((tri & (aov1["hits"][..., 0] > 0)).sum())
    both = tri & (a["history"] > 1) & (b["history"] > 1)
    assert both.sum() > 0.5 * tri.sum() > 0
    worst = float(np.abs(a["motion"].astype(F) - b["motion"].astype(F))[both].max())
    ha, hb = int((tri & (a["history"] > 1)).sum()), int((tri & (b["history"] > 1)).sum())
    print("rigid %s T=%s: %d triangle pixels, %d with history in both; worst |mv_A - mv_B| = %.3g px; mean |mv_B| = %.3g px; history A %d, B %d"
          % (kind, T.tolist(), int(tri.sum()), int(both.sum()), worst, float(np.abs(b["motion"][both]).mean()), ha, hb))
    assert float(np.abs(b["motion"][both]).max()) > 0.25            # the camera path really moved these pixels
    assert worst <= MV_BOUND
    assert abs(ha - hb) <= HISTORY_MARGIN


# ---------------------------------------------------------------------------------------------
# tracking: small triangles that move by more than their own size
# ---------------------------------------------------------------------------------------------
# measured with this test: the share of history pixels whose motion vector leads to their own primId in the previous frame
TRACK_MEASURED = dict(on=0.579, off=0.000)      # of 1607 / 1597 history pixels
TRACK_MARGIN = 0.5 * (TRACK_MEASURED["on"] - TRACK_MEASURED["off"])


def _tracking_run(option):
    sc = grid_mesh_scene(16, 8, -0.45, 0.45, 0.02, 0.42, -0.3)       # quads ~3 pixels wide at 64x36
    base = sc.face_arrays()[0].copy()
    ff = first_face(sc)
    step = np.float32([1.5 * 0.9 / 16, 0.0, 0.0])                     # one and a half quads per frame
    sim = TemporalSim(option=option)
    prev_ids, own, n = None, 0, 0
    for k in range(3):
        fp = translated(base, step * np.float32(k))
        scene = MovedScene(sc, fp, new_faces=True)
        acc, aov = _render(scene, M.launch_seeds(2, 0, 100 * k))
        sim.faces_changed()
        got = sim.run(acc, aov, 2, aov["samples"], cam_of(sc.params), face_pos=fp, first_face=ff)
        ids = aov["primId"][..., 0]
        if prev_ids is not None:
            h, w = ids.shape
            yy, xx = np.mgrid[0:h, 0:w]
            has = (got["history"] > 1) & (ids >= ff)
            qx = np.rint(xx - got["motion"][..., 0]).astype(int); qy = np.rint(yy - got["motion"][..., 1]).astype(int)
            ok = has & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            own += int((prev_ids[qy[ok], qx[ok]] == ids[ok]).sum()); n += int(has.sum())
        prev_ids = ids
    return own / max(n, 1), n


def test_small_fast_triangles_are_tracked_with_the_option_and_not_without():
    on, n_on = _tracking_run(1)
    off, n_off = _tracking_run(0)
    print("tracking: own primId at the reprojected pixel: option on %.3f of %d history pixels, off %.3f of %d" % (on, n_on, off, n_off))
    assert n_on > 200 and n_off > 200
    assert on - off >= TRACK_MARGIN


# ---------------------------------------------------------------------------------------------
# edge cases, on a synthetic plane: every pixel sees depth-4 geometry with the ids the test gives it
# ---------------------------------------------------------------------------------------------
def _camera(w, h, origin=(0.0, 0.0, 0.0)):
    o = np.array(origin, F)
    return cam_params(o, (2.0, 0.0, 0.0), (0.0, 2.0 * h / w, 0.0), o + np.array([-1.0, -float(h) / w, -1.0]))


def _plane(h, w, prim, depth=4.0, seed=0):
    yy, xx = np.mgrid[0:h, 0:w]
    dx = -1 + 2 * (xx + 0.5) / w
    dy = (-1 + 2 * (yy + 0.5) / h) * h / w
    z = depth * np.sqrt(dx * dx + dy * dy + 1)
    s = 2
    rng = np.random.RandomState(seed)
    accum = (1.0 + rng.rand(h, w, 3)).astype(np.float32)
    aovs = dict(albedo=np.full((h, w, 3), 0.5 * s, np.float32), normal=np.tile(np.float32([0, 0, s]), (h, w, 1)),
                depth=(z * s)[..., None].astype(np.float32), hits=np.full((h, w, 1), s, np.float32),
                primId=np.broadcast_to(np.asarray(prim, np.int32), (h, w)).copy(), matId=np.zeros((h, w), np.int32))
    return accum, aovs, s


H, W = 20, 32
BIG = np.float32([[-8, -8, -4, 8, -8, -4, 0, 8, -4]])          # one triangle that covers the whole view of the plane z = -4
PIXEL = 2.0 * 4.0 / W                                          # world width of a pixel on that plane


def _two_calls(sim, faces0, faces1, prim, **kw):
    a0, v0, s = _plane(H, W, prim, seed=1)
    sim.run(a0, v0, 1.0, s, _camera(W, H), face_pos=faces0, iterations=0, **kw)
    a1, v1, s = _plane(H, W, prim, seed=2)
    sim.faces_changed()
    return sim.run(a1, v1, 1.0, s, _camera(W, H), face_pos=faces1, iterations=0, **kw)


def test_a_moved_face_shifts_its_pixels_by_its_own_motion():
    """The big triangle moves 3 pixels to the right: every pixel finds its history 3 pixels to the left, as under a camera that moved
    3 pixels to the left."""
    got = _two_calls(TemporalSim(option=1), BIG, translated(BIG, (3 * PIXEL, 0, 0)), 0)
    has = got["history"] == 2
    assert has[:, 3:].all() and not has[:, :3].any()
    assert np.abs(got["motion"][..., 0][has] - 3).max() <= 1e-4 and np.abs(got["motion"][..., 1][has]).max() <= 1e-4
    assert got["face_info"] == dict(tracked_faces=1, moved_faces=1, moved_pixels=H * W)


def _expected_motion(now, prev, clamp=True):
    """Step 2's triangle case and step 3 for the camera of _camera(W, H) at the origin, in float64 from the header's text: per pixel the
    barycentrics (bu, bv) of the pixel's world point on the plane z = -4 with respect to the face's positions now, the affine motion, and
    the motion vector of the projection of P - mo.  Returns (mv [H, W, 2], bu, bv unclamped)."""
    now, prev = np.asarray(now, F).reshape(3, 3), np.asarray(prev, F).reshape(3, 3)
    d = now - prev                                          # exact: the float32 subtraction of the record is exact for these values
    assert np.array_equal((now.astype(np.float32) - prev.astype(np.float32)).astype(F), d)
    yy, xx = np.mgrid[0:H, 0:W]
    P = np.stack([4 * (-1 + 2 * (xx + 0.5) / W), 4 * (-1 + 2 * (yy + 0.5) / H) * H / W, np.full((H, W), -4.0)], -1)
    e1, e2 = now[1] - now[0], now[2] - now[0]
    # w = bu e1 + bv e2 in the triangle's plane: least squares on the 3x2 system (the projection of P onto the plane)
    sol = np.linalg.lstsq(np.stack([e1, e2], 1), (P - now[0]).reshape(-1, 3).T, rcond=None)[0]
    bu, bv = sol[0].reshape(H, W), sol[1].reshape(H, W)
    cu, cv = (np.clip(bu, -1, 2), np.clip(bv, -1, 2)) if clamp else (bu, bv)
    mo = d[0] + cu[..., None] * (d[1] - d[0]) + cv[..., None] * (d[2] - d[0])
    r = P - mo
    s = -r[..., 2]
    fx = (r[..., 0] / s + 1) / 2 * W - 0.5
    fy = (r[..., 1] / s + H / W) / (2 * H / W) * H - 0.5
    return np.stack([xx - fx, yy - fy], -1), bu, bv


# |mv - expected|: fx comes from ~25 rounded binary32 operations on magnitudes up to W * 1.5 = 48, 7e-5 pixel (the analysis of
# tests/test_temporal_cpu.py for this camera and plane); the triangle case adds bu, bv -- ~15 rounded operations each on values up to 2,
# 2e-6 -- times |d_i - d0| <= 1.5 world units = 6 pixels: 1.2e-5 pixel.  Together below 1e-4 pixel.  Measured (pytest -s prints it): 1.9e-6.
AFFINE_BOUND = 1e-4
# per-vertex displacements, all different: a shear plus a stretch, one vertex also in depth; multiples of 2^-6 so that now - prev is exact
AFFINE_D = np.float32([[0.25, 0.0, 0.0], [-0.5, 0.25, 0.0], [0.75, -0.5, 0.125]])


@pytest.mark.parametrize("case", ["inside", "clamped"])
def test_a_deformed_face_moves_each_pixel_by_the_affine_motion_at_its_world_point(case):
    """The three vertices move differently, so bu and bv decide the result.  inside: the big triangle, which covers the view but for its upper corners.
    clamped: a small triangle in the middle of the view named by every pixel, so most points lie far outside it and bu, bv are
    clamped to [-1, 2]."""
    now = BIG if case == "inside" else np.float32([[-0.5, -0.5, -4, 0.5, -0.5, -4, -0.5, 0.5, -4]])
    prev = (now.reshape(3, 3) - AFFINE_D).astype(np.float32).reshape(1, 9)
    got = _two_calls(TemporalSim(option=1), prev, now, 0)
    want, bu, bv = _expected_motion(now, prev)
    has = got["history"] == 2
    assert got["face_info"] == dict(tracked_faces=1, moved_faces=1, moved_pixels=H * W) and has.sum() > 0.5 * H * W
    err = float(np.abs(got["motion"].astype(F) - want)[has].max())
    free, _, _ = _expected_motion(now, prev, clamp=False)
    outside = (bu < -1) | (bu > 2) | (bv < -1) | (bv > 2)
    print("affine %s: %d pixels with history, worst |mv - float64| = %.3g px, |mv| up to %.3g px, bu in [%.2f, %.2f], bv in [%.2f, %.2f], %d outside the clamp"
          % (case, int(has.sum()), err, float(np.abs(want[has]).max()), bu.min(), bu.max(), bv.min(), bv.max(), int(outside.sum())))
    assert err <= AFFINE_BOUND
    # the case is what it says: the motion varies over the face, in both barycentric directions
    assert np.ptp(want[has][:, 0]) > 1 and np.ptp(want[has][:, 1]) > 0.5
    if case == "inside":
        assert not outside.any()                            # (the view's upper corners lie just outside the triangle, inside the clamp)
    else:
        assert (outside & has).sum() > 0.3 * H * W
        assert float(np.abs(free - want)[outside & has].max()) > 1.0      # without the clamp these pixels would land elsewhere
        for lo, hi, b in ((-1, 2, bu), (-1, 2, bv)):                        # both ends of both clamps are reached
            assert (b[has] < lo).any() and (b[has] > hi).any()


def test_a_zero_area_face_that_moves_takes_its_first_vertex_displacement():
    """nn = 0: bu = bv = 0, mo = d0.  The mirror's result: the bits of a proper triangle whose three vertices all move by d0."""
    d = np.float32([[2 * PIXEL, PIXEL, 0], [-1, 0, 0], [0, 5, 0]])
    for degenerate in (np.float32([[1, 1, -4] * 3]), np.float32([[0, 0, -4, 1, 0, -4, 2, 0, -4]])):      # now a point; now a segment
        before = (degenerate.reshape(3, 3) - d).astype(np.float32).reshape(1, 9)                          # a proper triangle before the move
        d0 = degenerate[0, :3] - before[0, :3]
        got = _two_calls(TemporalSim(option=1), before, degenerate, 0)
        # the reference run: BIG's vertices are small integers, so that adding d0 and subtracting again gives d0 exactly
        ref_before = (BIG.reshape(3, 3) - d0).astype(np.float32)
        assert np.array_equal(BIG.reshape(3, 3) - ref_before, np.tile(d0, (3, 1)))
        want = _two_calls(TemporalSim(option=1), ref_before.reshape(1, 9), BIG, 0)
        assert np.array_equal(_bits(got["motion"]), _bits(want["motion"])) and np.array_equal(_bits(got["out"]), _bits(want["out"]))
        assert got["face_info"] == dict(tracked_faces=1, moved_faces=1, moved_pixels=H * W)
        assert (got["history"] == 2).any() and np.abs(got["motion"][..., 0][got["history"] == 2] - 2).max() <= 1e-4


def test_a_face_moved_and_moved_back_has_no_displacement():
    """Call 2 sees the move; before call 3 the face moves away and back: the face pass runs, finds nine zeros, and the call gives
    TemporalSim's bits (the static shortcut)."""
    sim, idle = TemporalSim(option=1), TemporalSim(option=1)          # `idle` gets no update before its third call: its face pass does not run
    there = translated(BIG, (2 * PIXEL, 0, 0))
    for k, faces in enumerate((BIG, there)):
        a, v, s = _plane(H, W, 0, seed=1 + k)
        for m in (sim, idle):
            m.faces_changed()
            second = m.run(a, v, 1.0, s, _camera(W, H), face_pos=faces, iterations=0)
    assert second["face_info"]["moved_faces"] == 1 and (second["motion"][..., 0] != 0).any()
    a, v, s = _plane(H, W, 0, seed=3)
    sim.faces_changed(); sim.faces_changed()                # moptix_update_faces away, and back to `there`
    third = sim.run(a, v, 1.0, s, _camera(W, H), face_pos=there, iterations=0)
    assert third["face_info"] == dict(tracked_faces=1, moved_faces=0, moved_pixels=0)
    assert (third["motion"] == 0).all() and (third["history"] > 1).all()        # the static shortcut: every pixel onto itself
    want = idle.run(a, v, 1.0, s, _camera(W, H), face_pos=there, iterations=0)
    _same(third, want, "moved back")
    assert want["face_info"] == third["face_info"]


def test_a_face_count_change_keeps_the_history_and_tracks_nothing_in_that_call():
    sim = TemporalSim(option=1)
    two = np.concatenate([BIG, translated(BIG, (0, 0, -1))])
    a, v, s = _plane(H, W, 0, seed=1)
    sim.run(a, v, 1.0, s, _camera(W, H), face_pos=BIG, iterations=0)
    a, v, s = _plane(H, W, 0, seed=2)
    sim.faces_changed()                                     # moptix_add_mesh, moptix_build_accel; face 0 moved as well
    got = sim.run(a, v, 1.0, s, _camera(W, H), face_pos=translated(two, (PIXEL, 0, 0)), iterations=0)
    assert got["face_info"] == dict(tracked_faces=0, moved_faces=0, moved_pixels=0)
    assert got["info"]["frames"] == 2 and got["info"]["history_pixels"] == H * W and (got["motion"] == 0).all()
    a, v, s = _plane(H, W, 0, seed=3)
    sim.faces_changed()
    got = sim.run(a, v, 1.0, s, _camera(W, H), face_pos=translated(two, (2 * PIXEL, 0, 0)), iterations=0)
    assert got["face_info"] == dict(tracked_faces=2, moved_faces=2, moved_pixels=H * W)      # the new snapshot serves the next call


def test_turning_the_option_off_drops_the_snapshot():
    sim = TemporalSim(option=1)
    a, v, s = _plane(H, W, 0, seed=1)
    sim.run(a, v, 1.0, s, _camera(W, H), face_pos=BIG, iterations=0)
    sim.set_option(0); sim.set_option(1)
    sim.faces_changed()
    a, v, s = _plane(H, W, 0, seed=2)
    got = sim.run(a, v, 1.0, s, _camera(W, H), face_pos=translated(BIG, (PIXEL, 0, 0)), iterations=0)
    assert got["face_info"] == dict(tracked_faces=0, moved_faces=0, moved_pixels=0) and (got["motion"] == 0).all()
    assert got["info"]["frames"] == 2                       # the history itself stays
    sim.reset()                                             # moptix_temporal_reset drops both
    got = sim.run(a, v, 1.0, s, _camera(W, H), face_pos=BIG, iterations=0)
    assert got["info"]["frames"] == 1 and got["face_info"]["tracked_faces"] == 0


def test_spheres_and_quads_beside_moved_triangles_keep_their_own_rules():
    """Columns 0-9: sphere 0 (its centre moves one pixel up), 10-19: quad (id 1: never moves), 20-31: face 0 (moves 2 pixels right).
    The sphere's and the quad's pixels have TemporalSim's bits; the triangle's pixels move by 2."""
    prim = np.where(np.arange(W) < 10, 0, np.where(np.arange(W) < 20, 1, 2))[None, :]
    sim, ref = TemporalSim(option=1), TemporalSim()
    cen0, cen1 = np.float32([[0, 0, -4]]), np.float32([[0, PIXEL, -4]])
    a, v, s = _plane(H, W, prim, seed=1)
    sim.run(a, v, 1.0, s, _camera(W, H), cen0, face_pos=BIG, first_face=2, iterations=0); ref.run(a, v, 1.0, s, _camera(W, H), cen0, iterations=0)
    a, v, s = _plane(H, W, prim, seed=2)
    sim.faces_changed()
    got = sim.run(a, v, 1.0, s, _camera(W, H), cen1, face_pos=translated(BIG, (2 * PIXEL, 0, 0)), first_face=2, iterations=0)
    want = ref.run(a, v, 1.0, s, _camera(W, H), cen1, iterations=0)
    for n in ("out", "motion", "history"):
        assert np.array_equal(_bits(got[n][:, :20]), _bits(want[n][:, :20])), n
    assert np.abs(got["motion"][1:, :10, 1] - 1).max() <= 1e-4 and (got["motion"][:, 10:20] == 0).all()
    tri = got["motion"][:, 22:, 0]
    assert np.abs(tri - 2).max() <= 1e-4 and (want["motion"][:, 20:] == 0).all()
    assert got["face_info"] == dict(tracked_faces=1, moved_faces=1, moved_pixels=H * 12)


# ---------------------------------------------------------------------------------------------
# frame quality: recorded, not asserted (profiles/r14_face_motion.txt says which way it came out)
# ---------------------------------------------------------------------------------------------
def test_frame_quality_numbers_of_a_translating_coffee_mesh():
    w, h, frames, spp = 192, 108, 6, 4
    hs = M.HostScene("file:coffee", w, h)
    base = hs.face_arrays()[0].copy()
    ff = first_face(hs)
    step = np.float32([0.01, 0.0, 0.0])
    sims = {1: TemporalSim(option=1), 0: TemporalSim(option=0)}
    for k in range(frames):
        fp = translated(base, step * np.float32(k))
        scene = MovedScene(hs, fp)
        seeds = M.launch_seeds(spp, 0, 100 * k)
        acc, aov = _render(scene, seeds)
        got = {}
        for opt, sim in sims.items():
            sim.faces_changed()
            got[opt] = sim.run(acc, aov, spp, aov["samples"], cam_of(hs.params), face_pos=fp, first_face=ff)
    ref, _ = hostsim_render(scene, M.launch_seeds(512, 0, 5000))
    ref = ref / np.float32(512)
    e = {opt: rmse(got[opt]["out"], ref) for opt in got}
    print("quality coffee %dx%d, %d frames at %d spp, mesh +%.3g in x per frame: last-frame RMSE vs 512 spp: option on %.4f, off %.4f, noisy %.4f; "
          "history pixels on %d, off %d; mean h on %.2f, off %.2f"
          % (w, h, frames, spp, float(step[0]), e[1], e[0], rmse(acc / np.float32(spp), ref), got[1]["info"]["history_pixels"],
             got[0]["info"]["history_pixels"], got[1]["info"]["mean_history"], got[0]["info"]["mean_history"]))
    assert got[1]["face_info"]["moved_faces"] == len(base)
    assert np.isfinite(got[1]["out"]).all()


# ---------------------------------------------------------------------------------------------
# host-only entry points
# ---------------------------------------------------------------------------------------------
def test_face_info_and_the_option_without_a_device():
    lib = K.device_lib()
    assert lib.moptix_temporal_face_info(None, C.byref(K.TemporalFaceStats())) == K.ERR_INVALID
    assert "moptix_temporal_face_info" in K.DEVICE_SYMBOLS
    assert [f for f, _ in K.TemporalFaceStats._fields_] == ["trackedFaces", "movedFaces", "movedPixels"]
    assert C.sizeof(K.TemporalFaceStats) == 24
