"""Temporal accumulation (include/moptix.h "denoiser: temporal accumulation") without a GPU: the CPU mirror of the kernels
(tests/hostsim/temporalsim.cpp, the kernels' own per-pixel code from pt_temporal.h) against an independent float64 statement of the contract written
here from the header's text, the anchor to the spatial denoiser, the properties of reprojection, the history's life, the quality
on path-traced sequences and the C ABI's host-only entry points."""
import ctypes as C

import numpy as np
import pytest

from common import M, K, MovedScene, hostsim_render, rmse
from aov_helpers import aovsim_render
from denoise_helpers import denoisesim, synthetic_aovs
from temporal_helpers import (TEMPORAL_DEFAULTS, TemporalSim, cam_params, cam_of, centres_of, copy_spheres, moved_camera,
                              sphere_array)

F = np.float64
LUM = np.array([0.2126, 0.7152, 0.0722], F)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _with_ids(aovs, prim=None, mat=None):
    h, w = aovs["hits"].shape[:2]
    geo = aovs["hits"][..., 0] > 0
    a = dict(aovs)
    a["primId"] = np.where(geo, 0 if prim is None else prim, -1).astype(np.int32)
    a["matId"] = np.where(geo, 0 if mat is None else mat, -1).astype(np.int32)
    return a


# a camera at the origin looking down -z: pixel (x, y) sees direction (-1 + 2 (x + .5) / W, (-1 + 2 (y + .5) / H) * H / W, -1)
def _camera(w, h, origin=(0.0, 0.0, 0.0)):
    o = np.array(origin, F)
    return cam_params(o, (2.0, 0.0, 0.0), (0.0, 2.0 * h / w, 0.0), o + np.array([-1.0, -float(h) / w, -1.0]))


# ---------------------------------------------------------------------------------------------
# the contract's steps 1-6 in float64, pixel by pixel, from the header's text
# ---------------------------------------------------------------------------------------------
def _decode(accum, aovs, n_acc, s, demodulate):
    c = accum.astype(F) / n_acc
    hits = aovs["hits"][..., 0].astype(F)
    geo = hits > 0
    nr = aovs["normal"].astype(F) / s
    ln = np.sqrt((nr * nr).sum(-1, keepdims=True))
    n = np.where(ln > 0, nr / np.where(ln > 0, ln, 1), 0)
    z = np.where(geo, aovs["depth"][..., 0].astype(F) / np.where(geo, hits, 1), 0)
    a = np.maximum(aovs["albedo"].astype(F) / s, 1e-3) if demodulate else np.ones_like(c)
    return np.where(geo[..., None], c / a, c), n, z, geo


def _cam64(cam):
    return [np.array(getattr(cam, k).tolist(), F) for k in ("origin", "horizontal", "vertical", "scrLowerLeftCorner")]


def spec_temporal(frame, prev, t, margin=1e-4):
    """frame: dict(I, N, Z, geo, prim, mat, cam, centres); prev: None or dict(I_acc, h, m1, m2, N, Z, geo, mat, cam, centres).
    Returns the new history dict plus mv, hist (has history) and `unsure`: pixels where a validity decision is within `margin`
    (relative) of its threshold, which binary32 and float64 may take differently."""
    I, N, Z, geo = frame["I"], frame["N"], frame["Z"], frame["geo"]
    h_, w_ = geo.shape
    l = I @ LUM
    out = dict(I_acc=I.copy(), h=np.ones((h_, w_)), m1=l.copy(), m2=l * l, N=N, Z=Z, geo=geo, mat=frame["mat"], cam=frame["cam"],
               centres=frame["centres"], mv=np.zeros((h_, w_, 2)), hist=np.zeros((h_, w_), bool), unsure=np.zeros((h_, w_), bool))
    if prev is not None:
        o, hz, vt, ll = _cam64(frame["cam"])
        po, ph, pv, pll = _cam64(prev["cam"])
        A = np.stack([pll - po, ph, pv], axis=1)
        same_cam = all(np.array_equal(a, b) for a, b in zip((o, hz, vt, ll), (po, ph, pv, pll)))
        for y in range(h_):
            for x in range(w_):
                if not geo[y, x]:
                    continue
                d = ll + (x + 0.5) / w_ * hz + (y + 0.5) / h_ * vt - o
                P = o + Z[y, x] * d / np.linalg.norm(d)
                pid = frame["prim"][y, x]
                mo = frame["centres"][pid] - prev["centres"][pid] if 0 <= pid < len(frame["centres"]) else np.zeros(3)
                if same_cam and not mo.any():
                    fx, fy, zp = float(x), float(y), Z[y, x]
                else:
                    r = P - mo - po
                    if abs(np.linalg.det(A)) == 0:
                        continue
                    s, su, sv = np.linalg.solve(A, r)
                    if not s > 0:
                        continue
                    fx, fy, zp = su / s * w_ - 0.5, sv / s * h_ - 0.5, np.linalg.norm(r)
                if not (-1 < fx < w_ and -1 < fy < h_):
                    continue
                x0, y0 = int(np.floor(fx)), int(np.floor(fy))
                tx, ty = fx - x0, fy - y0
                sw, sI, s1, s2, hmin = 0.0, np.zeros(3), 0.0, 0.0, None
                for j in (0, 1):
                    for i in (0, 1):
                        qx, qy = x0 + i, y0 + j
                        wgt = (tx if i else 1 - tx) * (ty if j else 1 - ty)
                        if not (0 <= qx < w_ and 0 <= qy < h_) or not wgt > 0 or not prev["geo"][qy, qx]:
                            continue
                        if wgt < margin:
                            out["unsure"][y, x] = True
                        nd = float(N[y, x] @ prev["N"][qy, qx])
                        dz = abs(prev["Z"][qy, qx] - zp)
                        if abs(nd - t["normal_threshold"]) < margin or abs(dz - t["depth_tolerance"] * zp) < margin * zp:
                            out["unsure"][y, x] = True
                        if prev["mat"][qy, qx] != frame["mat"][y, x] or nd < t["normal_threshold"] or dz > t["depth_tolerance"] * zp:
                            continue
                        sw += wgt; sI += wgt * prev["I_acc"][qy, qx]; s1 += wgt * prev["m1"][qy, qx]; s2 += wgt * prev["m2"][qy, qx]
                        hmin = prev["h"][qy, qx] if hmin is None else min(hmin, prev["h"][qy, qx])
                if hmin is None or sw < 1e-2:
                    out["unsure"][y, x] |= hmin is not None and abs(sw - 1e-2) < margin
                    continue
                hh = min(hmin + 1, t["max_history"])
                a, am = max(1 / hh, t["alpha"]), max(1 / hh, t["alpha_moments"])
                ip, p1, p2 = sI / sw, s1 / sw, s2 / sw
                out["I_acc"][y, x] = ip + a * (I[y, x] - ip)
                out["m1"][y, x] = p1 + am * (l[y, x] - p1)
                out["m2"][y, x] = p2 + am * (l[y, x] ** 2 - p2)
                out["h"][y, x] = hh
                out["mv"][y, x] = (x - fx, y - fy)
                out["hist"][y, x] = True
    out["var"] = np.where(geo & (out["h"] >= t["variance_frames"]), np.maximum(out["m2"] - out["m1"] ** 2, 0), np.nan)
    return out


def test_mirror_matches_the_float64_contract_on_a_moving_synthetic_sequence():
    """Bound: I_acc is reached from the inputs through ~12 rounded operations for the world point (u, three 2-op components, the
    normalisation's 5, the fma), ~10 for the solve and fx / fy, 4 weights, and per channel 4 products + 4 sums + a division + 3 blend
    operations: ~40 operations of relative error <= 2^-24 each, and the bilinear fetch turns an error of fx (<= ~1e-5 pixel at these
    coordinates) into |dI/dx| * 1e-5.  With neighbouring values differing by O(1) relative that gives 4e-5 per frame; errors of the
    history are carried (damped by 1 - alpha_h) into later frames, so 4 frames stay below 2e-4 of the frame's scale.  The motion
    vector is fx itself: absolute 2e-4 pixel.  History lengths are integers and must agree exactly outside the `unsure` pixels."""
    h, w, s = 24, 36, 4
    sim = TemporalSim()
    t = dict(TEMPORAL_DEFAULTS, variance_frames=2)
    prev = None
    rng = np.random.RandomState(2)
    centres = np.zeros((3, 3), np.float32)
    n_unsure = n_hist = 0
    for k in range(4):
        accum, aovs, _ = synthetic_aovs(h, w, seed=40, background=0.2, n_samples=s)         # the same guide layers every frame
        accum = (accum * (0.7 + 0.6 * rng.rand(h, w, 1))).astype(np.float32)                # new noise
        yy, xx = np.mgrid[0:h, 0:w]
        prim = np.where(xx < w // 3, 1, 7)                                                  # the left third is "sphere 1"
        aovs = _with_ids(aovs, prim=prim, mat=(xx * 3) // w)
        cam = _camera(w, h, origin=(0.013 * k, -0.007 * k, 0.002 * k))
        centres = centres.copy(); centres[1] = np.float32([0.01 * k, 0.004 * k, 0.0])
        got = sim.run(accum, aovs, 2.0, s, cam, centres, temporal=t, iterations=1, demodulate=True)
        I, N, Z, geo = _decode(accum, aovs, 2.0, F(s), True)
        cur = spec_temporal(dict(I=I, N=N, Z=Z, geo=geo, prim=aovs["primId"], mat=aovs["matId"], cam=cam, centres=centres.astype(F)), prev, t)
        ok = ~cur["unsure"]
        if prev is not None:
            ok &= ~prev["tainted"]
        # a pixel whose decision is unsure may differ, and so may everything that later reads it: those are excluded, and must be few
        tainted = ~ok
        if prev is not None:
            tainted = tainted | _dilate(tainted, 3)
        cur["tainted"] = tainted
        ok = ~tainted
        assert np.array_equal(got["history"][ok], cur["h"][ok].astype(np.float32)), k
        scale = np.abs(cur["I_acc"]).mean()
        assert float(np.abs(got["pre"][..., :3].astype(F) - cur["I_acc"])[ok].max()) <= 2e-4 * scale, k
        assert float(np.abs(got["motion"].astype(F) - cur["mv"])[ok].max()) <= 2e-4, k
        tv = ok & ~np.isnan(cur["var"])
        if tv.any():                                        # m2 - m1^2 cancels: the error is relative to m2
            assert float((np.abs(got["pre"][..., 3].astype(F) - cur["var"])[tv] / np.maximum(cur["m2"][tv], 1e-6)).max()) <= 4e-4, k
        assert got["info"]["geometry_pixels"] == int(geo.sum())
        assert got["info"]["history_pixels"] + got["info"]["disoccluded_pixels"] == got["info"]["geometry_pixels"]
        n_unsure += int(tainted[geo].sum()); n_hist += int((cur["hist"] & ok).sum())
        prev = cur
    assert n_hist > 0.5 * 3 * h * w * 0.8 and n_unsure < 0.1 * 4 * h * w, (n_hist, n_unsure)


def _dilate(m, r):
    out = m.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out |= np.roll(np.roll(m, dy, 0), dx, 1)
    return out


# ---------------------------------------------------------------------------------------------
# the anchor: a first frame is the spatial denoiser, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(iterations=1, normal_power=7, demodulate=True), dict(iterations=0), dict(iterations=0, demodulate=True),
                                dict(iterations=8, normal_power=1, sigma_luminance=0.5, sigma_depth=3.0)])
def test_first_call_after_a_reset_is_the_spatial_denoiser_bit_for_bit(kw):
    accum, aovs, s = synthetic_aovs(29, 43, seed=7)
    aovs = _with_ids(aovs)
    sim = TemporalSim()
    want = denoisesim(accum, aovs, 3.0, s, **kw)
    for _ in range(2):
        got = sim.run(accum, aovs, 3.0, s, _camera(43, 29), temporal=dict(variance_frames=2), **kw)
        assert np.array_equal(_bits(got["out"]), _bits(want))
        assert (got["history"] == 1).all() and (got["motion"] == 0).all() and got["info"]["history_pixels"] == 0
        assert got["info"]["frames"] == 1 and got["info"]["disoccluded_pixels"] == got["info"]["geometry_pixels"]
        sim.reset()


# ---------------------------------------------------------------------------------------------
# properties of the accumulation and of the reprojection
# ---------------------------------------------------------------------------------------------
def test_static_frames_accumulate_to_their_mean():
    """alpha = 0: I_acc(n) = I_acc(n-1) + (I_n - I_acc(n-1)) / n, three roundings plus the division's per step on top of the carried
    error: n steps stay within 4 n ulp of the mean (n = 8: 32 ulp = 3.8e-6 relative to the largest frame value of the pixel)."""
    h, w, s, n = 21, 33, 4, 8
    _, aovs, _ = synthetic_aovs(h, w, seed=12, background=0.2, n_samples=s)
    aovs = _with_ids(aovs)
    geo = aovs["hits"][..., 0] > 0
    sim = TemporalSim()
    rng = np.random.RandomState(5)
    frames = []
    for k in range(n):
        accum = (rng.rand(h, w, 3) * 3).astype(np.float32)
        frames.append(accum)
        got = sim.run(accum, aovs, 1.0, s, _camera(w, h), temporal=dict(alpha=0.0, alpha_moments=0.0, max_history=n), iterations=0)
        assert (got["history"][geo] == k + 1).all() and (got["history"][~geo] == 1).all()
        assert (got["motion"] == 0).all()
        assert got["info"]["disoccluded_pixels"] == (int(geo.sum()) if k == 0 else 0)
        assert got["info"]["mean_history"] == k + 1 and got["info"]["frames"] == k + 1
    mean = np.mean(np.asarray(frames, F), axis=0)
    top = np.max(np.asarray(frames, F), axis=0)
    assert float((np.abs(got["out"].astype(F) - mean) / top)[geo].max()) <= 4 * n * 2.0 ** -24
    assert np.array_equal(_bits(got["out"][~geo]), _bits(frames[-1][~geo]))


def _plane_frame(h, w, cam_x, rng, depth=4.0, texture=None):
    """A fronto-parallel plane z = -depth seen by _camera at (cam_x, 0, 0): per-pixel ray length, constant normal; the beauty is a
    world-space texture (a function of the plane point) so that a pixel's history is its own surface point."""
    yy, xx = np.mgrid[0:h, 0:w]
    dx = -1 + 2 * (xx + 0.5) / w
    dy = (-1 + 2 * (yy + 0.5) / h) * h / w
    z = depth * np.sqrt(dx * dx + dy * dy + 1)
    wx, wy = cam_x + depth * dx, depth * dy
    s = 2
    tex = 1.0 + 0.5 * np.sin(3 * wx)[..., None] * np.array([1.0, 0.5, 0.25]) + 0.3 * np.cos(2 * wy)[..., None] if texture is None else texture(wx, wy)
    aovs = dict(albedo=np.full((h, w, 3), 0.5 * s, np.float32), normal=np.tile(np.float32([0, 0, s]), (h, w, 1)),
                depth=(z * s)[..., None].astype(np.float32), hits=np.full((h, w, 1), s, np.float32))
    return tex.astype(np.float32), _with_ids(aovs), s


def test_a_whole_pixel_translation_finds_its_history_at_the_shifted_pixel():
    h, w, shift = 20, 32, 3
    step = 2.0 * 4.0 / w                                   # world width of a pixel on the plane z = -4
    sim = TemporalSim()
    rng = np.random.RandomState(1)
    a0, aovs0, s = _plane_frame(h, w, 0.0, rng)
    sim.run(a0, aovs0, 1.0, s, _camera(w, h), iterations=0)
    a1, aovs1, s = _plane_frame(h, w, shift * step, rng)
    got = sim.run(a1, aovs1, 1.0, s, _camera(w, h, origin=(shift * step, 0, 0)), temporal=dict(alpha=0.0), iterations=0)
    # the camera moved right by 3 pixels' worth: pixel x shows what pixel x + 3 showed.  fx = x + 3 up to rounding, on either side of the
    # integer: the tap at x + 3 carries all the weight but ~1e-5, so a pixel has history iff x + 3 is inside the frame -- at x = w - 3 the
    # only tap inside (weight ~1e-5 when fx rounds below w) is under the 1e-2 minimum weight.  Exactly the columns that left the frame
    # are disoccluded.
    has = got["history"] == 2
    assert has[:, :w - shift].all() and not has[:, w - shift:].any()
    assert (got["history"][:, w - shift:] == 1).all()
    assert got["info"]["disoccluded_pixels"] == h * shift and got["info"]["history_pixels"] == h * (w - shift)
    # fx comes from ~25 rounded binary32 operations on magnitudes up to W * 1.5 = 48 (pixel coordinate times the depth ratios of
    # the solve): 25 * 2^-24 * 48 = 7e-5 pixel
    assert np.abs(got["motion"][..., 0][has] + shift).max() <= 1e-4 and np.abs(got["motion"][..., 1][has]).max() <= 1e-4
    # alpha_h = 1/2: the mean of this frame and of the shifted previous one (the same texture point).  The bilinear fetch turns fx's
    # 7e-5 into 7e-5 * |dI/dx| (<= 0.5 * 3 * step = 0.375 per pixel) = 3e-5, plus a few ulp of values ~2: bound 1e-4
    want = 0.5 * (a1[:, :w - shift].astype(F) + a0[:, shift:].astype(F))
    assert float(np.abs(got["out"][:, :w - shift] - want).max()) <= 1e-4


def test_a_camera_one_ulp_away_takes_the_general_path_and_maps_a_static_pixel_onto_itself():
    """The exact shortcut of step 3 needs the same camera bit for bit.  One ulp off, the projection itself must bring every pixel back
    to its own centre: |motion| within the 7e-5 pixel of the rounding analysis above (plus the ulp's own 1e-7), full history, and
    the blend that of the static case to within the bilinear residue."""
    h, w = 20, 32
    rng = np.random.RandomState(1)
    a0, aovs, s = _plane_frame(h, w, 0.0, rng)
    a1 = (a0 * np.float32(0.5)).astype(np.float32)
    o = np.float32([0.3, 0.2, 0.1])
    static, general = TemporalSim(), TemporalSim()
    static.run(a0, aovs, 1.0, s, _camera(w, h, origin=o), iterations=0)
    general.run(a0, aovs, 1.0, s, _camera(w, h, origin=o), iterations=0)
    o1 = o.copy(); o1[0] = np.nextafter(o[0], np.float32(1))
    ref = static.run(a1, aovs, 1.0, s, _camera(w, h, origin=o), temporal=dict(alpha=0.0), iterations=0)
    got = general.run(a1, aovs, 1.0, s, _camera(w, h, origin=o1), temporal=dict(alpha=0.0), iterations=0)
    assert (ref["motion"] == 0).all() and (ref["history"] == 2).all()
    assert (got["history"] == 2).all() and got["info"]["disoccluded_pixels"] == 0
    assert (got["motion"] != 0).any()                      # the general path really ran
    assert np.abs(got["motion"]).max() <= 1e-4
    assert float(np.abs(got["out"].astype(F) - ref["out"].astype(F)).max()) <= 1e-4


def test_a_moved_sphere_takes_its_history_along_and_uncovers_disocclusions():
    """A 'sphere' (primId 0, material 1, a disc of constant colour at depth 2) in front of a wall (primId 5, material 0, depth 6), camera
    fixed; between the frames the sphere's centre moves right by 4 pixels' worth at its depth."""
    h, w, s, shift = 24, 40, 2, 4
    yy, xx = np.mgrid[0:h, 0:w]
    dx = -1 + 2 * (xx + 0.5) / w
    dy = (-1 + 2 * (yy + 0.5) / h) * h / w
    norm = np.sqrt(dx * dx + dy * dy + 1)
    wall_c, ball_c = np.float32([0.2, 0.3, 0.9]), np.float32([0.9, 0.1, 0.1])

    def frame(cx):
        disc = (xx - cx) ** 2 + (yy - 12) ** 2 <= 36
        z = np.where(disc, 2.0, 6.0) * norm
        accum = np.where(disc[..., None], ball_c, wall_c).astype(np.float32)
        aovs = dict(albedo=np.full((h, w, 3), 0.5 * s, np.float32), normal=np.tile(np.float32([0, 0, s]), (h, w, 1)),
                    depth=(z * s)[..., None].astype(np.float32), hits=np.full((h, w, 1), s, np.float32),
                    primId=np.where(disc, 0, 5).astype(np.int32), matId=np.where(disc, 1, 0).astype(np.int32))
        return accum, aovs, disc
    move = shift * (2.0 * 2.0 / w)                         # 4 pixels at depth 2
    sim = TemporalSim()
    a0, aovs0, disc0 = frame(14)
    sim.run(a0, aovs0, 1.0, s, _camera(w, h), np.float32([[0, 0, -2]]), iterations=0)
    a1, aovs1, disc1 = frame(14 + shift)
    got = sim.run(a1, aovs1, 1.0, s, _camera(w, h), np.float32([[move, 0, -2]]), iterations=0)
    has = got["history"] == 2
    inner = (xx - 14 - shift) ** 2 + (yy - 12) ** 2 <= 16  # well inside the disc: all four taps on last frame's disc
    assert has[inner].all()
    assert np.abs(got["motion"][..., 0][inner] - shift).max() <= 1e-3 and np.abs(got["motion"][..., 1][inner]).max() <= 1e-3
    uncovered = disc0 & ~disc1
    assert uncovered.sum() > 20 and not has[uncovered].any()
    assert np.array_equal(_bits(got["out"][uncovered]), _bits(a1[uncovered]))            # the wall's colour, nothing of the sphere's
    still_wall = ~disc0 & ~disc1
    assert has[still_wall].all() and (got["motion"][still_wall] == 0).all()


# ---------------------------------------------------------------------------------------------
# the history's life
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["reset", "frame_size", "sphere_count", "demodulate", "iterations_zero"])
def test_history_drops(how):
    h, w = 16, 24
    accum, aovs, s = synthetic_aovs(h, w, seed=3, background=0.1)
    aovs = _with_ids(aovs)
    sim = TemporalSim()
    cen = np.zeros((2, 3), np.float32)
    kw = dict(iterations=2, demodulate=True)
    assert sim.run(accum, aovs, 1.0, s, _camera(w, h), cen, **kw)["info"]["history_pixels"] == 0
    second = sim.run(accum, aovs, 1.0, s, _camera(w, h), cen, **kw)
    assert second["info"]["history_pixels"] == second["info"]["geometry_pixels"] > 0 and second["info"]["frames"] == 2
    if how == "reset":
        sim.reset()
    elif how == "frame_size":
        accum, aovs, s = synthetic_aovs(h, w + 1, seed=3, background=0.1)
        aovs = _with_ids(aovs); w += 1
    elif how == "sphere_count":
        cen = np.zeros((3, 3), np.float32)
    elif how == "demodulate":
        kw = dict(iterations=2, demodulate=False)
    else:
        kw = dict(iterations=0, demodulate=True)           # iterations = 0 runs without demodulation
    third = sim.run(accum, aovs, 1.0, s, _camera(w, h), cen, **kw)
    assert third["info"]["history_pixels"] == 0 and third["info"]["frames"] == 1 and (third["history"] == 1).all()
    assert np.array_equal(_bits(third["out"]), _bits(denoisesim(accum, aovs, 1.0, s, **kw)))
    fourth = sim.run(accum, aovs, 1.0, s, _camera(w, h), cen, **kw)
    assert fourth["info"]["history_pixels"] == fourth["info"]["geometry_pixels"]


# ---------------------------------------------------------------------------------------------
# host-only entry points
# ---------------------------------------------------------------------------------------------
def test_defaults_and_null_arguments_without_a_device():
    lib = K.device_lib()
    t = K.TemporalParams()
    assert lib.moptix_temporal_defaults(C.byref(t)) == K.MOPTIX_OK
    got = dict(alpha=t.alpha, alpha_moments=t.alphaMoments, depth_tolerance=t.depthTolerance, normal_threshold=t.normalThreshold,
               max_history=t.maxHistory, variance_frames=t.varianceFrames)
    assert {k: np.float32(v) for k, v in got.items()} == {k: np.float32(v) for k, v in TEMPORAL_DEFAULTS.items()}
    assert lib.moptix_temporal_defaults(None) == K.ERR_INVALID
    p = K.DenoiseParams()
    assert lib.moptix_denoise_defaults(C.byref(p)) == K.MOPTIX_OK
    assert lib.moptix_denoise_temporal(None, C.byref(p), C.byref(t), 1.0) == K.ERR_INVALID
    assert lib.moptix_temporal_reset(None) == K.ERR_INVALID
    assert lib.moptix_temporal_info(None, C.byref(K.TemporalStats())) == K.ERR_INVALID
    assert lib.moptix_temporal_read(None, C.byref(K.TemporalBuffers())) == K.ERR_INVALID


def test_parameter_ranges_are_checked_before_anything_needs_a_device():
    """The argument checks of moptix_denoise_temporal run before the context is looked at, so they can be reached without a GPU: with a
    NULL context a bad parameter is reported as that parameter (the library's own error text), good ones as the null context."""
    lib = K.device_lib()
    lib.moptix_last_error.argtypes = [C.c_void_p]; lib.moptix_last_error.restype = C.c_char_p
    p = K.DenoiseParams()
    assert lib.moptix_denoise_defaults(C.byref(p)) == K.MOPTIX_OK

    def why(field=None, value=None, n_acc=1.0, denoise=None):
        t = K.TemporalParams()
        assert lib.moptix_temporal_defaults(C.byref(t)) == K.MOPTIX_OK
        if field:
            setattr(t, field, value)
        q = K.DenoiseParams.from_buffer_copy(p)
        if denoise:
            setattr(q, denoise[0], denoise[1])
        assert lib.moptix_denoise_temporal(None, C.byref(q), C.byref(t), n_acc) == K.ERR_INVALID
        return lib.moptix_last_error(None).decode()
    assert "null context" in why()
    for field, bad, word in (("alpha", -0.1, "alpha"), ("alpha", 1.5, "alpha"), ("alphaMoments", float("nan"), "alphaMoments"),
                             ("alphaMoments", 2.0, "alphaMoments"), ("depthTolerance", -1.0, "depthTolerance"),
                             ("depthTolerance", float("inf"), "depthTolerance"), ("normalThreshold", 1.5, "normalThreshold"),
                             ("normalThreshold", -2.0, "normalThreshold"), ("normalThreshold", float("nan"), "normalThreshold"),
                             ("maxHistory", 0, "maxHistory"), ("maxHistory", 65537, "maxHistory"), ("varianceFrames", 0, "varianceFrames"),
                             ("varianceFrames", -3, "varianceFrames")):
        assert word in why(field, bad), (field, bad)
    for field, good in (("alpha", 0.0), ("alpha", 1.0), ("depthTolerance", 0.0), ("normalThreshold", -1.0), ("normalThreshold", 1.0),
                        ("maxHistory", 1), ("maxHistory", 65536), ("varianceFrames", 65536)):
        assert "null context" in why(field, good), (field, good)
    assert "nAccumulation" in why(n_acc=0.0) and "nAccumulation" in why(n_acc=float("nan"))
    assert "iterations" in why(denoise=("iterations", 9)) and "normalPower" in why(denoise=("normalPower", 0))
    t = K.TemporalParams()
    assert lib.moptix_denoise_temporal(None, None, C.byref(t), 1.0) == K.ERR_INVALID
    assert lib.moptix_denoise_temporal(None, C.byref(p), None, 1.0) == K.ERR_INVALID


# ---------------------------------------------------------------------------------------------
# quality: >= 6 frames at 4 spp on disjoint seeds, the last frame against 512 spp of its own scene and camera
# ---------------------------------------------------------------------------------------------
FRAMES, SPP = 6, 4


def _sequence(kind):
    """yields (scene of frame k, camera, sphere centres)"""
    if kind == "cornell_quads":
        hs = M.HostScene(kind, 192, 108)
        for k in range(FRAMES):
            p = moved_camera(hs.params, (0.004 * k, 0.002 * k, 0.0))
            yield MovedScene(hs, params=p), cam_of(p), None
    else:
        hs = M.HostScene("random_spheres", 192, 108, iarg=60)
        sph, n = sphere_array(hs)
        angle = C.c_float(0.0)
        for k in range(FRAMES):
            K.host_lib().mohost_animate_spheres(sph, n, 0.002, C.byref(angle))
            p = K.Params.from_buffer_copy(hs.params)
            K.host_lib().mohost_video_camera(angle.value, 192 / 108, C.byref(p.cam))
            frame = copy_spheres(sph, n)
            yield MovedScene(hs, spheres=frame, params=p), cam_of(p), centres_of(frame, n)


# measured with this test (DESIGN.md "Denoiser", temporal table): last-frame RMSE of the temporal entry over the spatial denoiser's
MEASURED = {"cornell_quads": 0.750, "random_spheres": 0.786}


@pytest.mark.parametrize("kind", ["cornell_quads", "random_spheres"])
def test_temporal_beats_the_spatial_denoiser_on_the_last_frame(kind, record_property):
    sim = TemporalSim()
    for k, (scene, cam, centres) in enumerate(_sequence(kind)):
        seeds = M.launch_seeds(SPP, 0, 100 * k)
        accum, _ = hostsim_render(scene, seeds)
        aovs = aovsim_render(scene, seeds)
        got = sim.run(accum, aovs, SPP, aovs["samples"], cam, centres)
    ref, _ = hostsim_render(scene, M.launch_seeds(512, 0, 5000))
    ref = ref / np.float32(512)
    spatial = denoisesim(accum, aovs, SPP, aovs["samples"])
    geo = aovs["hits"][..., 0] > 0
    share = float((got["history"][geo] >= TEMPORAL_DEFAULTS["variance_frames"]).mean())
    e_noisy, e_sp, e_tp = rmse(accum / np.float32(SPP), ref), rmse(spatial, ref), rmse(got["out"], ref)
    ratio = e_tp / e_sp
    record_property("rmse_ratio", ratio)
    print("%s 192x108 frame %d: RMSE noisy %.4f, spatial %.4f, temporal %.4f, temporal / spatial %.3f; h >= %d on %.3f of the geometry pixels, "
          "mean h %.2f" % (kind, FRAMES, e_noisy, e_sp, e_tp, ratio, TEMPORAL_DEFAULTS["variance_frames"], share, got["info"]["mean_history"]))
    assert share >= 0.5                                    # the sequence really keeps its history
    assert e_tp < e_sp
    if MEASURED[kind] is not None:
        assert ratio <= MEASURED[kind] * 1.1
