"""The packet kernel's lean build (csrc/packetkernel.hip: no FEAT_* program of csrc/pt_types.h compiled in) against the general one.

A scene whose tables cannot reach the texture path, the sphere-light draw, the Lambertian / metal / glass programs or the analytic
sphere loops runs the lean build (option "specialize", default 1; "kernel_features_used" reports the mask of the last launch's trace
kernel, 15 = every program).  What it leaves out is control flow the tables rule out, so every accumulator bit must be the general
kernel's, the queue kernel's and the per-lane kernel's; a scene with any ONE of the features must stay on the general kernel; and the
choice is made per launch from the tables as they are then.  320x180 frames, two launches, through the C ABI."""
import ctypes as C
import math

import numpy as np
import pytest

from common import M
from packet_helpers import DRAIN_DEFAULT, FEAT_ALL, bits as _bits, packet_ctx, write_floor_block_scene      # noqa: F401 (packet_ctx: a fixture)

pytestmark = pytest.mark.gpu

K = M._capi
W, H = 320, 180
FEAT_TEXTURE, FEAT_SPHERE_LIGHT, FEAT_PLAIN_MATERIALS, FEAT_SPHERES = 1, 2, 4, 8
SEEDS = M.launch_seeds(2)


def _render(ctx, counted=False):
    ctx.accum_clear()
    st = ctx.render_counted(SEEDS) if counted else ctx.render(SEEDS)
    return ctx.accum_read(), st


# ---- lean scene, the same bits ---------------------------------------------------------------------------------------------------------

def _lean_scene(name, tmp_path):
    """coffee: the benchmark scene (no Disney GLASS material: the NEAR = false kernels).  panes: a Disney GLASS pane over an opaque one
    under a quad light (tests/common.py) -- lean-eligible as well, and the only way to the NEAR = true lean kernels."""
    if name == "coffee":
        return M.HostScene("file:coffee", W, H)
    from common import write_glass_over_opaque_scene
    return M.HostScene("file:cornell", W, H, base_folder=write_glass_over_opaque_scene(tmp_path, True))


@pytest.mark.parametrize("node_format", [64, 128])
@pytest.mark.parametrize("drain_below", [DRAIN_DEFAULT, 0])
@pytest.mark.parametrize("scene", ["coffee", "panes"])
def test_lean_kernel_gives_the_general_kernels_bits(packet_ctx, tmp_path, scene, node_format, drain_below):
    ctx = packet_ctx
    hs = _lean_scene(scene, tmp_path)
    ctx.set_option("node_format", node_format); ctx.set_option("drain_below", drain_below)
    ctx.load(hs)
    lean, _ = _render(ctx)
    assert ctx.get_option("kernel_variant_used") == 4 and ctx.get_option("node_format_used") == node_format
    assert ctx.get_option("kernel_features_used") == 0
    assert lean.any()
    _, st_lean = _render(ctx, counted=True)                   # the counting build is a general one
    assert ctx.get_option("kernel_features_used") == FEAT_ALL
    assert np.array_equal(_bits(ctx.accum_read()), _bits(lean))
    ctx.set_option("specialize", 0)
    general, _ = _render(ctx)
    assert ctx.get_option("kernel_variant_used") == 4 and ctx.get_option("kernel_features_used") == FEAT_ALL
    assert np.array_equal(_bits(general), _bits(lean))
    _, st_general = _render(ctx, counted=True)
    for f in ("primaryRays", "bounceRays", "shadowRays", "closestHits"):
        assert getattr(st_lean, f) == getattr(st_general, f) and getattr(st_lean, f) > 0, f
    ctx.set_option("specialize", 1)
    for variant in (3, 0):
        ctx.set_option("kernel_variant", variant)
        other, _ = _render(ctx)
        assert ctx.get_option("kernel_variant_used") == variant and ctx.get_option("kernel_features_used") == FEAT_ALL
        assert np.array_equal(_bits(other), _bits(lean)), "variant %d" % variant


# ---- each feature alone keeps the general kernel -----------------------------------------------------------------------------------------

def _write_base_scene(tmp_path):
    """Untextured Disney meshes under one quad light: a floor, a back wall and a block -- lean-eligible, within variant 4's limits."""
    return M.HostScene("file:cornell", W, H, base_folder=write_floor_block_scene(tmp_path))


def _f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _add_material(ctx, m):
    mid = C.c_int32()
    ctx._chk(ctx._L.moptix_add_material(ctx._h, C.byref(m), C.byref(mid)))
    return mid.value


def _add_panel(ctx, mat, with_uv):
    """A tilted two-triangle panel in front of the back wall, left of the block."""
    pos = np.array([[-2.2, 0.2, 1.2], [-2.2, 1.6, 1.5], [-1.0, 1.6, 1.5], [-1.0, 0.2, 1.2]], np.float32)
    uv = np.array([[-0.3, 0.0], [-0.3, 1.7], [1.4, 1.7], [1.4, 0.0]], np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    ctx._chk(ctx._L.moptix_add_mesh(ctx._h, _f32p(pos), 4, None, 0, _f32p(uv) if with_uv else None, 4 if with_uv else 0,
                                    _i32p(idx), None, _i32p(idx) if with_uv else None, 2, mat))


def _disney_like(hs, i=0):
    return K.Material.from_buffer_copy(hs.flat()["materials"][i])


def _add_textured_panel(ctx, hs):
    yy, xx = np.mgrid[0:8, 0:8]
    px = np.ones((8, 8, 4), np.float32)
    px[..., 0] = np.where((xx + yy) % 2 == 0, 0.9, 0.1); px[..., 1] = xx / 7.0; px[..., 2] = yy / 7.0
    tid = C.c_int32()
    ctx._chk(ctx._L.moptix_add_texture(ctx._h, _f32p(px), 8, 8, C.byref(tid)))
    m = _disney_like(hs)
    assert m.kind == K.MAT_DISNEY
    m.disney.albedoID = tid.value
    _add_panel(ctx, _add_material(ctx, m), with_uv=True)


def _set_light(ctx, sphere):
    l = K.LightParams()
    if sphere:
        l.shape = K.LIGHT_SPHERE
        l.position = K.Float3(1.0, 2.2, -0.5); l.radius = 0.4; l.area = 4.0 * math.pi * 0.4 * 0.4
        l.normal = K.Float3(0, -1, 0); l.emission = K.Float3(25, 25, 25)
    else:
        l.shape = K.LIGHT_QUAD
        l.position = K.Float3(-1, 2.5, -1); l.u = K.Float3(1, 0, 0); l.v = K.Float3(0, 0, 1)
        l.normal = K.Float3(0, -1, 0); l.area = 1.0; l.emission = K.Float3(12, 12, 12)
    ctx._chk(ctx._L.moptix_set_lights(ctx._h, C.byref(l), 1))


def _add_lambertian_panel(ctx, hs, kind=None):
    m = K.Material()
    m.kind = K.MAT_LAMBERTIAN if kind is None else kind
    m.albedo = K.Float3(0.2, 0.6, 0.8); m.fuzz = 0.1; m.refIdx = 1.5
    _add_panel(ctx, _add_material(ctx, m), with_uv=False)


def _add_emissive_sphere(ctx, hs):
    """An analytic sphere beside the meshes.  Its material is a light's (no Disney material on an analytic primitive: variant 4's limit)."""
    m = K.Material()
    m.kind = K.MAT_LIGHT
    m.emission = K.Float3(3, 2, 1)
    s = K.SphereParams()
    s.radius = 0.35; s.center = K.Float3(1.6, 0.35, 0.6)
    mid = np.array([_add_material(ctx, m)], np.int32)
    ctx._chk(ctx._L.moptix_add_spheres(ctx._h, C.byref(s), _i32p(mid), 1))


FEATURES = {
    "texture": (FEAT_TEXTURE, _add_textured_panel),
    "sphere_light": (FEAT_SPHERE_LIGHT, lambda ctx, hs: _set_light(ctx, True)),
    "lambertian": (FEAT_PLAIN_MATERIALS, _add_lambertian_panel),
    "metal": (FEAT_PLAIN_MATERIALS, lambda ctx, hs: _add_lambertian_panel(ctx, hs, K.MAT_METAL)),
    "glass": (FEAT_PLAIN_MATERIALS, lambda ctx, hs: _add_lambertian_panel(ctx, hs, K.MAT_GLASS)),
    "sphere": (FEAT_SPHERES, _add_emissive_sphere),
}


def _load_with(ctx, hs, change):
    ctx.load(hs)
    if change is not None:
        change(ctx, hs)
        ctx.build_accel("Trbvh")
        ctx._chk(ctx._L.moptix_validate(ctx._h))


@pytest.mark.parametrize("node_format", [64, 128])
@pytest.mark.parametrize("feature", sorted(FEATURES))
def test_one_feature_keeps_the_general_kernel(packet_ctx, tmp_path, feature, node_format):
    ctx = packet_ctx
    bit, change = FEATURES[feature]
    hs = _write_base_scene(tmp_path)
    ctx.set_option("node_format", node_format)
    _load_with(ctx, hs, None)
    base, _ = _render(ctx)
    assert ctx.get_option("kernel_variant_used") == 4 and ctx.get_option("kernel_features_used") == 0      # the base scene is lean
    _load_with(ctx, hs, change)
    g, _ = _render(ctx)
    assert ctx.get_option("kernel_variant_used") == 4 and ctx.get_option("node_format_used") == node_format
    used = ctx.get_option("kernel_features_used")
    assert used & bit and used == FEAT_ALL
    assert not np.array_equal(_bits(g), _bits(base))          # the feature is visible in the frame
    ctx.set_option("kernel_variant", 0)
    ref, _ = _render(ctx)
    assert ctx.get_option("kernel_variant_used") == 0
    assert np.array_equal(_bits(g), _bits(ref))


# ---- the choice is not stale -------------------------------------------------------------------------------------------------------------

def _fresh_render(hs, change):
    ctx = M.Context(0)
    try:
        ctx.set_option("kernel_variant", 4)
        _load_with(ctx, hs, change)
        img, _ = _render(ctx)
        return img, ctx.get_option("kernel_features_used")
    finally:
        ctx.close()


def _rebuild(ctx):
    ctx.build_accel("Trbvh")
    ctx._chk(ctx._L.moptix_validate(ctx._h))


def test_the_choice_follows_the_scene_between_launches(packet_ctx, tmp_path):
    ctx = packet_ctx
    hs = _write_base_scene(tmp_path)
    _load_with(ctx, hs, None)
    lean, _ = _render(ctx)
    assert ctx.get_option("kernel_features_used") == 0
    # a sphere light comes ...
    _set_light(ctx, True); _rebuild(ctx)
    lit, _ = _render(ctx)
    assert ctx.get_option("kernel_features_used") == FEAT_ALL
    fresh, used = _fresh_render(hs, lambda c, h: _set_light(c, True))
    assert used == FEAT_ALL and np.array_equal(_bits(lit), _bits(fresh)) and not np.array_equal(_bits(lit), _bits(lean))
    # ... and goes: moptix_set_lights replaces the table
    _set_light(ctx, False); _rebuild(ctx)
    back, _ = _render(ctx)
    assert ctx.get_option("kernel_features_used") == 0
    fresh, used = _fresh_render(hs, lambda c, h: _set_light(c, False))
    assert used == 0 and np.array_equal(_bits(back), _bits(fresh))
    # a textured material comes, assigned to new faces ...
    _add_textured_panel(ctx, hs); _rebuild(ctx)
    tex, _ = _render(ctx)
    assert ctx.get_option("kernel_features_used") == FEAT_ALL

    def light_then_panel(c, h):
        _set_light(c, False); _add_textured_panel(c, h)
    fresh, used = _fresh_render(hs, light_then_panel)
    assert used == FEAT_ALL and np.array_equal(_bits(tex), _bits(fresh)) and not np.array_equal(_bits(tex), _bits(back))
    # ... and only a new scene takes a material out of the table again
    _load_with(ctx, hs, None)
    again, _ = _render(ctx)
    assert ctx.get_option("kernel_features_used") == 0 and np.array_equal(_bits(again), _bits(lean))


def test_specialize_is_an_option_and_kernel_features_used_is_read_only(gpu_ctx):
    assert gpu_ctx.get_option("specialize") == 1
    with pytest.raises(M.MoptixError):
        gpu_ctx.set_option("specialize", 2)
    with pytest.raises(M.MoptixError):
        gpu_ctx.set_option("kernel_features_used", 0)
