"""The packet kernel's slim build (csrc/packetkernel.hip: pt_packetkernel, lean, AUX = false, GLASS = NEAR) against its twin with borrowed
slots and glass (pt_packetkernel_aux), the general build and the per-lane kernel.

A lean launch that borrows no slot ("aux_depth" 0, or 1e8 samples and more with "slots_in_use" left alone) in a scene without a Disney
GLASS material -- or with one under "shadow_rule" 1, where shadow rays keep their nearest candidate -- runs the slim build
("kernel_slim_used" 1).  What it leaves out is code such a launch cannot reach, so every accumulator bit must be the other builds'.
Small frames, "kernel_variant" 4 set explicitly so that they reach the packet kernel at all.  A render under test always follows a render
of OTHER seeds (tests/packet_helpers.py render_after_other_seeds says why)."""
import numpy as np
import pytest

from common import M, write_glass_over_opaque_scene
from packet_helpers import DRAIN_DEFAULT, FEAT_ALL, bits as _bits, packet_ctx, render_after_other_seeds as _render      # noqa: F401 (packet_ctx: a fixture)

pytestmark = pytest.mark.gpu


def test_coffee_slim_gives_the_bits_of_the_twin_with_borrowed_slots_the_general_build_and_the_per_lane_kernel(packet_ctx):
    ctx = packet_ctx
    seeds = M.launch_seeds(4)
    ctx.load(M.HostScene("file:coffee", 96, 54))
    slim, used = _render(ctx, seeds, aux_depth=0)
    assert used == (4, 0, 1), used
    assert slim.any()
    # the twin, with borrowed slots really in use: 128 of the 576 slots carry no path from the start, every path of depth >= 1 borrows
    twin, used = _render(ctx, seeds, aux_depth=1, slots_in_use=448)
    assert used == (4, 0, 0), used
    assert np.array_equal(_bits(twin), _bits(slim))
    general, used = _render(ctx, seeds, aux_depth=0, slots_in_use=-1, specialize=0)
    assert used == (4, FEAT_ALL, 0), used
    assert np.array_equal(_bits(general), _bits(slim))
    lane, used = _render(ctx, seeds, specialize=1, kernel_variant=0)
    assert used == (0, FEAT_ALL, 0), used
    assert np.array_equal(_bits(lane), _bits(slim))


@pytest.mark.parametrize("glass_below", [True, False])
@pytest.mark.parametrize("shadow_rule", [1, 0])
def test_glass_panes_run_the_slim_build_only_where_shadow_rays_keep_their_nearest_candidate(packet_ctx, tmp_path, shadow_rule, glass_below):
    """A Disney GLASS pane and an opaque one between the floor and the light: under "shadow_rule" 1 the NEAR kernels run, whose slim build
    keeps the glass code; under 0 the NEAR = false kernels, whose slim build has none -- the material table keeps the launch on the twin."""
    ctx = packet_ctx
    seeds = M.launch_seeds(4)
    ctx.set_option("shadow_rule", shadow_rule)
    ctx.load(M.HostScene("file:cornell", 96, 54, base_folder=write_glass_over_opaque_scene(tmp_path, glass_below)))
    lean, used = _render(ctx, seeds, aux_depth=0)
    assert used == (4, 0, 1 if shadow_rule == 1 else 0), used
    assert lean.any()
    general, used = _render(ctx, seeds, specialize=0)
    assert used == (4, FEAT_ALL, 0), used
    assert np.array_equal(_bits(general), _bits(lean))


def _closed_box(tmp_path, width, height):
    """A closed cube of twelve triangles, a near-white, near-specular Disney material inside and out, a small quad light under its lid, and
    the camera moved to its centre: a path ends only where it meets the light or where a sample fails, so most of them walk to the
    256-bounce cap."""
    d = tmp_path / "scenes" / "cornell"
    d.mkdir(parents=True)
    (d / "box.obj").write_text("v -1 -1 -1\nv 1 -1 -1\nv 1 1 -1\nv -1 1 -1\nv -1 -1 1\nv 1 -1 1\nv 1 1 1\nv -1 1 1\n"
                               "f 1 2 3 4\nf 8 7 6 5\nf 1 5 6 2\nf 2 6 7 3\nf 3 7 8 4\nf 4 8 5 1\n")
    (d / "cornell.scene").write_text(
        "material Wall\n{\n\tcolor 0.95 0.95 0.95\n\troughness 0.05\n}\n"
        "mesh\n{\n\tfile box.obj\n\tmaterial Wall\n}\n"
        "light\n{\n\ttype Quad\n\tposition -0.1 0.98 -0.1\n\tv1 0.1 0.98 -0.1\n\tv2 -0.1 0.98 0.1\n\temission 40 40 40\n}\n")
    hs = M.HostScene("file:cornell", width, height, base_folder=str(tmp_path / "scenes") + "/")
    p = hs.params
    cam = p.cam
    for ax in "xyz":                      # the cornell camera looks at the box's centre from outside: the same view from the centre itself
        shift = 0.0 - getattr(cam.origin, ax)
        setattr(cam.scrLowerLeftCorner, ax, getattr(cam.scrLowerLeftCorner, ax) + shift)
        setattr(cam.origin, ax, 0.0)
    return hs, p


@pytest.mark.parametrize("drain_below", [0, DRAIN_DEFAULT])
def test_capped_paths_finish_without_borrowed_slots(packet_ctx, tmp_path, drain_below):
    """The launch's tail without borrowed slots, with the drain kernel and without: every sample is finished (the bits are the per-lane
    kernel's, after a frame of other seeds) and the watchdog flag is clear (the render returns)."""
    ctx = packet_ctx
    seeds = M.launch_seeds(2)
    hs, params = _closed_box(tmp_path, 32, 18)
    ctx.load(hs)
    ctx.set_params(params)
    ctx.set_option("drain_below", drain_below)
    slim, used = _render(ctx, seeds, aux_depth=0)
    assert used == (4, 0, 1), used
    assert slim.any() and np.isfinite(slim).all()
    ctx.accum_clear()
    st = ctx.render_counted(seeds)                 # the counting build: the premise, and the same bits once more
    print("closed box: %d samples, %d bounce rays, %.1f per sample" % (st.samples, st.bounceRays, st.bounceRays / max(1, st.samples)))
    assert st.samples == 32 * 18 * 2
    assert st.bounceRays >= 100 * st.samples       # a mean of 100 bounces under a cap of 256: most paths walk to the cap
    assert np.array_equal(_bits(ctx.accum_read()), _bits(slim))
    lane, used = _render(ctx, seeds, kernel_variant=0)
    assert used == (0, FEAT_ALL, 0), used
    assert np.array_equal(_bits(lane), _bits(slim))
