"""Helpers of the packet-kernel GPU tests: the builds a launch can run (general, lean with borrowed slots, slim) are told apart by the
read-only options "kernel_variant_used", "kernel_features_used" and "kernel_slim_used"."""
import numpy as np
import pytest

from common import M

FEAT_ALL = 15          # "kernel_features_used": every FEAT_* program of csrc/pt_types.h
DRAIN_DEFAULT = 64     # options as moptix_create leaves them
AUX_DEFAULT = 16
OPTION_DEFAULTS = (("kernel_variant", -1), ("node_format", 0), ("specialize", 1), ("drain_below", DRAIN_DEFAULT), ("aux_depth", AUX_DEFAULT),
                   ("slots_in_use", -1), ("shadow_rule", 1))
OTHER_SEEDS = M.launch_seeds(2, first=100)


def bits(a):
    return a.view(np.uint32)


@pytest.fixture
def packet_ctx(gpu_ctx):
    """The session's context with the packet kernel asked for; every option the packet tests touch goes back to its default afterwards."""
    gpu_ctx.set_option("kernel_variant", 4)
    yield gpu_ctx
    gpu_ctx.set_partition(0, 1)
    for name, value in OPTION_DEFAULTS:
        gpu_ctx.set_option(name, value)


def kernel_used(ctx):
    return ctx.get_option("kernel_variant_used"), ctx.get_option("kernel_features_used"), ctx.get_option("kernel_slim_used")


def render_after_other_seeds(ctx, seeds, **options):
    """One frame of `seeds` under `options`, after a frame of other seeds under the same options: the per-sample buffer then holds nothing
    an unfinished sample could pass for.  Returns the frame and (variant, features, slim) of its trace kernel."""
    for name, value in options.items():
        ctx.set_option(name, value)
    ctx.accum_clear(); ctx.render(OTHER_SEEDS)
    ctx.accum_clear(); ctx.render(seeds)          # raises if the watchdog flag is set (tests/test_gpu_configs.py)
    return ctx.accum_read(), kernel_used(ctx)


def write_floor_block_scene(root, block_material="Block", floor_material="Floor", tilted_normals=False):
    """Untextured Disney meshes under one quad light: a floor and a back wall with vertex normals (tilted_normals: two different ones per
    face), a block without -- lean-eligible, within variant 4's limits.  Returns the base folder for M.HostScene("file:cornell", ...)."""
    d = root / "scenes" / "cornell"
    d.mkdir(parents=True, exist_ok=True)
    if tilted_normals:
        (d / "floor.obj").write_text("v -3 0 -2\nv -3 0 2\nv 3 0 2\nv 3 0 -2\nvn 0 1 0\nvn 0.2 0.9 0.1\nf 1//1 2//2 3//1 4//2\n"
                                     "v -3 0 2\nv -3 3.4 2\nv 3 3.4 2\nv 3 0 2\nvn 0 0 -1\nvn 0.1 0.2 -0.9\nf 5//3 6//4 7//3 8//4\n")
    else:
        (d / "floor.obj").write_text("v -3 0 -2\nv -3 0 2\nv 3 0 2\nv 3 0 -2\nvn 0 1 0\nf 1//1 2//1 3//1 4//1\n"
                                     "v -3 0 2\nv -3 3.4 2\nv 3 3.4 2\nv 3 0 2\nvn 0 0 -1\nf 5//2 6//2 7//2 8//2\n")
    (d / "block.obj").write_text(
        "v -0.5 0 -0.5\nv 0.5 0 -0.5\nv 0.5 0 0.5\nv -0.5 0 0.5\nv -0.5 0.8 -0.5\nv 0.5 0.8 -0.5\nv 0.5 0.8 0.5\nv -0.5 0.8 0.5\n"
        "f 5 8 7 6\nf 1 2 6 5\nf 2 3 7 6\nf 3 4 8 7\nf 4 1 5 8\n")
    (d / "cornell.scene").write_text(
        "material Floor\n{\n\tcolor 0.7 0.7 0.7\n\troughness 0.6\n}\n"
        "material Block\n{\n\tcolor 0.8 0.3 0.2\n\troughness 0.3\n\tclearcoat 0.5\n}\n"
        "mesh\n{\n\tfile floor.obj\n\tmaterial %s\n}\n"
        "mesh\n{\n\tfile block.obj\n\tmaterial %s\n}\n"
        "light\n{\n\ttype Quad\n\tposition -1 2.5 -1\n\tv1 0 2.5 -1\n\tv2 -1 2.5 0\n\temission 12 12 12\n}\n" % (floor_material, block_material))
    return str(root / "scenes") + "/"
