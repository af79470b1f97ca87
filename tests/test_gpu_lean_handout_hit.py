"""The lean packet kernel's own hand-out and hit record against the general kernel (csrc/megakernel.h handout_lean, csrc/pt_types.h TriFace).

The lean build (option "specialize" 1, "kernel_features_used" 0) maps a hand-out index to its pixel with one routine of its own and reads a
hit's face from one 64-byte record that holds the geometric normal ready-made; the general build ("specialize" 0, features 15) keeps
handout_to_item / item_to_pixel and Tri48 + TriShade.  Same integers, same float operations on the same inputs: every accumulator bit must
agree -- for each hand-out order, as each rank of a partition, with and without vertex normals, on the NEAR kernels (a Disney GLASS pane),
after a vertex update with refit and after a change of the faces' materials (a stale face record would show there), and through the
adaptive pass's order list.  37x19 frames (neither side a multiple of the 8x8 tile), 3 and 17 launch seeds, variant 4 forced."""
import numpy as np
import pytest

from common import M, write_glass_over_opaque_scene
from packet_helpers import FEAT_ALL, bits as _bits, write_floor_block_scene

pytestmark = pytest.mark.gpu

W, H = 37, 19
SEED_COUNTS = (3, 17)


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    c.set_option("kernel_variant", 4)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults(ctx):
    yield
    ctx.set_option("specialize", 1); ctx.set_option("tile_major", 3); ctx.set_partition(0, 1)


def _scene(name, tmp_path, width=W, height=H, **kw):
    if name == "panes":      # a Disney GLASS pane over an opaque one (tests/common.py): the NEAR = true lean kernels; every face has normals
        return M.HostScene("file:cornell", width, height, base_folder=write_glass_over_opaque_scene(tmp_path, True))
    # a floor and a back wall WITH vertex normals, a block WITHOUT
    return M.HostScene("file:cornell", width, height, base_folder=write_floor_block_scene(tmp_path, tilted_normals=True, **kw))


def _render(ctx, n, specialize):
    ctx.set_option("specialize", specialize)
    ctx.accum_clear()
    ctx.render(M.launch_seeds(n))
    assert ctx.get_option("kernel_variant_used") == 4
    assert ctx.get_option("kernel_features_used") == (0 if specialize else FEAT_ALL)
    return ctx.accum_read()


def _lean_equals_general(ctx, what=""):
    """Both builds for each seed count; returns the lean frames."""
    out = []
    for n in SEED_COUNTS:
        lean, general = _render(ctx, n, 1), _render(ctx, n, 0)
        assert lean.any(), "%s %d seeds: empty frame" % (what, n)
        diff = int((_bits(lean) != _bits(general)).any(axis=-1).sum())
        assert diff == 0, "%s %d seeds: %d pixels differ between the lean and the general kernel" % (what, n, diff)
        out.append(lean)
    return out


@pytest.mark.parametrize("tile_major", [0, 1, 3])
@pytest.mark.parametrize("scene", ["meshes", "panes"])
def test_lean_kernel_matches_general_for_each_hand_out_order(ctx, tmp_path, scene, tile_major):
    hs = _scene(scene, tmp_path)
    if scene == "meshes":
        has = hs.face_arrays()[2]
        assert has.any() and not has.all()          # faces with vertex normals and faces without
    ctx.set_option("tile_major", tile_major)
    ctx.load(hs)
    _lean_equals_general(ctx, "%s tile_major %d" % (scene, tile_major))


@pytest.mark.parametrize("rank", [0, 1, 2])
def test_lean_kernel_matches_general_as_each_rank_of_three(ctx, tmp_path, rank):
    hs = _scene("meshes", tmp_path)
    ctx.set_partition(0, 1); ctx.load(hs)
    whole = _render(ctx, SEED_COUNTS[0], 1)
    ctx.set_partition(rank, 3); ctx.load(hs)
    part = _lean_equals_general(ctx, "rank %d of 3" % rank)[0]
    # the rank's own tiles hold the whole frame's bits, the other ranks' tiles stay clear
    mine = part.any(axis=-1)
    assert mine.any() and not mine.all()
    assert np.array_equal(_bits(part)[mine], _bits(whole)[mine])


def test_face_records_follow_a_vertex_update_with_refit(ctx, tmp_path):
    hs = _scene("meshes", tmp_path)
    ctx.load(hs)
    before = _lean_equals_general(ctx, "before the update")
    pos, nrm, has, _ = hs.face_arrays()
    pos = pos.reshape(-1, 3, 3).copy(); nrm = nrm.reshape(-1, 3, 3).copy()
    flat = np.where(has == 0)[0]
    # the block (no normals) leans over and grows: p0 and the geometric normal of each of its faces change
    p = pos[flat]
    p[..., 0] += 0.6 * p[..., 1]; p[..., 1] *= 1.5
    pos[flat] = p
    # the floor's and the wall's vertex normals tilt
    nrm[has != 0] += np.float32([0.15, 0.0, 0.1])
    ctx.update_faces(0, pos, nrm)
    ctx.refit_accel()
    after = _lean_equals_general(ctx, "after update + refit")
    for a, b in zip(before, after):
        assert not np.array_equal(_bits(a), _bits(b))
    # the same faces through a build from scratch: the refitted records are the builder's
    ctx.build_accel("Trbvh")
    rebuilt = _lean_equals_general(ctx, "after update + rebuild")
    for a, b in zip(after, rebuilt):
        assert np.array_equal(_bits(a), _bits(b))


def test_face_records_follow_a_change_of_the_faces_materials(ctx, tmp_path):
    ctx.load(_scene("meshes", tmp_path))
    before = _lean_equals_general(ctx, "before the change")
    ctx.load(_scene("meshes", tmp_path, block_material="Floor", floor_material="Block"))      # the same faces, the materials swapped
    after = _lean_equals_general(ctx, "after the change")
    for a, b in zip(before, after):
        assert not np.array_equal(_bits(a), _bits(b))


def test_adaptive_pass_lean_on_against_off(ctx, tmp_path):
    """64x40: the adaptive passes hand their pixels out through their own order list ("tile_major" 3 with PassOverride)."""
    hs = _scene("meshes", tmp_path, width=64, height=40)
    ctx.load(hs)
    seeds = M.launch_seeds(24)
    got = []
    for specialize in (1, 0):
        ctx.set_option("specialize", specialize)
        ctx.adaptive_clear()
        st = ctx.render_adaptive(seeds, threshold=0.05, min_samples=8, batch=8)
        assert ctx.get_option("kernel_variant_used") == 4 and ctx.get_option("kernel_features_used") == (0 if specialize else FEAT_ALL)
        assert st["passes"] >= 2 and st["samples_traced"] < st["samples_uniform"]      # some pass rendered a subset of the pixels
        got.append((ctx.accum_read(), ctx.adaptive_read()["count"]))
    ctx.accum_clear()      # leave the context to plain renders
    assert got[0][0].any()
    assert np.array_equal(got[0][1], got[1][1])
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0]))
