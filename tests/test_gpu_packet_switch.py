"""The packet kernel's ray switch in the scheduler loop (csrc/packetkernel_body.h, SWITCH) against the general build, which keeps it in the leaf pass.

A packet holds up to three shadow rays and the continuation, traced one after the other.  Where a ray ends in the node loop (a step that enters
no child with an empty stack: an unoccluded shadow ray, a miss) and the packet holds another one, the slim kernels with SWITCH load the next
ray's row in the loop's leave handler and put the slot back on the wave's node ring one iteration later; every other kernel sends the slot
through a leaf pass.  Same rays, same order, same arithmetic: the accumulation buffer of the slim build ("kernel_slim_used" 1) must equal the
general build's ("specialize" 0) bit for bit -- on both node formats, on the NEAR slim kernel (a Disney GLASS pane under "shadow_rule" 1: its
shadow rays never end early, every one ends by exhaustion), with pools down to their last paths while switches are pending and paths handed to
the drain kernel, as each rank of a partition, after a vertex update with refit, and in the adaptive pass.  A render raises if the watchdog
flag is set, so every case also says that no slot was lost.  64x64 frames, "kernel_variant" 4 and "aux_depth" 0 so that a launch this small
runs the slim build at all; a render under test follows a render of other seeds (tests/packet_helpers.py says why)."""
import numpy as np
import pytest

from common import M, write_glass_over_opaque_scene
from packet_helpers import FEAT_ALL, bits as _bits, kernel_used, packet_ctx as _packet_ctx, render_after_other_seeds

pytestmark = pytest.mark.gpu

W = H = 64


@pytest.fixture(scope="module")
def coffee():
    return M.HostScene("file:coffee", W, H)


@pytest.fixture
def packet_ctx(_packet_ctx):
    """tests/packet_helpers.py packet_ctx, and no borrowed slots."""
    _packet_ctx.set_option("aux_depth", 0)
    return _packet_ctx


def _render(ctx, seeds, specialize):
    """One frame of `seeds` by the slim build (`specialize` 1) or the general one (0), after a frame of other seeds."""
    frame, used = render_after_other_seeds(ctx, seeds, specialize=specialize)
    assert used == ((4, 0, 1) if specialize else (4, FEAT_ALL, 0)), used
    return frame


def _slim_equals_general(ctx, seeds, what):
    slim, general = _render(ctx, seeds, 1), _render(ctx, seeds, 0)
    assert slim.any() and np.isfinite(slim).all(), what
    diff = int((_bits(slim) != _bits(general)).any(axis=-1).sum())
    assert diff == 0, "%s: %d pixels differ between the slim and the general kernel" % (what, diff)
    return slim


@pytest.mark.parametrize("node_format", [64, 128])
def test_coffee_on_both_node_formats(packet_ctx, coffee, node_format):
    """Every lit hit makes a packet of two to four rays, and unoccluded shadow rays end in the node loop."""
    ctx = packet_ctx
    ctx.set_option("node_format", node_format)
    ctx.load(coffee)
    _slim_equals_general(ctx, M.launch_seeds(4), "coffee, %d-byte nodes" % node_format)
    assert ctx.get_option("node_format_used") == node_format


@pytest.mark.parametrize("glass_below", [True, False])
def test_glass_panes_on_the_near_kernel(packet_ctx, tmp_path, glass_below):
    ctx = packet_ctx
    ctx.set_option("shadow_rule", 1)
    ctx.load(M.HostScene("file:cornell", W, H, base_folder=write_glass_over_opaque_scene(tmp_path, glass_below)))
    _slim_equals_general(ctx, M.launch_seeds(4), "glass pane %s the opaque one" % ("below" if glass_below else "above"))


@pytest.mark.parametrize("slots_in_use,drain_below", [(64, 0), (64, 64), (32, 64)])
def test_pools_down_to_their_last_paths(packet_ctx, coffee, slots_in_use, drain_below):
    """64 (32) slots per pool and one sample per pixel: the pools run out of work items while ray switches are pending; with "drain_below" at
    or above "slots_in_use" a pool hands its paths to the drain kernel as soon as the work counter is exhausted."""
    ctx = packet_ctx
    ctx.set_option("slots_in_use", slots_in_use)
    ctx.set_option("drain_below", drain_below)
    ctx.load(coffee)
    _slim_equals_general(ctx, M.launch_seeds(1), "slots_in_use %d drain_below %d" % (slots_in_use, drain_below))


def test_each_rank_of_two(packet_ctx, coffee):
    ctx = packet_ctx
    seeds = M.launch_seeds(4)
    ctx.load(coffee)
    whole = _render(ctx, seeds, 1)
    covered = np.zeros((H, W), bool)
    for rank in (0, 1):
        ctx.set_partition(rank, 2); ctx.load(coffee)
        part = _slim_equals_general(ctx, seeds, "rank %d of 2" % rank)
        mine = part.any(axis=-1)
        assert mine.any() and not mine.all()
        assert np.array_equal(_bits(part)[mine], _bits(whole)[mine])
        covered |= mine
    assert np.array_equal(covered, whole.any(axis=-1))


def test_after_a_vertex_update_with_refit(packet_ctx, coffee):
    ctx = packet_ctx
    seeds = M.launch_seeds(4)
    ctx.load(coffee)
    before = _slim_equals_general(ctx, seeds, "before the update")
    pos, nrm, _, _ = coffee.face_arrays()
    pos = pos.reshape(-1, 3, 3).copy()
    pos[..., 0] += np.float32(0.2) * pos[..., 1]          # the scene leans over: every box of the tree changes, its topology stays
    ctx.update_faces(0, pos, nrm)
    ctx.refit_accel()
    after = _slim_equals_general(ctx, seeds, "after update + refit")
    assert not np.array_equal(_bits(before), _bits(after))


def test_adaptive_pass(packet_ctx, coffee):
    """The adaptive passes hand a subset of the pixels out through their own order list."""
    ctx = packet_ctx
    ctx.load(coffee)
    seeds = M.launch_seeds(24)
    got = []
    for specialize in (1, 0):
        ctx.set_option("specialize", specialize)
        ctx.adaptive_clear()
        st = ctx.render_adaptive(seeds, threshold=0.05, min_samples=8, batch=8)
        assert kernel_used(ctx) == ((4, 0, 1) if specialize else (4, FEAT_ALL, 0)), kernel_used(ctx)
        assert st["passes"] >= 2 and st["samples_traced"] < st["samples_uniform"]      # some pass rendered a subset of the pixels
        got.append((ctx.accum_read(), ctx.adaptive_read()["count"]))
    ctx.accum_clear()      # leave the context to plain renders
    assert got[0][0].any()
    assert np.array_equal(got[0][1], got[1][1])
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0]))
