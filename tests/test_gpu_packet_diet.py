"""The slim packet kernels' diet (csrc/packetkernel.hip, DIET) against the general build, which has none of it.

The slim kernels take the node loop's lane mask from ONE compare -- which leans on "a lane without a slot never stands at a node" -- and
feed tmin and tbest to the slab test without a canonicalising instruction.  Neither changes a value: the accumulation buffer of the slim
build ("kernel_slim_used" 1) must equal the general build's ("specialize" 0) bit for bit -- on coffee with both node formats, on a tree deep
enough for the stacks' overflow rows in HBM, on exact duplicates (equal-t ties), at "leaf_size" 1, 4 and 8, as one rank of two, and with
pools down to their last paths (lanes without a slot while others walk).  A render raises if the watchdog flag is set.  Small frames,
"kernel_variant" 4 and "aux_depth" 0 so that a launch this small runs the slim build at all; a render under test follows a render of other
seeds (tests/packet_helpers.py says why).

"leaf_size" 8: the round's issue had a leaf pass of one four-triangle chunk in the slim kernels and therefore wanted such a tree on the twin
("kernel_slim_used" 0).  That step was built, measured, found to be no gain and is not in the code (NOTEBOOK.md round 24): every leaf size
runs the slim kernel, whose leaf pass loops over chunks as before, and the case checks that."""
import numpy as np
import pytest

from common import M
from lbvh_cases import case_scene
from packet_helpers import FEAT_ALL, bits as _bits, packet_ctx as _packet_ctx, render_after_other_seeds

pytestmark = pytest.mark.gpu

W = H = 64
LDS_STACK_ENTRIES = 9      # csrc/packetkernel.hip kStackN: deeper stack levels live in the slot's overflow row


@pytest.fixture(scope="module")
def coffee():
    return M.HostScene("file:coffee", W, H)


@pytest.fixture
def packet_ctx(_packet_ctx):
    """tests/packet_helpers.py packet_ctx, no borrowed slots, and the builder's leaf size back at its default afterwards."""
    _packet_ctx.set_option("aux_depth", 0)
    yield _packet_ctx
    _packet_ctx.set_option("leaf_size", 4)


def _render(ctx, seeds, specialize, slim=1):
    """One frame of `seeds` by the lean build (`specialize` 1; `slim`: whether that must be the slim kernel) or the general one (0)."""
    frame, used = render_after_other_seeds(ctx, seeds, specialize=specialize)
    assert used == ((4, 0, slim) if specialize else (4, FEAT_ALL, 0)), used
    return frame


def _lean_equals_general(ctx, seeds, what, slim=1):
    lean, general = _render(ctx, seeds, 1, slim), _render(ctx, seeds, 0)
    assert lean.any() and np.isfinite(lean).all(), what
    diff = int((_bits(lean) != _bits(general)).any(axis=-1).sum())
    assert diff == 0, "%s: %d pixels differ between the lean and the general kernel" % (what, diff)
    return lean


@pytest.mark.parametrize("node_format", [64, 128])
def test_coffee_on_both_node_formats(packet_ctx, coffee, node_format):
    ctx = packet_ctx
    ctx.set_option("node_format", node_format)
    ctx.load(coffee)
    _lean_equals_general(ctx, M.launch_seeds(4), "coffee, %d-byte nodes" % node_format)
    assert ctx.get_option("node_format_used") == node_format


def test_a_tree_deeper_than_the_lds_stack(packet_ctx):
    """Box sizes in geometric progression: a deep tree, whose stack bound puts levels into the overflow rows under the slim kernel."""
    ctx = packet_ctx
    ctx.load(case_scene("geometric", 96, 54))
    assert 3 * ctx.accel_info().treeDepth + 1 > LDS_STACK_ENTRIES
    _lean_equals_general(ctx, M.launch_seeds(2), "geometric")


def test_duplicates_tie_at_equal_t(packet_ctx):
    """Every triangle several times over: candidates at exactly equal t, decided by the primitive id."""
    ctx = packet_ctx
    ctx.load(case_scene("duplicates", 96, 54))
    _lean_equals_general(ctx, M.launch_seeds(2), "duplicates")


@pytest.mark.parametrize("leaf_size", [1, 4, 8])
def test_leaf_sizes(packet_ctx, coffee, leaf_size):
    """Leaves of one, of up to four (one chunk of the leaf pass) and of up to eight triangles (two chunks): the slim kernel every time."""
    ctx = packet_ctx
    ctx.set_option("leaf_size", leaf_size)
    ctx.load(coffee)
    assert ctx.accel_info().maxLeafSize == leaf_size
    _lean_equals_general(ctx, M.launch_seeds(2), "leaf_size %d" % leaf_size)      # (_render asserts "kernel_slim_used" 1 of the slim frame)


def test_one_rank_of_two(packet_ctx, coffee):
    ctx = packet_ctx
    ctx.set_partition(1, 2)
    ctx.load(coffee)
    part = _lean_equals_general(ctx, M.launch_seeds(4), "rank 1 of 2")
    mine = part.any(axis=-1)
    assert mine.any() and not mine.all()


@pytest.mark.parametrize("drain_below", [0, 64])
def test_a_pool_down_to_its_last_paths(packet_ctx, coffee, drain_below):
    """64 slots per pool and one sample per pixel: the pools run out of work items; with "drain_below" 64 they hand their paths to the drain kernel."""
    ctx = packet_ctx
    ctx.set_option("slots_in_use", 64)
    ctx.set_option("drain_below", drain_below)
    ctx.load(coffee)
    _lean_equals_general(ctx, M.launch_seeds(1), "slots_in_use 64 drain_below %d" % drain_below)
