"""The packet kernel's lean instantiations (csrc/packetkernel.hip: pt_packetkernel<false,true,false,NEAR,N64>, compiled without the FEAT_*
programs of csrc/pt_types.h) against its general ones (pt_packetkernel_general), as the shipped code objects describe them
(tools/kernel_resources.py reads the AMDGPU metadata embedded in libmoptix.so).  The point of the lean build is the register
allocation: no spilled vector register, no scratch, half the spilled scalar registers.  The numbers are this round's
(profiles/r19_kernel_resources.txt); an edit that moves them has to say so here and there."""
import os
import sys

import pytest

from common import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

PREFIX = "_ZN2pt12_GLOBAL__N_1"
TAIL = "EEvNS_10LaunchArgsE"


def _sym(name, near, n64):
    return "%s%d%sILb0ELb1ELb0ELb%dELb%dE%s" % (PREFIX, len(name), name, near, n64, TAIL)


# (NEAR, N64) -> spilled scalar registers of the lean kernel as built in round 19
LEAN_SGPR_SPILLS = {(0, 1): 30, (1, 1): 29, (0, 0): 21, (1, 0): 22}
# (NEAR, N64) -> (spilled vector, spilled scalar) registers of the general kernel: the 64-byte-node ones are the pins of
# tests/test_capi_symbols.py from round 6, the 128-byte-node twins are what the library showed before the lean kernels came
GENERAL_SPILLS = {(0, 1): (4, 61), (1, 1): (3, 62), (0, 0): (3, 53), (1, 0): (3, 53)}
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


@pytest.fixture(scope="module")
def res():
    from kernel_resources import kernel_resources
    return kernel_resources(os.path.join(REPO, "minimaloptix_amd", "lib", "libmoptix.so"))


def test_there_are_four_lean_kernels_and_sixteen_general_ones(res):
    lean = [k for k in res if "15pt_packetkernelI" in k]
    general = [k for k in res if "23pt_packetkernel_generalI" in k]
    assert sorted(lean) == sorted(_sym("pt_packetkernel", near, n64) for near in (0, 1) for n64 in (0, 1))
    assert len(general) == 16      # CNT x FAST x NEAR x N64


@pytest.mark.parametrize("near,n64", sorted(LEAN_SGPR_SPILLS))
def test_lean_kernel_spills_no_vector_register_and_fewer_scalars_than_its_twin(res, near, n64):
    lean, twin = res[_sym("pt_packetkernel", near, n64)], res[_sym("pt_packetkernel_general", near, n64)]
    print("NEAR=%d N64=%d lean %s | general %s" % (near, n64, lean, twin))
    assert lean["vgpr_spill_count"] == 0 and lean["private_segment_fixed_size"] == 0, lean
    assert lean["sgpr_spill_count"] <= LEAN_SGPR_SPILLS[(near, n64)], lean
    assert lean["sgpr_spill_count"] < twin["sgpr_spill_count"], (lean, twin)
    for f in FIELDS:      # no field of the lean kernel exceeds its twin's
        assert lean[f] <= twin[f], (f, lean, twin)


@pytest.mark.parametrize("near,n64", sorted(GENERAL_SPILLS))
def test_general_kernels_keep_their_allocation(res, near, n64):
    g = res[_sym("pt_packetkernel_general", near, n64)]
    v, s = GENERAL_SPILLS[(near, n64)]
    print("NEAR=%d N64=%d general %s" % (near, n64, g))
    assert g["vgpr_count"] <= 168 and g["group_segment_fixed_size"] <= 53760, g
    assert g["vgpr_spill_count"] <= v and g["sgpr_spill_count"] <= s, g
