"""The packet kernel's three builds (csrc/packetkernel.hip) as the shipped code objects describe them (tools/kernel_resources.py reads the
AMDGPU metadata embedded in libmoptix.so): the slim kernels pt_packetkernel<false,true,false,NEAR,N64> (lean -- without the FEAT_* programs
of csrc/pt_types.h -- without borrowed slots and, for NEAR = false, without Disney GLASS and with the ray switch in the scheduler loop),
their twins with borrowed slots and glass, pt_packetkernel_aux (the lean kernels of rounds 19-20), and the general kernels
pt_packetkernel_general<CNT,true,FAST,NEAR,N64>.  The point of the lean builds is the register allocation: no spilled vector register, no
scratch, half the spilled scalar registers; a slim kernel takes code away from its twin and must not cost a register, a spill or a byte
of LDS more than the kernel it was cut from, and every kernel stays within three workgroups of four waves per CU.  The pins are those of
rounds 6 and 19 (profiles/r19_kernel_resources.txt); an edit that moves them has to say so here and there."""
import os
import sys

import pytest

from common import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

PREFIX = "_ZN2pt12_GLOBAL__N_1"
TAIL = "EEvNS_10LaunchArgsE"
# (NEAR, N64) -> spilled scalar registers of the lean kernel as built in round 19
LEAN_SGPR_SPILLS = {(0, 1): 30, (1, 1): 29, (0, 0): 21, (1, 0): 22}
# (NEAR, N64) -> (spilled vector, spilled scalar) registers of the general kernel: the 64-byte-node ones are the pins of
# tests/test_capi_symbols.py from round 6, the 128-byte-node twins are what the library showed before the lean kernels came
GENERAL_SPILLS = {(0, 1): (4, 61), (1, 1): (3, 62), (0, 0): (3, 53), (1, 0): (3, 53)}
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")
VGPRS_AT_THREE_WAVES = 168
LDS_THIRD_OF_A_CU = 53760
NEAR_N64 = [(near, n64) for near in (0, 1) for n64 in (0, 1)]


def _sym(name, near, n64, cnt=0, fast=0):
    return "%s%d%sILb%dELb1ELb%dELb%dELb%dE%s" % (PREFIX, len(name), name, cnt, fast, near, n64, TAIL)


@pytest.fixture(scope="module")
def res():
    from kernel_resources import kernel_resources
    return kernel_resources(os.path.join(REPO, "minimaloptix_amd", "lib", "libmoptix.so"))


def test_there_are_four_slim_kernels_four_twins_and_sixteen_general_ones(res):
    slim = [k for k in res if "15pt_packetkernelI" in k]
    twins = [k for k in res if "pt_packetkernel_auxI" in k]
    general = [k for k in res if "23pt_packetkernel_generalI" in k]
    assert sorted(slim) == sorted(_sym("pt_packetkernel", near, n64) for near, n64 in NEAR_N64)
    assert sorted(twins) == sorted(_sym("pt_packetkernel_aux", near, n64) for near, n64 in NEAR_N64)
    assert not [k for k in twins if "pt_packetkernelI" in k]      # the twins' name is outside the pins that go by the slim kernels'
    assert len(general) == 16      # CNT x FAST x NEAR x N64
    for near, n64 in NEAR_N64:
        for cnt in (0, 1):
            for fast in (0, 1):
                assert _sym("pt_packetkernel_general", near, n64, cnt, fast) in res, (near, n64, cnt, fast)


@pytest.mark.parametrize("near,n64", sorted(LEAN_SGPR_SPILLS))
def test_slim_kernel_stays_within_its_twin_and_the_general_kernel(res, near, n64):
    slim = res[_sym("pt_packetkernel", near, n64)]
    twin, general = res[_sym("pt_packetkernel_aux", near, n64)], res[_sym("pt_packetkernel_general", near, n64)]
    print("NEAR=%d N64=%d slim %s | twin %s | general %s" % (near, n64, slim, twin, general))
    assert slim["vgpr_spill_count"] == 0 and slim["private_segment_fixed_size"] == 0, slim
    assert slim["sgpr_spill_count"] <= LEAN_SGPR_SPILLS[(near, n64)], slim
    assert slim["sgpr_spill_count"] < general["sgpr_spill_count"], (slim, general)
    for f in FIELDS:      # no field of the slim kernel exceeds its twin's or the general kernel's
        assert slim[f] <= twin[f], (f, slim, twin)
        assert slim[f] <= general[f], (f, slim, general)
    assert slim["vgpr_count"] <= VGPRS_AT_THREE_WAVES and slim["group_segment_fixed_size"] <= LDS_THIRD_OF_A_CU, slim


@pytest.mark.parametrize("near,n64", sorted(GENERAL_SPILLS))
def test_general_kernels_keep_their_allocation(res, near, n64):
    g = res[_sym("pt_packetkernel_general", near, n64)]
    v, s = GENERAL_SPILLS[(near, n64)]
    print("NEAR=%d N64=%d general %s" % (near, n64, g))
    assert g["vgpr_count"] <= VGPRS_AT_THREE_WAVES and g["group_segment_fixed_size"] <= LDS_THIRD_OF_A_CU, g
    assert g["vgpr_spill_count"] <= v and g["sgpr_spill_count"] <= s, g
