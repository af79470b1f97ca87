"""The slim packet kernels with the ray switch in the scheduler loop (csrc/packetkernel_body.h, SWITCH), as the shipped code objects describe
them (tools/kernel_resources.py).  The switch keeps a 16-byte row and a slot id per lane alive through the pass that follows; that must not
cost a slim kernel a vector spill, scratch, or a register, a spilled scalar or a byte of LDS more than its twin (pt_packetkernel_aux) has,
and the timed instantiation stays within three workgroups of four waves per CU.  The twins and the general kernels, which keep the switch
in the leaf pass, are still there under their names."""
import os
import sys

import pytest

from common import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

PREFIX = "_ZN2pt12_GLOBAL__N_1"
TAIL = "EEvNS_10LaunchArgsE"
# (NEAR, N64) -> spilled scalar registers: the pins of tests/test_packet_slim_cpu.py
LEAN_SGPR_SPILLS = {(0, 1): 30, (1, 1): 29, (0, 0): 21, (1, 0): 22}
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")
LDS_THIRD_OF_A_CU = 53760


def _sym(name, near, n64, cnt=0, fast=0):
    return "%s%d%sILb%dELb1ELb%dELb%dELb%dE%s" % (PREFIX, len(name), name, cnt, fast, near, n64, TAIL)


@pytest.fixture(scope="module")
def res():
    from kernel_resources import kernel_resources
    return kernel_resources(os.path.join(REPO, "minimaloptix_amd", "lib", "libmoptix.so"))


@pytest.mark.parametrize("near,n64", sorted(LEAN_SGPR_SPILLS))
def test_slim_kernel_stays_within_its_twin(res, near, n64):
    slim, twin = res[_sym("pt_packetkernel", near, n64)], res[_sym("pt_packetkernel_aux", near, n64)]
    print("NEAR=%d N64=%d slim %s | twin %s" % (near, n64, slim, twin))
    assert slim["vgpr_spill_count"] == 0 and slim["private_segment_fixed_size"] == 0, slim
    assert slim["sgpr_spill_count"] <= LEAN_SGPR_SPILLS[(near, n64)], slim
    for f in FIELDS:
        assert slim[f] <= twin[f], (f, slim, twin)
    assert slim["vgpr_count"] <= 168 and slim["group_segment_fixed_size"] <= LDS_THIRD_OF_A_CU, slim


def test_the_four_twins_and_the_general_kernels_still_exist(res):
    for near in (0, 1):
        for n64 in (0, 1):
            assert _sym("pt_packetkernel_aux", near, n64) in res
            for cnt in (0, 1):
                for fast in (0, 1):
                    assert _sym("pt_packetkernel_general", near, n64, cnt, fast) in res, (near, n64, cnt, fast)
    slim = [k for k in res if "pt_packetkernelI" in k]
    assert sorted(slim) == sorted(_sym("pt_packetkernel", near, n64) for near in (0, 1) for n64 in (0, 1))
