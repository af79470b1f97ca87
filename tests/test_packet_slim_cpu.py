"""The packet kernel's slim instantiations (csrc/packetkernel.hip: pt_packetkernel<false,true,false,NEAR,N64>, lean, without borrowed
slots and, for NEAR = false, without Disney GLASS) against their twins with both (pt_packetkernel_aux, the lean kernels of rounds 19-20
under a new name), as the shipped code objects describe them (tools/kernel_resources.py).  The slim build takes code away; it must not
cost a register, a spill or a byte of LDS more than the kernel it was cut from."""
import os
import sys

import pytest

from common import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))

PREFIX = "_ZN2pt12_GLOBAL__N_1"
TAIL = "EEvNS_10LaunchArgsE"
# (NEAR, N64) -> spilled scalar registers: the pins of tests/test_packet_features_cpu.py for the kernels of this name
LEAN_SGPR_SPILLS = {(0, 1): 30, (1, 1): 29, (0, 0): 21, (1, 0): 22}
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


def _sym(name, near, n64):
    return "%s%d%sILb0ELb1ELb0ELb%dELb%dE%s" % (PREFIX, len(name), name, near, n64, TAIL)


@pytest.fixture(scope="module")
def res():
    from kernel_resources import kernel_resources
    return kernel_resources(os.path.join(REPO, "minimaloptix_amd", "lib", "libmoptix.so"))


def test_the_four_twins_exist_under_their_new_name(res):
    twins = [k for k in res if "pt_packetkernel_auxI" in k]
    assert sorted(twins) == sorted(_sym("pt_packetkernel_aux", near, n64) for near in (0, 1) for n64 in (0, 1))
    assert not [k for k in twins if "pt_packetkernelI" in k]      # the new name is outside the pins that go by the old one


@pytest.mark.parametrize("near,n64", sorted(LEAN_SGPR_SPILLS))
def test_slim_kernel_needs_no_more_than_its_twin(res, near, n64):
    slim, twin = res[_sym("pt_packetkernel", near, n64)], res[_sym("pt_packetkernel_aux", near, n64)]
    print("NEAR=%d N64=%d slim %s | twin %s" % (near, n64, slim, twin))
    assert slim["vgpr_spill_count"] == 0 and slim["private_segment_fixed_size"] == 0, slim
    assert slim["sgpr_spill_count"] <= LEAN_SGPR_SPILLS[(near, n64)], slim
    for f in FIELDS:
        assert slim[f] <= twin[f], (f, slim, twin)
