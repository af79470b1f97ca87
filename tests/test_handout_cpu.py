"""The lean packet kernel's hand-out on the host (csrc/megakernel.h handout_lean, magic_div; the check itself is tests/handout/handout_check.cpp).

handout_lean must map every hand-out index to the work item, sample, pixel, x, y and in-frame flag that handout_to_item ->
item_to_pixel -> begin_sample's `pixel % width, pixel / width` give, for "tile_major" 0-3, with and without an order list, one to eight
ranks; and the multiply-and-shift division it uses must agree with `/` and `%` for every non-negative int dividend.  The program includes
the header the kernels include, is compiled here with the host compiler and run once per group of cases."""
import os
import subprocess

import pytest

from common import REPO

SRC = os.path.join(REPO, "tests", "handout", "handout_check.cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("handout") / "handout_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + os.path.join(REPO, "minimaloptix_amd", "csrc"), "-o", exe, SRC], check=True)
    return exe


def _run(program, mode):
    r = subprocess.run([program, mode], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok " + mode), r.stdout
    return int(r.stdout.split()[-2])


def test_small_frames_every_index(program):
    """8x8 and 37x19, nSeeds in {1, 3, 16, 255, 256}, nRanks in {1, 2, 3, 8} as every rank, tile_major 0-3, with and without an order list: every k."""
    assert _run(program, "small") > 1000000


def test_full_hd_frame_ends_and_boundaries(program):
    """1920x1080, the same parameters: the first and last 4,096 indices and every multiple of the items of a tile and of a sample, +- 1."""
    assert _run(program, "large") > 1000000


def test_multiply_and_shift_division_is_exact(program):
    """d in {1, 2, 3, 5, 7, 64, 192, 240, 16320, 16384, 2^30 - 1, 2^31 - 1} and 1,000 seeded random divisors: n / d and n % d for n in
    {0, 1, d - 1, d, d + 1, 2^31 - 1} and at the multiples of d +- 1 (all of them up to 2^20 multiples, else 2^20 seeded random ones)."""
    assert _run(program, "magic") > 1000000
