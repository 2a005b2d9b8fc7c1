"""The F(4x4) rule and workspace query for stacked tile groups (several short images per workgroup, pwc_conv_wino4.hip) -- host code only."""
import pytest

from opticalflow_amd import _lib


@pytest.fixture
def lib():
    lib = _lib.load()
    saved = _lib.get_option("w4_stacked")
    yield lib
    _lib.set_option("w4_stacked", saved)


def test_rule_takes_the_level4_lattice_launches(lib):
    p4 = lib.pwc_conv3x3_wino4_preferred
    for B in (2, 4, 16, 32):
        assert p4(64 * B, 128, 14, 32, 96, 1) == 1          # dc_conv4: 64 couts plain (16-row groups) + 32 couts, two 14x32 images per workgroup
        assert p4(256 * B, 96, 7, 16, 64, 1) == 1           # dc_conv5 on 7x16 images, four per workgroup
    # batch 1: 32 groups of two images x 4 Cin slices = 128 workgroups, under w4_small_min_wgs -> the plan keeps the 3-level context
    assert p4(64, 128, 14, 32, 96, 1) == 0
    # a ragged Cin chunk cannot be cut out of the middle of a group: level 6's dense layers (Cin 81 + ...) stay off
    assert p4(16, 81, 7, 16, 128, 1) == 0
    assert p4(32, 196, 7, 16, 196, 1) == 0                  # an odd 32-cout block on 7x16: no stacked 32-cout form of that width
    assert p4(1024, 128, 14, 32, 64, 1) == 1                # the plain narrow form is unchanged


def test_option_restores_the_round4_rule(lib):
    p4 = lib.pwc_conv3x3_wino4_preferred
    _lib.set_option("w4_stacked", 0)
    assert p4(1024, 128, 14, 32, 96, 1) == 0 and p4(4096, 96, 7, 16, 64, 1) == 0
    assert p4(1024, 128, 14, 32, 64, 1) == 1 and p4(16, 565, 112, 256, 128, 1) == 1


def test_workspace_counts_groups_of_images(lib):
    wsb = lib.pwc_conv3x3_wino4_workspace_bytes
    # 512 images of 7x16 = 128 groups of four = 128 workgroups -> two Cin slices; a slice's partial tile is 32 rows x 16 columns x 64 couts
    assert wsb(512, 96, 7, 16, 64) == 2 * 128 * 64 * 32 * 16 * 4
    assert wsb(4096, 96, 7, 16, 64) == 0                    # batch 16: 1024 workgroups, four whole rounds
    assert wsb(1024, 128, 14, 32, 96) == 0
