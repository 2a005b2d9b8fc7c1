"""The fp32 direct 3x3 kernel's tile tables (csrc/pwc_conv_mfma.h, Tiles<stride, dilation>) against what the suite launches: a tile
is compiled if and only if it is in a table, and every entry must be launched by an audited plan (launch_audit.KERNELS_REQUIRED) or by a
parity case (launch_audit.TILE_CASES).  The tables are read from the host-only census tool, built here from the same header."""
import os
import re
import shutil
import subprocess

import pytest

import launch_audit as LA

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc is not installed")
    exe = str(tmp_path_factory.mktemp("census") / "conv_tile_census")
    subprocess.run([hipcc, "--cuda-host-only", "-O2", "-std=c++17", "-I" + os.path.join(REPO, "opticalflow_amd", "csrc"),
                    "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tools", "conv_tile_census.hip"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def table(census):
    return subprocess.run([census, "--list"], check=True, capture_output=True, text=True).stdout.splitlines()


def test_tables_are_what_plans_and_tile_cases_launch(table):
    assert len(table) == len(set(table)) == 93
    # unfolded, unsplit labels of the tile family: the folded tile (last argument 16) and the split-K form are launched past the tables
    plans = {k for k in LA.KERNELS_REQUIRED if k.startswith("conv3x3_mfma_kernel<") and k.endswith(", 0>")}
    cases = {c[7] for c in LA.TILE_CASES if c[7].startswith("conv3x3_mfma_kernel<")}
    assert len(cases) == 71 and not (plans & cases), sorted(plans & cases)
    assert set(table) == plans | cases, (sorted(set(table) - plans - cases), sorted((plans | cases) - set(table)))


def test_committed_census_is_of_these_tables(table):
    """profiles/conv_tile_census.txt lists exactly the tables' tiles, in their order, each picked somewhere in the box (the walk itself
    takes a minute and is not repeated here)"""
    with open(os.path.join(REPO, "profiles", "conv_tile_census.txt")) as f:
        rows = re.findall(r"^  <(\d+), (\d+), (\d+), (\d+), (\d+)> picks (\d+)$", f.read(), re.M)
    assert ["conv3x3_mfma_kernel<%s, %s, %s, %s, %s, 0>" % r[:5] for r in rows] == table
    assert all(int(r[5]) > 0 for r in rows)
