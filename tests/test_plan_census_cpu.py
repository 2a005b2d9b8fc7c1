"""The fp32 plan's routing decisions over a grid of small geometries, computed without a device (tests/plan_census.py), against what
the launch audit's configurations reach: a rule change that sends a layer to a route, a split or a plan shape that no audited
configuration has fails HERE, on the CPU, until a configuration covering it is added to test_gpu_launch_audit.CONFIGS.

The grid: B = 1..8, H = 64..384 and W = 64..640 in steps of 64 (every size script_pwc.py / inference_kitti.py pad to), with
B x H x W <= plan_census.GRID_MAX_BHW = 8 x 192 x 320 (364 of the box's 480 points; plan_census.py says why).  Default options; the
configurations with non-default options count towards the cover like the others."""
import time

import pytest

import plan_census as PC
from test_gpu_launch_audit import CONFIGS


@pytest.fixture(scope="module")
def config_census():
    """every configuration builds on the CPU device (a plan that raised here would raise on the device too)"""
    return PC.config_census(CONFIGS)


@pytest.fixture(scope="module")
def grid_census():
    t0 = time.time()
    out = {g: PC.signatures(*g) for g in PC.grid()}
    print("\nplan census: %d geometries in %.1f s" % (len(out), time.time() - t0))
    return out


def test_every_configuration_builds_and_matches_the_stored_census(config_census):
    assert len(config_census) == len(CONFIGS) and all(len(s) > 40 for s, _ in config_census.values())
    stored = PC.load_config_census()
    assert set(stored) == set(config_census), "tests/golden/plan_census_configs.json is stale: run python tests/plan_census.py"
    for cid, (sigs, shape) in config_census.items():
        assert stored[cid] == (sigs, shape), (
            "the census of %s changed (a routing rule, an option default, or a device with other than 256 compute units): only now %s, "
            "only stored %s, shape %s vs %s -- after a deliberate rule change run python tests/plan_census.py"
            % (cid, sorted(sigs - stored[cid][0]), sorted(stored[cid][0] - sigs), shape, stored[cid][1]))


def test_grid_is_the_stated_one():
    g = PC.grid()
    assert len(g) == 364 and len(set(g)) == 364
    assert (8, 192, 320) in g and (8, 320, 192) in g and (6, 256, 320) in g and (1, 384, 640) in g and (4, 384, 320) in g
    assert (7, 256, 320) not in g and (8, 384, 640) not in g
    assert all(h % 64 == 0 and w % 64 == 0 and 1 <= b <= 8 for b, h, w in g)


def _uncovered(grid_census, config_census):
    sigs = set().union(*[s for s, _ in config_census.values()])
    shapes = {sh for _, sh in config_census.values()}
    missing = {}
    for g, (s, sh) in sorted(grid_census.items(), key=lambda kv: kv[0][0] * kv[0][1] * kv[0][2]):
        for item in sorted(s - sigs) + ([("plan shape",) + sh] if sh not in shapes else []):
            missing.setdefault(item, g)                # the smallest geometry that shows it
    return missing


def test_every_signature_on_the_grid_is_audited(grid_census, config_census):
    missing = _uncovered(grid_census, config_census)
    assert not missing, "no launch-audit configuration reaches (signature: smallest geometry B, H, W): %s" % missing


def test_each_new_configuration_is_needed(grid_census, config_census):
    """the cover is minimal where it was extended: without any one of the small-geometry configurations a signature goes unaudited"""
    new = ("b8-192x320", "b8-384x64", "b6-192x192", "b8-320x192")
    assert set(new) <= set(config_census)
    for cid in new:
        rest = {k: v for k, v in config_census.items() if k != cid}
        assert _uncovered(grid_census, rest), cid
