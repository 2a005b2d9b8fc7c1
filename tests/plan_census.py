"""Census of the fp32 plan's routing decisions, without a device (tests/test_plan_census_cpu.py, tests/test_gpu_launch_audit.py).

PwcPlan resolves every convolution's route while it is built (`planning`): the rules are host arithmetic of the library
(pwc_conv3x3_wino4_preferred, pwc_conv3x3_wino_preferred, the *_workspace_bytes queries that answer > 0 exactly when a launch is
cut along Cin) and of engine.py (_rule, _split96_wanted, the lattice context network, the head levels).  So the plan can be built on
torch.device("cpu") with the four filter-packing calls stubbed: no kernel is launched, no compute call is made, and the table
plan.routes is the same one a device plan of that geometry holds -- as long as the library counts the same number of compute units.
Without a device it falls back to 256, the MI355X's count; test_launch_audit compares the device plan with the census and says so
when they differ.

A signature is (layer, route, split workspace wanted, dilation); a plan's shape is (ctx_lattice, ctx_lattice4, dc4_split, levels on
the streaming head, levels on the 10-channel head).  This module is a helper, not a test module."""
from __future__ import annotations

import json
import os
from typing import Dict, FrozenSet, Optional, Tuple

import pytest
import torch

PACKERS = ("pack_conv3x3", "pack_conv3x3_wino", "pack_conv3x3_wino4", "pack_pyr1_wino")

_PARAMS: Dict[str, Dict[str, torch.Tensor]] = {}


def _params(variant: str) -> Dict[str, torch.Tensor]:
    """filter banks of the right shapes (the rules read shapes only)"""
    if variant not in _PARAMS:
        from opticalflow_amd import PWCDCNet, PWCDCNet_old
        net = (PWCDCNet if variant == "dc" else PWCDCNet_old)()
        _PARAMS[variant] = {k: torch.zeros(shape) for k, shape in net.manifest()}
    return _PARAMS[variant]


def _needs_workspace(route: str, n: int, cin: int, h: int, w: int, cout: int, stride: int, dilation: int) -> bool:
    """what PwcPlan._route adds to workspace_need for this launch, as a yes / no"""
    from opticalflow_amd import ops
    if route == "split96":
        return max(ops.conv3x3_wino4_workspace_bytes(n, cin, h, w, 64), ops.conv3x3_wino_workspace_bytes(n, cin, h, w, 32, 1)) > 0
    if route == "wino4":
        return ops.conv3x3_wino4_workspace_bytes(n, cin, h, w, cout) > 0
    if route == "wino2":
        return ops.conv3x3_wino_workspace_bytes(n, cin, h, w, cout, dilation) > 0
    if route == "direct":
        return ops.conv3x3_workspace_bytes(n, cin, h, w, cout, stride, dilation) > 0
    return False


def plan_signatures(plan) -> FrozenSet[Tuple[str, str, bool, int]]:
    """the (layer, route, split workspace, dilation) set of a built plan, on any device"""
    out = set()
    for (key, n, cin, h, w, cout, stride, dilation, _act, _res, _forced), route in plan.routes.items():
        layer = key[:-2] if key.endswith(".0") else key
        out.add((layer, route, _needs_workspace(route, n, cin, h, w, cout, stride, dilation), dilation))
    return frozenset(out)


def plan_shape(plan) -> Tuple[bool, bool, bool, Tuple[int, ...], Tuple[int, ...]]:
    return (bool(plan.ctx_lattice), bool(plan.ctx_lattice4), bool(plan.dc4_split),
            tuple(l for l in sorted(plan.stream_head) if plan.stream_head[l]), tuple(sorted(plan.head10)))


def signatures(B: int, H: int, W: int, variant: str = "dc", options: Optional[Dict[str, int]] = None):
    """(signature set, plan shape) of PwcPlan(B, H, W) built on the CPU device in planning mode under `options` (library options
    set for the build and restored afterwards)"""
    from opticalflow_amd import _lib, engine, ops
    saved = {k: _lib.get_option(k) for k in (options or {})}
    with pytest.MonkeyPatch.context() as mp:
        for name in PACKERS:
            mp.setattr(ops, name, lambda weight: torch.empty(0))
        try:
            for k, v in (options or {}).items():
                _lib.set_option(k, v)
            plan = engine.PwcPlan(_params(variant), B, H, W, torch.device("cpu"), variant=variant)
            return plan_signatures(plan), plan_shape(plan)
        finally:
            for k, v in saved.items():
                _lib.set_option(k, v)


# ---- the grid of tests/test_plan_census_cpu.py -----------------------------------------------------------------------------------
GRID_B = tuple(range(1, 9))
GRID_H = tuple(range(64, 384 + 1, 64))
GRID_W = tuple(range(64, 640 + 1, 64))
# B x H x W of a grid point stays at or under this cap (the full box would be 8 x 384 x 640 = 4x as much).  The walk itself is cheap
# (a plan per point: ~80 lazy buffer allocations and ~70 rule queries, a few seconds for the whole box); the cap is what the launch
# audit can follow: every signature under it is reached by a configuration whose float64 references cost no more than those of
# "opts-b2-256x512" (at most four images per launch and two end-to-end items are recomputed on the CPU).  Beyond it the same layers move
# on towards their large-map routes, which the 448x1024 configurations audit; DESIGN.md lists what the box holds beyond the cap
GRID_MAX_BHW = 8 * 192 * 320


def grid():
    return [(b, h, w) for b in GRID_B for h in GRID_H for w in GRID_W if b * h * w <= GRID_MAX_BHW]


# ---- the census of the launch audit's own configurations, stored (tests/golden/plan_census_configs.json) -----------------------------
# so that the GPU audit compares its device plans with what was computed WITHOUT a device; test_plan_census_cpu.py keeps the file equal
# to a fresh census.  Regenerate after a deliberate rule change:  python tests/plan_census.py
CONFIG_CENSUS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_census_configs.json")


def config_census(configs):
    return {cid: signatures(B, H, W, variant, opts) for cid, variant, B, H, W, opts, _why in configs}


def load_config_census():
    with open(CONFIG_CENSUS) as f:
        raw = json.load(f)
    return {cid: (frozenset((l, r, bool(s), int(d)) for l, r, s, d in v["signatures"]),
                  (bool(v["shape"][0]), bool(v["shape"][1]), bool(v["shape"][2]), tuple(v["shape"][3]), tuple(v["shape"][4])))
            for cid, v in raw.items()}


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from test_gpu_launch_audit import CONFIGS
    with open(CONFIG_CENSUS, "w") as f:
        json.dump({cid: {"signatures": sorted(map(list, s)), "shape": list(map(lambda v: list(v) if isinstance(v, tuple) else v, sh))}
                   for cid, (s, sh) in config_census(CONFIGS).items()}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", CONFIG_CENSUS)
