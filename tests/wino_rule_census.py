"""Census of the four pure Winograd queries over a box of layer geometries, without a device (tests/test_wino_rules_cpu.py).

pwc_conv3x3_wino4_preferred / _workspace_bytes (F(4x4)) and pwc_conv3x3_wino_preferred / _workspace_bytes (F(2x2), at dilations
1, 2, 4 and 8) are host arithmetic of the library: what PwcPlan._route, tests/plan_census.py and launch_audit.split_need rest on.  The
walk below asks all of them at every point of the box under each option setting and keeps, per setting, the number of points, how
often each query says yes / non-zero, and a SHA-256 over the packed stream of answers.  tests/golden/wino_rule_census.json stores
that for the library the fixture was made with; the test keeps a rewrite of the host code equal to it, answer for answer.

Without a device the library counts 256 compute units (the MI355X's count); the answers of a device with another count differ.
Regenerate only after a DELIBERATE rule change:  python tests/wino_rule_census.py.  This module is a helper, not a test module."""
from __future__ import annotations

import hashlib
import json
import os
import sys
from array import array
from typing import Dict, List, Tuple

BOX_B = (1, 2, 3, 4, 8, 16, 64, 256, 1024)
BOX_CIN = (16, 32, 81, 96, 128, 196, 565)
BOX_H = tuple(range(4, 64 + 1, 4)) + (7, 14, 112, 128)            # {4, 8, ..., 64} with 28 and 56 in it, and 7, 14, 112, 128
# 30, 62, 126: W % 4 != 0 (F(4x4) refuses, F(2x2) stores without 16-byte vectors)
BOX_W = tuple(range(4, 128 + 1, 4)) + (160, 256, 320) + (30, 62, 126)
BOX_COUT = (32, 64, 96, 128, 196)
BOX_MAX_BHW = 4 * 16 * 112 * 256
DILATIONS = (1, 2, 4, 8)

# (name, library options that differ from the defaults)
SETTINGS: Tuple[Tuple[str, Dict[str, int]], ...] = (
    ("default", {}),
    ("w4_tailsplit=0", {"w4_tailsplit": 0}),
    ("w4_smallsplit=0", {"w4_smallsplit": 0}),
    ("w4_stacked=0", {"w4_stacked": 0}),
    ("w4_small_min_wgs=64", {"w4_small_min_wgs": 64}),
    ("conv_wino4=0", {"conv_wino4": 0}),
)
# every option a setting touches must be at its default while another setting is walked
DEFAULTS = {"w4_tailsplit": 1, "w4_smallsplit": 1, "w4_stacked": 1, "w4_small_min_wgs": 160, "conv_wino4": 1}

QUERIES = ("wino4_preferred", "wino4_workspace", "wino2_preferred", "wino2_workspace")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino_rule_census.json")


def box() -> List[Tuple[int, int, int, int, int]]:
    return [(b, cin, h, w, cout) for b in BOX_B for cin in BOX_CIN for h in BOX_H for w in BOX_W for cout in BOX_COUT
            if b * h * w <= BOX_MAX_BHW]


def walk(points) -> Dict:
    """the answers of the four queries at every point under the options set now: counts (F(2x2): over the (point, dilation) pairs)
    and the hash of the stream [p4, ws4, p2(d) and ws2(d) for d in DILATIONS] per point, as little-endian int64"""
    from opticalflow_amd import _lib
    lib = _lib.load()
    p4, ws4, p2, ws2 = (lib.pwc_conv3x3_wino4_preferred, lib.pwc_conv3x3_wino4_workspace_bytes,
                        lib.pwc_conv3x3_wino_preferred, lib.pwc_conv3x3_wino_workspace_bytes)
    out = array("q")
    for b, cin, h, w, cout in points:
        out.append(p4(b, cin, h, w, cout, 1))
        out.append(ws4(b, cin, h, w, cout))
        for d in DILATIONS:
            out.append(p2(b, cin, h, w, cout, d))
            out.append(ws2(b, cin, h, w, cout, d))
    per = 2 + 2 * len(DILATIONS)
    assert out.itemsize == 8 and len(out) == per * len(points)
    if sys.byteorder == "big":
        out.byteswap()
    digest = hashlib.sha256(out.tobytes()).hexdigest()
    if sys.byteorder == "big":
        out.byteswap()
    res = {"points": len(points), "sha256": digest,
           "wino4_preferred": sum(1 for v in out[0::per] if v == 1),
           "wino4_workspace": sum(1 for v in out[1::per] if v > 0),
           "wino2_preferred": sum(1 for i in range(len(DILATIONS)) for v in out[2 + 2 * i::per] if v == 1),
           "wino2_workspace": sum(1 for i in range(len(DILATIONS)) for v in out[3 + 2 * i::per] if v > 0)}
    return res


def census() -> Dict[str, Dict]:
    """walk() under every setting; the library's options are restored afterwards"""
    from opticalflow_amd import _lib
    points = box()
    saved = {k: _lib.get_option(k) for k in DEFAULTS}
    try:
        out = {}
        for name, opts in SETTINGS:
            for k, v in {**DEFAULTS, **opts}.items():
                _lib.set_option(k, v)
            out[name] = walk(points)
        return out
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)


def load_fixture() -> Dict[str, Dict]:
    with open(FIXTURE) as f:
        return json.load(f)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    with open(FIXTURE, "w") as f:
        json.dump(census(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE)
