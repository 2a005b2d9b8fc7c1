"""The four pure Winograd queries (pwc_conv3x3_wino4_preferred / _workspace_bytes, pwc_conv3x3_wino_preferred / _workspace_bytes)
over a box of layer geometries and six option settings, against the answers stored in tests/golden/wino_rule_census.json
(tests/wino_rule_census.py): the host code that plans a layer's launches may be rewritten, its answers may not move.  No device is
needed; without one the library counts 256 compute units, and the stored answers are those of 256."""
import pytest

import wino_rule_census as WC


@pytest.fixture(scope="module")
def census():
    return WC.census()


@pytest.fixture(scope="module")
def stored():
    return WC.load_fixture()


def test_box_is_the_stated_one():
    pts = WC.box()
    assert len(pts) == len(set(pts)) == 223055
    assert all(b * h * w <= WC.BOX_MAX_BHW for b, _, h, w, _ in pts)
    ws = {w for _, _, _, w, _ in pts}
    assert {30, 62, 126} <= ws and {4, 128, 160, 256, 320} <= ws
    assert [name for name, _ in WC.SETTINGS] == ["default", "w4_tailsplit=0", "w4_smallsplit=0", "w4_stacked=0", "w4_small_min_wgs=64",
                                                 "conv_wino4=0"]


def test_stored_census_can_tell_a_change(stored):
    """the conditions under which a pass means something, on the stored file alone: at the defaults every query answers both ways on
    at least 1 % of what it was asked (F(2x2): the (point, dilation) pairs), and every non-default setting moves the stream"""
    assert set(stored) == {name for name, _ in WC.SETTINGS}
    d = stored["default"]
    assert d["points"] == len(WC.box())
    for q in WC.QUERIES:
        asked = d["points"] * (len(WC.DILATIONS) if q.startswith("wino2") else 1)
        assert 0.01 * asked <= d[q] <= 0.99 * asked, (q, d[q], asked)
    hashes = {name: v["sha256"] for name, v in stored.items()}
    for name, h in hashes.items():
        assert name == "default" or h != hashes["default"], name


@pytest.mark.parametrize("setting", [name for name, _ in WC.SETTINGS])
def test_queries_answer_as_stored(census, stored, setting):
    assert census[setting] == stored[setting], (
        "the Winograd rule / scratch queries answer differently under %s (counts of yes / non-zero answers and the hash of the whole "
        "stream): now %s, stored %s -- a change of the host planning code, an option default, or a device with other than the 256 "
        "compute units the library counts when there is none; only after a deliberate rule change run python tests/wino_rule_census.py"
        % (setting, census[setting], stored[setting]))
