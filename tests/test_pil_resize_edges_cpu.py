"""Pillow-exact resize at its edges, host side (no GPU, and no Pillow except the live sweep): the NumPy oracle against the Pillow-made
fixture tests/golden/g20_pil_resize_edges.npz on every named case and every sweep entry, the special float values, and the proof that
the fixture exercises Image.resize's two rules above the passes (no pass on an unchanged axis; vertical pass first for a tall source):
the oracle with either rule switched off fails exactly the cases of that rule."""
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
import pil_resize_oracle as R

TALL = ("tall", "tall_upx", "tall_edge_in")
NOT_TALL = ("tall_edge_out", "tall_no_down")
# col_src (300 x 1) is in the tall regime too, but a one-column source has the single coefficient 1.0 on x, so the order cannot show
IN_REGIME = TALL + ("col_src",)


@pytest.fixture(scope="module")
def golden():
    return load_golden("g20_pil_resize_edges.npz")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_but_nan(got, want):
    """NaN at the same places, every other element bit-equal (so -0.0 is not +0.0); a NaN's sign and payload are not compared."""
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(_bits(got)[~gn], _bits(want)[~wn])


def test_fixture_records_pillow_version_and_is_small(golden):
    assert re.match(r"\d+\.\d+", str(golden["pillow_version"]))
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "g20_pil_resize_edges.npz")) < 1000000
    assert golden["sweep_geometry"].tolist() == [list(src + dst) for _, src, dst in R.AXIS_SWEEP]
    assert golden["sweep_u8_sha"].shape == golden["sweep_f32_sha"].shape == (len(R.AXIS_SWEEP), 32)


def test_case_tables_are_the_stated_ones():
    assert len(R.FRAME_EDGE_CASES) == 19 and len(R.PLANE_EDGE_CASES) == 15 and len(R.PLANE_SPECIAL_CASES) == 5
    assert R.sweep_lengths(16) == [1, 2, 15, 16, 17, 31, 32, 49, 78, 115, 127, 128, 9]
    assert R.sweep_lengths(1) == [1, 2, 4, 3, 7, 8] and 90 <= len(R.AXIS_SWEEP) // 2 <= 110
    for name in R.FRAME_EDGE_CASES:
        _, src, dst, _ = R.FRAME_EDGE_CASES[name]
        assert R.vertical_first(src, dst) == (name in IN_REGIME), name
    assert sum(R.vertical_first(src, dst) for _, src, dst in R.AXIS_SWEEP) == 4          # I = 648, 913, 1039, 1040 -> 130
    assert not R.vertical_first((600, 6), (130, 5)) and R.vertical_first((601, 6), (600, 5)) and not R.vertical_first((601, 6), (601, 5))
    seeds = [c[-1] for t in (R.FRAME_CASES, R.FLOW_CASES, R.FRAME_EDGE_CASES, R.PLANE_EDGE_CASES, R.PLANE_SPECIAL_CASES) for c in t.values()]
    assert len(set(seeds)) == len(seeds)


# ------------------------------------------------------------------ oracle == fixture
@pytest.mark.parametrize("name", sorted(R.FRAME_EDGE_CASES))
def test_oracle_frames_equal_fixture(golden, name):
    n, src, dst, seed = R.FRAME_EDGE_CASES[name]
    frames = R.make_frames(n, src, seed)
    assert R.digest(frames) == str(golden["frame_%s_sha" % name]), "the case's input recipe changed"
    got = np.stack([R.resize_u8(f, dst) for f in frames])
    want = golden["frame_%s_u8" % name]
    assert got.shape == want.shape and np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())


@pytest.mark.parametrize("name", sorted(R.PLANE_EDGE_CASES))
def test_oracle_planes_equal_fixture(golden, name):
    n, c, src, dst, seed = R.PLANE_EDGE_CASES[name]
    x = R.make_planes(n, c, src, seed)
    assert x.shape == (n, c) + src and x.dtype == np.float32
    assert R.digest(x) == str(golden["plane_%s_sha" % name]), "the case's input recipe changed"
    got = R.resize_planes(x, dst)
    want = golden["plane_%s_f32" % name]
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), "%d elements differ" % int((_bits(got) != _bits(want)).sum())


@pytest.mark.parametrize("name", sorted(R.PLANE_SPECIAL_CASES))
def test_oracle_special_values_equal_fixture(golden, name):
    src, dst, seed = R.PLANE_SPECIAL_CASES[name]
    x = R.make_special(src, seed)
    assert R.digest(x) == str(golden["special_%s_sha" % name]), "the case's input recipe changed"
    assert np.isnan(x[0, 1, -1, -1]) and np.isnan(x).sum() == 1 and np.isinf(x).sum() == 2 and (x == np.float32(3e38)).sum() == 4
    assert np.signbit(x[0, 0, 5, 7]) and x[0, 0, 5, 7] == 0 and 0 < x[0, 1, 3, 12] < np.finfo(np.float32).tiny
    want = golden["special_%s_f32" % name]
    got = R.resize_planes(x, dst)
    assert _same_but_nan(got, want)
    if name == "identity":                                    # Pillow copies: one NaN, and the negative zero is still one
        assert np.isnan(want).sum() == 1 and np.array_equal(_bits(want)[~np.isnan(want)], _bits(x)[~np.isnan(x)])
    if name in R.UNCHANGED_AXIS_SPECIALS:
        assert not _same_but_nan(R.resize_planes(x, dst, skip_unchanged=False), want), "the case does not exercise the unchanged-axis rule"
    else:
        assert _same_but_nan(R.resize_planes(x, dst, skip_unchanged=False), want)


def test_oracle_sweep_digests_equal_fixture(golden):
    bad = []
    for i, (O, src, dst) in enumerate(R.AXIS_SWEEP):
        frame, plane = R.sweep_inputs(i)
        if not np.array_equal(R.digest_bytes(R.resize_u8(frame[0], dst)), golden["sweep_u8_sha"][i]):
            bad.append(("u8", src, dst))
        if not np.array_equal(R.digest_bytes(R.resize_f32(plane, dst)), golden["sweep_f32_sha"][i]):
            bad.append(("f32", src, dst))
    assert not bad, bad[:10]


# ------------------------------------------------------------------ the fixture exercises both rules
def test_horizontal_first_restatement_fails_the_tall_cases_only(golden):
    for name in TALL + NOT_TALL:
        n, src, dst, seed = R.FRAME_EDGE_CASES[name]
        got = np.stack([R.resize_u8(f, dst, tall_rule=False) for f in R.make_frames(n, src, seed)])
        assert np.array_equal(got, golden["frame_%s_u8" % name]) == (name in NOT_TALL), name
    for name in ("tall", "tall_edge_in", "tall_edge_out"):
        n, c, src, dst, seed = R.PLANE_EDGE_CASES[name]
        got = R.resize_planes(R.make_planes(n, c, src, seed), dst, tall_rule=False)
        assert np.array_equal(_bits(got), _bits(golden["plane_%s_f32" % name])) == (name == "tall_edge_out"), name
    # the sweep's four tall entries, and only they, depend on the rule
    for i, (O, src, dst) in enumerate(R.AXIS_SWEEP):
        if O == 130 and src[1] == 6:
            frame, plane = R.sweep_inputs(i)
            same = (np.array_equal(R.digest_bytes(R.resize_u8(frame[0], dst, tall_rule=False)), golden["sweep_u8_sha"][i])
                    and np.array_equal(R.digest_bytes(R.resize_f32(plane, dst, tall_rule=False)), golden["sweep_f32_sha"][i]))
            assert same == (not R.vertical_first(src, dst)), (src, dst)


def test_identity_pass_on_bytes_changes_nothing():
    """Why the frames kernel needs no unchanged-axis branch: the identity coefficient is exactly 2^22 and (2^21 + v * 2^22) >> 22 == v."""
    f = R.make_frames(1, (24, 40), 701)[0]
    for dst in ((24, 40), (24, 90), (50, 40)):
        assert np.array_equal(R.resize_u8(f, dst), R.resize_u8(f, dst, skip_unchanged=False))
    v = np.arange(256, dtype=np.int64)
    assert np.array_equal(((1 << 21) + v * (1 << 22)) >> 22, v)


# ------------------------------------------------------------------ oracle == live Pillow on the sweep
def test_oracle_equals_live_pillow_on_the_axis_sweep():
    Image = pytest.importorskip("PIL.Image")
    bad = []
    for i, (O, src, dst) in enumerate(R.AXIS_SWEEP):
        frame, plane = R.sweep_inputs(i)
        want = np.array(Image.fromarray(frame[0]).resize((dst[1], dst[0]), Image.BILINEAR))
        if not np.array_equal(R.resize_u8(frame[0], dst), want):
            bad.append(("u8", src, dst))
        wantf = np.array(Image.fromarray(plane).resize((dst[1], dst[0]), Image.BILINEAR))
        if not np.array_equal(_bits(R.resize_f32(plane, dst)), _bits(wantf)):
            bad.append(("f32", src, dst))
    assert not bad, bad[:10]
