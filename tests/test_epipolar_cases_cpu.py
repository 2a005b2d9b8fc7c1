"""CPU checks of tests/epipolar_cases.py: the conditions on the cases that allow the GPU tests to ask `every count equal` of the
float64 oracle, the structural facts each case exists for, and a negative control per comparator -- each passes on the oracle's
own result and fails on a deliberately wrong NumPy variant of the step it guards."""
import numpy as np
import pytest

import epipolar_cases as EC
import epipolar_oracle as O

EPS = np.finfo(np.float64).eps
PREFIXES = (1, 63, 64, 65)


def _all_fits():
    for name in EC.RANSAC_CASES:
        yield name, EC.oracle_fit(name), EC.CASES[name].thresh
    yield "tie-rule", EC.tie_rule_fit()[0], EC.CASES[EC.TIE_CASE].thresh
    for b in (0, 1):
        yield "mixed-batch[%d]" % b, EC.oracle_fit_mixed(b), EC.MIXED.thresh


# ---------------------------------------------------------------- conditions on the cases
@pytest.mark.parametrize("name", EC.RANSAC_CASES + ("mixed-batch[0]", "mixed-batch[1]", "tie-rule"))
def test_cases_keep_clear_of_the_threshold_and_of_close_singular_values(name):
    """A Jacobi and a LAPACK singular vector differ by about eps sigma_1 / gap, at most 2e-11 for a gap of 1e-5; the distances
    inherit an error of that order, so a count can differ only for a distance within ~1e-10 of thresh: 1e-6 leaves four orders."""
    fit, thresh = {n: (f, t) for n, f, t in _all_fits()}[name]
    assert fit["hyps"].shape[0] == (EC.TIE_ITERS if name == "tie-rule" else (EC.MIXED if name.startswith("mixed") else EC.CASES[name]).iters)
    dmin, gmin = EC.hypothesis_margins(fit, thresh)
    print("%s: min |d - thresh| / thresh = %.2e, min (s7 - s8) / s1 = %.2e" % (name, dmin, gmin))
    assert dmin > EC.THRESH_MARGIN, (name, dmin)
    assert gmin >= EC.GAP_MARGIN, (name, gmin)
    assert EPS / gmin <= 2.3e-11


def test_tie_rule_table_keeps_the_first_of_four_equal_rows():
    fit, b0, later = EC.tie_rule_fit()
    assert fit["ok"] and fit["best"] == b0 and len(set(later)) == 3 and all(p > b0 for p in later)
    assert all(np.array_equal(fit["idx"][p], fit["idx"][b0]) and fit["counts"][p] == fit["counts"][b0] for p in later)
    assert later[0] // 64 == b0 // 64                     # another lane of the same wave (lanes = indices mod 256)
    assert (later[1] - b0) == 256                         # the same lane, one trip of its loop later
    assert later[2] >= EC.TIE_ITERS // 64 * 64 and EC.TIE_ITERS % 64 and later[2] // 64 % 4 != b0 // 64 % 4      # partial block, another wave


def test_shorter_runs_are_prefixes_with_the_same_margins():
    full = EC.oracle_fit("one-chunk-ragged")
    for k in PREFIXES:
        fit = EC.oracle_fit("one-chunk-ragged", k)
        assert np.array_equal(fit["counts"], full["counts"][:k]) and np.array_equal(fit["idx"], full["idx"][:k])


def test_eight_inliers_refit_is_well_conditioned():
    """The refit diagonalises the Gram matrix of the 8 x 9 inlier system: its 8th vector is accurate to about
    eps sigma_1^2 / (sigma_7^2 - sigma_8^2), which has to stay far inside the 1e-8 asked of F."""
    fit = EC.oracle_fit("eight-inliers")
    s, n = EC.refit_spectrum(fit, EC.CASES["eight-inliers"].thresh)
    assert n == 8 and s.shape == (8,)
    print("eight-inliers refit: s1/s8 = %.1f, (s7 - s8)/s1 = %.2e" % (s[0] / s[7], (s[6] - s[7]) / s[0]))
    assert (s[6] - s[7]) / s[0] >= EC.GAP_MARGIN
    assert s[0] / s[7] <= 1e3
    assert EPS * s[0] ** 2 / (s[6] ** 2 - s[7] ** 2) <= 1e-12


# ---------------------------------------------------------------- structural facts
def test_case_geometry_is_ragged_where_claimed():
    for name, c in EC.CASES.items():
        rows = EC.oracle_pairs(EC.case_flow(name), c.stride)
        assert (len(rows), EC.cap_of(c)) == EC.POINTS[name], name
        plane = c.H * c.W
        assert plane % 2048 and plane % 1024 and plane % 256, name       # loss chunk, select lanes, map / mask / backward groups
    c = EC.CASES["sub-wave"]
    assert c.W % c.stride and c.H % c.stride and c.H * c.W < 1024 and EC.POINTS["sub-wave"][0] < 64
    c = EC.CASES["one-chunk-ragged"]
    assert c.W % c.stride and c.H % c.stride and 64 < c.iters < 128 and c.iters % 64
    c = EC.CASES["holes-one-chunk"]
    N, cap = EC.POINTS["holes-one-chunk"]
    assert c.W % c.stride and c.H % c.stride and N < cap <= 1024 and c.iters % 64 and c.H * c.W > 3 * 2048
    c = EC.CASES["holes-multi-chunk"]
    N, cap = EC.POINTS["holes-multi-chunk"]
    assert c.W % c.stride and cap > 4 * 1024 and cap % 1024 and N < cap and N > 3 * 1024 and N % 1024
    # invalid lanes in every compaction chunk, so the carried base differs from the chunk start everywhere after the first
    fl = EC.case_flow("holes-multi-chunk")
    grid_valid = np.isfinite(fl[0][::c.stride, ::c.stride]).ravel()
    assert all((~grid_valid[c0:c0 + 1024]).any() for c0 in range(0, cap, 1024))


def test_one_chunk_ragged_has_a_tie_for_the_best_count():
    fit = EC.oracle_fit("one-chunk-ragged")
    top = np.flatnonzero(fit["counts"] == fit["counts"].max())
    assert len(top) >= 2 and fit["best"] == top[0] and fit["counts"].max() == 222


@pytest.mark.parametrize("seed", [1003, 1006, 1007, 1013])
def test_eight_inliers_best_count_is_eight(seed):
    c = EC.CASES["eight-inliers"]
    fl = (2 * np.random.default_rng(seed).standard_normal((2, c.H, c.W))).astype(np.float32)
    if seed == c.flow[1]:
        assert np.array_equal(fl, EC.case_flow("eight-inliers"))
    fit = EC.oracle_ransac(fl, c.stride, c.thresh, c.iters)
    assert fit["ok"] and fit["counts"].max() == 8
    assert EC.refit_spectrum(fit, c.thresh)[1] == 8


def test_mixed_batch_point_counts():
    flows, mask = EC.mixed_batch()
    N = [len(EC.oracle_pairs(flows[b], EC.MIXED.stride, mask[b])) for b in range(4)]
    assert N == [512, 420, 5, 0]
    assert EC.oracle_fit_mixed(0)["ok"] and EC.oracle_fit_mixed(1)["ok"]
    for b in (2, 3):
        fit = EC.oracle_fit_mixed(b)
        assert not fit["ok"] and fit["best"] == -1 and not fit["counts"].any() and fit["counts"].shape == (EC.MIXED.iters,)


def test_mask_variants_share_one_pattern():
    c = EC.CASES["holes-one-chunk"]
    var, keep = EC.mask_variants(c.H, c.W)
    assert set(var) == {"bool", "uint8", "float32", "float16", "int32"}
    for k, m in var.items():
        assert m.dtype == np.dtype(k) and np.array_equal(m != 0, keep), k
    assert {0.0, 0.25, -1.0} == set(np.unique(var["float32"])) == set(np.unique(var["float16"]).astype(np.float64))
    assert set(np.unique(var["uint8"])) == {0, 1, 255}
    rows = EC.oracle_pairs(EC.case_flow("holes-one-chunk"), c.stride, keep)
    assert 8 <= len(rows) < EC.POINTS["holes-one-chunk"][0]


# ---------------------------------------------------------------- comparators: pass on the oracle, fail on a wrong variant
def _compact(flow, stride, restart):
    """epi_pairs_kernel's chunked compaction in NumPy; restart=True is the defect: the write offset starts again at each chunk."""
    H, W = flow.shape[1:]
    ys, xs = np.mgrid[0:H:stride, 0:W:stride]
    x, y = xs.ravel().astype(np.float64), ys.ravel().astype(np.float64)
    x2, y2 = x + flow[0][ys, xs].ravel().astype(np.float64), y + flow[1][ys, xs].ravel().astype(np.float64)
    valid = np.isfinite(x2) & np.isfinite(y2)
    out, base = np.zeros((x.size, 4)), 0
    for c0 in range(0, x.size, 1024):
        v = np.flatnonzero(valid[c0:c0 + 1024]) + c0
        off = 0 if restart else base
        out[off:off + v.size] = np.column_stack([x[v], y[v], x2[v], y2[v]])
        base += v.size
    return out, base


def test_check_pairs_sees_an_offset_that_restarts_at_a_chunk():
    name = "holes-multi-chunk"
    fl, stride = EC.case_flow(name), EC.CASES[name].stride
    rows = EC.oracle_pairs(fl, stride)
    EC.check_pairs(*_compact(fl, stride, False), rows)
    with pytest.raises(AssertionError, match="rows differ"):
        EC.check_pairs(*_compact(fl, stride, True), rows)
    # within one chunk the defect is invisible: the reason the multi-chunk case exists
    fl1, s1 = EC.case_flow("holes-one-chunk"), EC.CASES["holes-one-chunk"].stride
    EC.check_pairs(*_compact(fl1, s1, True), EC.oracle_pairs(fl1, s1))
    with pytest.raises(AssertionError, match="N = "):
        EC.check_pairs(rows, len(rows) - 1, rows)


def _refit(fit, thresh, best, **kw):
    inl = O.sampson(fit["hyps"][best], fit["p1"], fit["p2"]) < thresh
    return O.eight_point(fit["p1"][inl], fit["p2"][inl], **kw)


def test_check_ransac_sees_the_last_of_tied_counts():
    name = "one-chunk-ragged"
    fit, thresh = EC.oracle_fit(name), EC.CASES[name].thresh
    assert EC.check_ransac(fit["F"], True, fit["best"], fit["counts"], fit) == 0.0
    last = len(fit["counts"]) - 1 - int(np.argmax(fit["counts"][::-1]))
    assert last != fit["best"]
    with pytest.raises(AssertionError, match="best = "):
        EC.check_ransac(_refit(fit, thresh, last), True, last, fit["counts"], fit)
    # (the two tied hypotheses may share their inlier set and so their refit: `best` is what has to be compared)
    wrong = fit["counts"].copy()
    wrong[5] += 1
    with pytest.raises(AssertionError, match="counts differ"):
        EC.check_ransac(fit["F"], True, fit["best"], wrong, fit)
    with pytest.raises(AssertionError):
        EC.check_ransac(np.full((3, 3), np.nan), True, fit["best"], fit["counts"], fit)


def test_check_ransac_sees_a_refit_that_always_takes_the_ninth_vector():
    name = "eight-inliers"
    fit, thresh = EC.oracle_fit(name), EC.CASES[name].thresh
    assert np.array_equal(_refit(fit, thresh, fit["best"]), fit["F"])
    EC.check_ransac(fit["F"], True, fit["best"], fit["counts"], fit)
    with pytest.raises(AssertionError, match="F_ref"):
        EC.check_ransac(_refit(fit, thresh, fit["best"], full_matrices=True), True, fit["best"], fit["counts"], fit)
    # with nine or more inliers both take the same vector: only the n = 8 case can tell
    fit9 = EC.oracle_fit("sub-wave")
    F9 = _refit(fit9, EC.CASES["sub-wave"].thresh, fit9["best"], full_matrices=True)
    EC.check_ransac(F9, True, fit9["best"], fit9["counts"], fit9)


def test_check_ransac_failed_fit():
    fit = EC.oracle_fit_mixed(2)
    EC.check_ransac(np.zeros(9), False, -1, np.zeros(EC.MIXED.iters, np.int32), fit)
    with pytest.raises(AssertionError):
        EC.check_ransac(np.zeros(9), False, 0, np.zeros(EC.MIXED.iters, np.int32), fit)
    with pytest.raises(AssertionError):
        EC.check_ransac(np.eye(3), False, -1, np.zeros(EC.MIXED.iters, np.int32), fit)


def _oracle_map(name):
    fit = EC.oracle_fit(name)
    return EC.oracle_distance(EC.case_flow(name), fit["F"])


def test_check_threshold_sees_the_wrong_lerp_branch():
    name = "one-chunk-ragged"
    F = EC.oracle_fit(name)["F"]
    told = 0
    for nf in (2, 5):
        d = EC.oracle_distance(EC.sparse_flow(name, nf), F)
        fin = d[np.isfinite(d)]
        assert fin.size == nf
        for q in EC.SPARSE_RATIOS:
            for tau, kr, mk in ((1e300, q, 0.0), (1e300, 1e-9, q)):       # as keep_ratio, and as the relaxation's min_keep
                thr, keep = EC.numpy_threshold(d, tau, kr, mk)
                assert thr == float(np.quantile(fin, q))
                EC.check_threshold(thr, keep, d, tau, kr, mk)
                thr2, keep2 = EC.numpy_threshold(d, tau, kr, mk, quantile=EC.quantile_low_branch)
                g = (nf - 1) * q - np.floor((nf - 1) * q)
                if thr2 != thr:
                    assert g >= 0.5
                    told += 1
                    with pytest.raises(AssertionError, match="numpy gives"):
                        EC.check_threshold(thr2, keep2, d, tau, kr, mk)
    assert told >= 4, "these maps have to tell _lerp's two expressions apart"
    # between neighbours of a dense map the two expressions round alike: the full-size cases cannot tell them apart
    dd = _oracle_map(name)
    q = EC.ratio_with_fraction(dd.size, 0.5, 0.95, 0.2)
    assert EC.quantile_low_branch(dd.ravel(), q) == np.quantile(dd, q)


def test_check_threshold_sees_less_than_for_less_or_equal():
    d = _oracle_map("one-chunk-ragged")
    q = EC.integral_ratio(d.size)
    thr, keep = EC.numpy_threshold(d, 1e300, q, 0.05)
    assert (d == thr).sum() >= 1                      # an integral virtual index: thr is one of the distances
    EC.check_threshold(thr, keep, d, 1e300, q, 0.05)
    with pytest.raises(AssertionError, match="pixels differ"):
        EC.check_threshold(thr, np.isfinite(d) & (d < thr), d, 1e300, q, 0.05)
    # no finite distance: NaN and all true
    nan = np.full((3, 5), np.nan)
    EC.check_threshold(float("nan"), np.ones((3, 5), bool), nan, 1.0, 0.2, 0.05)
    with pytest.raises(AssertionError):
        EC.check_threshold(1.0, np.ones((3, 5), bool), nan, 1.0, 0.2, 0.05)


def test_select_settings_reach_every_branch():
    for name in ("sub-wave", "holes-multi-chunk"):
        d = _oracle_map(name)
        fin = d[np.isfinite(d)]
        n1 = fin.size - 1
        st = {t: (tau, kr, mk) for t, tau, kr, mk in EC.select_settings(d)}
        frac = lambda q: n1 * q - np.floor(n1 * q)      # noqa: E731
        assert 0 < frac(st["frac<0.5"][1]) < 0.5 <= frac(st["frac>=0.5"][1]) and frac(st["integral"][1]) == 0
        assert 0 < frac(st["relax-frac<0.5"][2]) < 0.5 <= frac(st["relax-frac>=0.5"][2]) and frac(st["relax-integral"][2]) == 0
        share = lambda t: (np.isfinite(d) & (d <= t)).mean()      # noqa: E731

        def first_thr(tau, kr):
            return min(tau, np.quantile(fin, kr)) if 0 < kr < 1 else tau
        for tag, (tau, kr, mk) in st.items():
            relaxes = 0 < mk < 1 and share(first_thr(tau, kr)) < mk
            assert relaxes == tag.startswith("relax"), (name, tag)
        tau, kr, mk = st["relax-tightens"]
        assert EC.numpy_threshold(d, tau, kr, mk)[0] <= tau
        assert st["tau-below-quantile"][0] < np.quantile(fin, st["tau-below-quantile"][1])
        assert not any(0 < st[t][1] < 1 for t in ("keep-off-high", "keep-off-low", "keep-off-one", "both-off"))
        assert not any(0 < st[t][2] < 1 for t in ("min-off-high", "min-off-low", "both-off"))


def test_check_distance_bound_and_finite_pattern():
    d = _oracle_map("holes-one-chunk")
    assert EC.check_distance(d, d) == 0.0
    scale = np.sqrt(d[np.isfinite(d)]).max()
    off = d.copy()
    i = np.unravel_index(np.nanargmax(d), d.shape)
    off[i] = (np.sqrt(d[i]) + 3e-9 * scale) ** 2
    with pytest.raises(AssertionError, match="sqrt-form"):
        EC.check_distance(off, d)
    pat = d.copy()
    pat[np.unravel_index(np.flatnonzero(~np.isfinite(d))[0], d.shape)] = 0.0
    with pytest.raises(AssertionError, match="finite pattern"):
        EC.check_distance(pat, d)


def test_check_loss_sees_a_count_that_includes_pixels_past_the_plane():
    name = "one-chunk-ragged"
    fl = EC.case_flow(name)[None]
    F32 = EC.oracle_fit(name)["F"].astype(np.float32)
    sel = np.random.default_rng(3).random((1,) + fl.shape[2:]) < 0.6
    loss, grad = O.soft_loss(fl, F32, sel.astype(np.float64), "huber", 1e-3, 0.1)
    EC.check_loss(loss, grad.astype(np.float32), loss, grad, sel)
    # the defect: the last 2048-pixel chunk counted whole (87 phantom pixels past the 1961 of the plane)
    cnt, plane = int(sel.sum()), fl.shape[2] * fl.shape[3]
    cnt_bad = cnt + (-plane) % 2048
    assert cnt_bad == cnt + 87
    with pytest.raises(AssertionError, match="loss"):
        EC.check_loss(loss * cnt / cnt_bad, grad * cnt / cnt_bad, loss, grad, sel)
    with pytest.raises(AssertionError, match="gradient error"):
        EC.check_loss(loss, grad * cnt / cnt_bad, loss, grad, sel)
    # a gradient at an unselected pixel, however small, and a write behind the buffer
    leak = grad.copy()
    leak[0, 1][np.unravel_index(np.flatnonzero(~sel[0])[0], sel.shape[1:])] = 1e-30
    with pytest.raises(AssertionError, match="unselected"):
        EC.check_loss(loss, leak, loss, grad, sel)
    EC.check_loss(loss, grad, loss, grad, sel, guard=np.full(8, 777.0), sentinel=777.0)
    with pytest.raises(AssertionError, match="past the plane"):
        EC.check_loss(loss, grad, loss, grad, sel, guard=np.array([777.0, 0.0]), sentinel=777.0)
    # nothing selected: exactly 0
    EC.check_loss(0.0, np.zeros_like(grad), 0.0, np.zeros_like(grad))
    with pytest.raises(AssertionError):
        EC.check_loss(1e-30, np.zeros_like(grad), 0.0, np.zeros_like(grad))


def test_oracle_table_argument_and_out_of_range_rule():
    name = "sub-wave"
    fit = EC.oracle_fit(name)
    c = EC.CASES[name]
    same = EC.oracle_ransac(EC.case_flow(name), c.stride, c.thresh, None, idx=fit["idx"])
    assert np.array_equal(same["counts"], fit["counts"]) and same["best"] == fit["best"] and np.array_equal(same["F"], fit["F"])
    idx = fit["idx"].copy()
    idx[3, 5] = len(fit["p1"])
    bad = EC.oracle_ransac(EC.case_flow(name), c.stride, c.thresh, None, idx=idx)
    assert bad["counts"][3] == 0 and np.isnan(bad["hyps"][3]).all()
    keep = np.arange(c.iters) != 3
    assert np.array_equal(bad["counts"][keep], fit["counts"][keep])
    # the sampler's table is prefix-stable: a shorter run is a prefix of a longer one
    short = EC.oracle_fit(name, 17)
    assert np.array_equal(short["idx"], fit["idx"][:17]) and np.array_equal(short["counts"], fit["counts"][:17])
