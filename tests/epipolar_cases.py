"""Ragged cases of the epipolar operator (csrc/pwc_epipolar.hip) and the comparators its GPU tests use.  A helper, not a test
module: tests/test_epipolar_cases_cpu.py pins the conditions that make the float64 oracle safe to compare with exactly and shows
that every comparator can fail; tests/test_gpu_epipolar_edges.py runs the kernels on the cases.

The g9 fixture has two geometries, 96 x 128 at stride 4 and 384 x 512 at stride 6, whose pixel counts are multiples of 256, 1024
and 2048, whose H and W are multiples of the stride and whose only multi-chunk sample drops no point.  The cases here are built
from epipolar_oracle.rigid_flow and NumPy generators only, at sizes where every one of those coincidences fails:

  sub-wave           23 x 41, stride 5 (W % stride != 0): 45 points, 943 pixels -- fewer than one loss chunk (2048), than the
                     select kernel's 1024 lanes, and 3 map workgroups + 175
  one-chunk-ragged   37 x 53, stride 3: 234 points, 1961 pixels; 70 iterations = one score block of 64 hypotheses + 6; the two
                     largest counts tie (222), so the first-index rule decides `best`
  holes-one-chunk    61 x 127, stride 4: cap 512, 15 % of flow[0] NaN -> N = 420 (compaction with invalid lanes, one chunk);
                     7747 pixels = 3 loss chunks + 1603 = 30 map workgroups + 67; 130 iterations = two score blocks + 2
  holes-multi-chunk  100 x 183, stride 2: cap 4600 = 4 compaction chunks + 504, N = 3925 < cap (base carried across chunks next to
                     invalid lanes), 3 score chunks + 853
  eight-inliers      17 x 23, stride 4: 30 points of pure noise, thresh 0.05: the best count is exactly 8, so the refit takes
                     the k = n = 8th row of the Gram matrix and not the 9th
  mixed-batch        four 61 x 127 samples in one call: clean (N = 512), holed (N = 420), image mask leaving 5 points, all NaN
  mask-dtypes        the holed sample with one image-mask pattern as bool / uint8 / float32 / float16 / int32
"""
import functools
from collections import namedtuple

import numpy as np

import epipolar_oracle as O

Case = namedtuple("Case", "H W stride iters thresh flow holes")
# flow: ("rigid", seed) = O.rigid_flow(H, W, seed); ("normal", seed) = float32(2 * default_rng(seed).standard_normal((2, H, W)))
# holes: None or (seed, share): flow[0] = NaN where default_rng(seed).random((H, W)) < share
CASES = {
    "sub-wave": Case(23, 41, 5, 64, 0.5, ("rigid", 123), None),
    "one-chunk-ragged": Case(37, 53, 3, 70, 0.5, ("rigid", 137), None),
    "holes-one-chunk": Case(61, 127, 4, 130, 0.5, ("rigid", 161), (0, 0.15)),
    "holes-multi-chunk": Case(100, 183, 2, 130, 0.5, ("rigid", 200), (17, 0.15)),
    "eight-inliers": Case(17, 23, 4, 70, 0.05, ("normal", 1003), None),
}
RANSAC_CASES = tuple(CASES)
SAMPLER_SEED = 0
# expected (N, cap): pinned by test_epipolar_cases_cpu.py
POINTS = {"sub-wave": (45, 45), "one-chunk-ragged": (234, 234), "holes-one-chunk": (420, 512),
          "holes-multi-chunk": (3925, 4600), "eight-inliers": (30, 30)}

MIXED = Case(61, 127, 4, 130, 0.5, None, None)
MIXED_CLEAN_SEED, MIXED_FEW_SEED = 162, 163

F_TOL = 1e-8          # ||F - F_ref|| / ||F_ref||: test_ransac_matches_reference_g9
LOSS_TOL = 1e-6       # loss and gradient, relative: test_soft_loss_matches_oracle
DIST_TOL = 1e-9       # |sqrt d - sqrt d_ref| <= DIST_TOL max sqrt d_ref: test_sampson_distance_matches_oracle
MASK_SHARE = 1e-4     # share of pixels that may differ from the oracle's mask, each within MASK_AT_THR of the threshold
MASK_AT_THR = 1e-6
THRESH_MARGIN = 1e-6  # no oracle distance within this (relative) of the RANSAC threshold ...
GAP_MARGIN = 1e-5     # ... and (sigma_7 - sigma_8) / sigma_1 of every hypothesis' 8 x 9 system at least this


def cap_of(c):
    return -(-c.H // c.stride) * -(-c.W // c.stride)


def _base_flow(c):
    kind, seed = c.flow
    if kind == "rigid":
        return O.rigid_flow(c.H, c.W, seed)
    return (2 * np.random.default_rng(seed).standard_normal((2, c.H, c.W))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case_flow(name):
    c = CASES[name]
    fl = _base_flow(c)
    if c.holes is not None:
        seed, share = c.holes
        fl[0][np.random.default_rng(seed).random((c.H, c.W)) < share] = np.nan
    fl.setflags(write=False)
    return fl


def case_flow(name):
    """[2,H,W] float32 of a single-sample case (a fresh copy)."""
    return _case_flow(name).copy()


def hw2(flow_2hw):
    return np.ascontiguousarray(np.asarray(flow_2hw).transpose(1, 2, 0))


def mixed_batch():
    """(flows [4,2,H,W] float32, image mask [4,H,W] bool): clean, holed, five grid points left by the mask, all NaN."""
    c = MIXED
    few = np.zeros((c.H, c.W), bool)
    few[2 * c.stride, 3 * c.stride:8 * c.stride:c.stride] = True          # five grid points of one grid row
    few[1::c.stride, :] = True                                           # off-grid rows: must not count
    flows = np.stack([O.rigid_flow(c.H, c.W, MIXED_CLEAN_SEED), case_flow("holes-one-chunk"),
                      O.rigid_flow(c.H, c.W, MIXED_FEW_SEED), np.full((2, c.H, c.W), np.nan, np.float32)])
    mask = np.stack([np.ones((c.H, c.W), bool), np.ones((c.H, c.W), bool), few, np.ones((c.H, c.W), bool)])
    return flows, mask


def mask_variants(H, W, seed=7):
    """One image-mask pattern in every dtype the "nonzero" rule of _args._mask_arg takes: {name: array [H,W]} and the bool
    pattern.  A third of the pixels are dropped (0); the kept ones hold two different non-zero values per dtype."""
    code = np.random.default_rng(seed).integers(0, 3, (H, W))
    val = {"bool": (False, True, True), "uint8": (0, 1, 255), "float32": (0.0, 0.25, -1.0), "float16": (0.0, 0.25, -1.0),
           "int32": (0, 1, -7)}
    out = {k: np.asarray(v, dtype=k)[code] for k, v in val.items()}
    return out, code != 0


def oracle_pairs(flow_2hw, stride, mask_hw=None):
    """[N,4] float64 rows (x, y, x + fu, y + fv) in grid order: what epi_pairs_kernel writes."""
    p1, p2 = O.flow_to_pairs(hw2(flow_2hw), stride, mask_hw)
    return np.column_stack([p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]])


def oracle_distance(flow_2hw, Fm):
    """O.distance_map [H,W]; non-finite flow gives non-finite distances there, quietly."""
    with np.errstate(invalid="ignore", over="ignore"):
        return O.distance_map(hw2(flow_2hw), np.asarray(Fm, np.float64).reshape(3, 3))


def pairs_to_points(rows):
    one = np.ones(len(rows))
    return np.column_stack([rows[:, 0], rows[:, 1], one]), np.column_stack([rows[:, 2], rows[:, 3], one])


def oracle_ransac(flow_2hw, stride, thresh, iters, mask_hw=None, idx=None):
    p1, p2 = O.flow_to_pairs(hw2(flow_2hw), stride, mask_hw)
    fit = O.ransac(p1, p2, iters, thresh, SAMPLER_SEED, idx)
    fit["p1"], fit["p2"] = p1, p2
    return fit


@functools.lru_cache(maxsize=None)
def oracle_fit(name, iters=None):
    """The oracle's RANSAC result of a single-sample case (cached: computed once per process, never modified)."""
    c = CASES[name]
    return oracle_ransac(_case_flow(name), c.stride, c.thresh, c.iters if iters is None else iters)


@functools.lru_cache(maxsize=None)
def oracle_fit_mixed(b):
    flows, mask = mixed_batch()
    return oracle_ransac(flows[b], MIXED.stride, MIXED.thresh, MIXED.iters, mask[b])


TIE_CASE, TIE_ITERS = "holes-one-chunk", 458          # seven blocks of 64 hypotheses + 10


@functools.lru_cache(maxsize=None)
def tie_rule_fit():
    """(oracle fit on a doctored table, b0, later): the sampler's 458-row table of TIE_CASE with the winner's row b0 copied to
    three later rows -- another lane of b0's wave in the refit kernel's argmax, the same lane one stride of 256 later, and the
    last, partial block of 64 hypotheses."""
    c = CASES[TIE_CASE]
    table = O.index_table(POINTS[TIE_CASE][0], SAMPLER_SEED, TIE_ITERS)
    b0 = oracle_ransac(_case_flow(TIE_CASE), c.stride, c.thresh, None, idx=table)["best"]
    full = TIE_ITERS // 64 * 64
    later = (b0 + 7, b0 + 256, full + (b0 + 3) % (TIE_ITERS - full))
    assert b0 % 64 < 57 and later[1] < full, b0
    table = table.copy()
    for p in later:
        table[p] = table[b0]
    table.setflags(write=False)
    return oracle_ransac(_case_flow(TIE_CASE), c.stride, c.thresh, None, idx=table), b0, later


def hypothesis_margins(fit, thresh):
    """(smallest |d - thresh| / thresh over every hypothesis and point, smallest (sigma_7 - sigma_8) / sigma_1 over every
    hypothesis' 8 x 9 system) of an oracle fit: the two input conditions under which `every count equal` may be asked."""
    p1, p2 = fit["p1"], fit["p2"]
    dmin, gmin = np.inf, np.inf
    for i, Fc in enumerate(fit["hyps"]):
        if not np.isfinite(Fc).all():
            continue
        d = O.sampson(Fc, p1, p2)
        dmin = min(dmin, float(np.abs(d - thresh).min()) / thresh)
        s = np.linalg.svd(O.design_matrix(p1[fit["idx"][i]], p2[fit["idx"][i]])[0], compute_uv=False)
        gmin = min(gmin, float((s[6] - s[7]) / s[0]))
    return dmin, gmin


def refit_spectrum(fit, thresh):
    """Singular values of the winner's inlier system (n x 9), the matrix whose Gram matrix the refit diagonalises."""
    p1, p2 = fit["p1"], fit["p2"]
    inl = O.sampson(fit["hyps"][fit["best"]], p1, p2) < thresh
    return np.linalg.svd(O.design_matrix(p1[inl], p2[inl])[0], compute_uv=False), int(inl.sum())


# ---------------------------------------------------------------- comparators (pure NumPy, on downloaded arrays)
def check_pairs(pts, n, oracle_rows):
    """The first n rows of pts [cap,4] are the oracle's (x, y, x2, y2), exactly and in order.  Exact is right: every value is an
    integer or float64(x) + float64(float32), one rounding that both sides do alike."""
    n = int(n)
    assert n == len(oracle_rows), "N = %d, the oracle keeps %d" % (n, len(oracle_rows))
    pts = np.asarray(pts)
    assert pts.dtype == np.float64 and pts.shape[0] >= n and pts.shape[1] == 4
    bad = np.flatnonzero((pts[:n] != oracle_rows).any(axis=1))
    assert bad.size == 0, "%d of %d rows differ, first at %d: %s != %s" % (bad.size, n, bad[0], pts[bad[0]], oracle_rows[bad[0]])


def check_ransac(F, ok, best, counts, fit):
    """ok, best and every count equal the oracle's (best -1 and all-zero counts for N < 8); F within F_TOL (Frobenius, relative)
    of the oracle's refit, and exactly 0 where the fit fails.  Returns the relative error of F (0.0 for a failed fit)."""
    counts = np.asarray(counts).astype(np.int64)
    assert bool(ok) == bool(fit["ok"]), "ok = %s, the oracle says %s" % (bool(ok), fit["ok"])
    assert counts.shape == fit["counts"].shape
    bad = np.flatnonzero(counts != fit["counts"])
    assert bad.size == 0, "%d counts differ, first at %d: %d != %d" % (bad.size, bad[0], counts[bad[0]], fit["counts"][bad[0]])
    assert int(best) == int(fit["best"]), "best = %d, the oracle's first strictly largest count is at %d" % (int(best), fit["best"])
    F = np.asarray(F, np.float64).reshape(3, 3)
    if not fit["ok"]:
        assert not F.any(), "F of a failed fit is not 0"
        return 0.0
    rel = float(np.linalg.norm(F - fit["F"]) / np.linalg.norm(fit["F"]))
    assert rel <= F_TOL, "||F - F_ref|| / ||F_ref|| = %.3e > %.0e" % (rel, F_TOL)     # also fails on NaN
    return rel


def numpy_threshold(dist, tau, keep_ratio, min_keep, quantile=np.quantile):
    """build_epipolar_mask_from_flow's threshold from a distance map, as written there (train_fundamental.py:298-327):
    (thr, or None when no distance is finite, and the keep mask)."""
    dist = np.asarray(dist)
    fin = np.isfinite(dist)
    if not fin.any():
        return None, np.ones(dist.shape, bool)
    thr = float(tau)
    if 0 < keep_ratio < 1:
        thr = min(thr, float(quantile(dist[fin], keep_ratio)))
    if 0 < min_keep < 1 and (fin & (dist <= thr)).mean() < min_keep:
        thr = min(float(tau), float(quantile(dist[fin], min_keep)))
    return thr, fin & (dist <= thr)


def check_threshold(thr, mask, dist, tau, keep_ratio, min_keep):
    """thr is numpy's quantile logic on the kernel's OWN distances, bit for bit (NaN and an all-true mask when none is finite),
    and the mask is finite & (d <= thr).  Returns the expected threshold."""
    want, keep = numpy_threshold(dist, tau, keep_ratio, min_keep)
    thr = float(thr)
    mask = np.asarray(mask).astype(bool).reshape(np.asarray(dist).shape)
    if want is None:
        assert np.isnan(thr) and mask.all(), "no finite distance: thr %r, %d pixels dropped" % (thr, int((~mask).sum()))
        return want
    assert thr == want, "thr = %r, numpy gives %r (difference %.3e)" % (thr, want, thr - want)
    bad = int((mask != keep).sum())
    assert bad == 0, "%d pixels differ from finite & (d <= thr)" % bad
    return want


def check_mask_against_oracle(mask, thr, flow_2hw, F_ref, tau, keep_ratio, min_keep):
    """The two conditions of test_mask_matches_reference_g9 against the oracle's own distances: at most MASK_SHARE of the pixels
    differ, each with an oracle distance within MASK_AT_THR (relative) of the oracle's threshold.  Returns the count."""
    dref = oracle_distance(flow_2hw, F_ref)
    mref, tref = O.threshold_mask(dref, tau, keep_ratio, min_keep)
    mask = np.asarray(mask).astype(bool).reshape(mref.shape)
    bad = mask != mref
    if tref is None:
        assert np.isnan(float(thr)) and not bad.any()
        return 0
    assert bad.sum() <= MASK_SHARE * bad.size, "%d of %d pixels differ from the oracle's mask" % (int(bad.sum()), bad.size)
    assert np.all(np.abs(dref[bad] - tref) <= MASK_AT_THR * tref), "a differing pixel is not at the threshold"
    assert abs(float(thr) - tref) <= 1e-6 * abs(tref), "thr = %r, oracle %r" % (float(thr), tref)
    return int(bad.sum())


def check_distance(d, dref):
    """Same finite pattern; |sqrt d - sqrt d_ref| <= DIST_TOL max sqrt d_ref on the finite ones (x2^T F x1 cancels, so the bound
    follows sqrt d, the quantity that rounds in fp64).  Returns the worst error as a share of the bound's scale."""
    d, dref = np.asarray(d), np.asarray(dref)
    assert d.shape == dref.shape and d.dtype == np.float64
    f = np.isfinite(dref)
    assert np.array_equal(np.isfinite(d), f), "finite pattern differs at %d pixels" % int((np.isfinite(d) != f).sum())
    if not f.any():
        return 0.0
    scale = np.sqrt(dref[f]).max()
    err = float(np.abs(np.sqrt(d[f]) - np.sqrt(dref[f])).max() / scale) if scale > 0 else float(np.abs(d[f]).max())
    assert err <= DIST_TOL, "sqrt-form error %.3e > %.0e" % (err, DIST_TOL)
    return err


def check_loss(loss, grad, oracle_loss, oracle_grad, sel=None, guard=None, sentinel=None):
    """loss and grad [B,2,H,W] within LOSS_TOL (relative; the gradient against its largest oracle entry); the gradient exactly 0
    at every unselected pixel (sel [B,H,W] bool; by default where the oracle's is 0 in both channels); a loss of exactly 0 when
    the oracle selects nothing.  guard: what lies behind the gradient buffer in memory, which must still hold `sentinel` --
    nothing is written past the plane.  Returns (relative loss error, gradient error over its scale)."""
    loss, grad, oracle_grad = float(loss), np.asarray(grad, np.float64), np.asarray(oracle_grad, np.float64)
    assert grad.shape == oracle_grad.shape, (grad.shape, oracle_grad.shape)
    if sel is None:
        sel = (oracle_grad != 0).any(axis=1)
    sel = np.asarray(sel, bool).reshape(grad.shape[0], grad.shape[2], grad.shape[3])
    off = ~np.broadcast_to(sel[:, None], grad.shape)
    assert not grad[off].any(), "%d gradient entries of unselected pixels are not 0" % int(np.count_nonzero(grad[off]))
    if guard is not None:
        assert np.all(np.asarray(guard) == sentinel), "written past the plane"
    if oracle_loss == 0.0:
        assert loss == 0.0 and not grad.any(), "nothing is selected: loss %r" % loss
        return 0.0, 0.0
    el = abs(loss - oracle_loss) / abs(oracle_loss)
    assert el <= LOSS_TOL, "loss %r, oracle %r: relative error %.3e > %.0e" % (loss, oracle_loss, el, LOSS_TOL)     # and on NaN
    scale = np.abs(oracle_grad).max()
    eg = float(np.abs(grad - oracle_grad).max() / scale)
    assert eg <= LOSS_TOL, "gradient error %.3e of its largest entry > %.0e" % (eg, LOSS_TOL)
    return el, eg


# ---------------------------------------------------------------- settings that reach every branch of the select kernel
def ratio_with_fraction(nfin, lo, hi, start):
    """The first q = start + 0.0137 i whose virtual index (nfin - 1) q has a fractional part in [lo, hi)."""
    for i in range(1000):
        q = start + 0.0137 * i
        vi = (nfin - 1) * q
        if 0 < q < 1 and lo <= vi - np.floor(vi) < hi:
            return q
    raise ValueError("no ratio for %d" % nfin)


def quantile_low_branch(x, q):
    """NOT numpy's: the linear quantile with _lerp's `t >= 0.5` branch left out, always a + (b - a) g."""
    x = np.sort(x)
    vi = (x.size - 1) * q
    k = int(np.floor(vi))
    a, b = x[k], x[min(k + 1, x.size - 1)]
    return a + (b - a) * (vi - k)


def sparse_flow(name, n_finite, seed=11):
    """The case's flow with flow[0] = inf at all but n_finite pixels (chosen among its finite ones): a distance map with
    exactly n_finite finite entries.  Few, widely spaced distances are also the only maps on which _lerp's two expressions differ
    in their bits -- between neighbours of a dense map (b - a) g is far below an ulp of a and both round alike."""
    fl = case_flow(name)
    ok = np.flatnonzero(np.isfinite(fl).all(axis=0).ravel())
    keep = np.random.default_rng(seed).choice(ok, n_finite, replace=False)
    u = np.full(fl[0].size, np.inf, np.float32)
    u[keep] = fl[0].ravel()[keep]
    fl[0] = u.reshape(fl[0].shape)
    return fl


SPARSE_RATIOS = (0.05, 0.2, 0.3, 0.5, 0.55, 0.6, 0.7, 0.8, 0.9, 0.95)


def integral_ratio(nfin, start=0.2):
    """A q in (0, 1) whose virtual index (nfin - 1) q is an integer as fp64 computes it."""
    for k in range(int(start * (nfin - 1)) + 1, nfin - 1):
        q = k / (nfin - 1)
        if (nfin - 1) * q == float(k):
            return q
    raise ValueError("no integral ratio for %d" % nfin)


def select_settings(d):
    """[(tag, tau, keep_ratio, min_keep)] for a map d with at least a few hundred finite distances: the three branches of numpy's
    linear interpolation (fraction < 0.5, >= 0.5, integral virtual index) for keep_ratio and for min_keep, each step switched
    off from either side of (0, 1), tau below and above the quantile, and a min_keep that does / does not start the relaxation."""
    d = np.asarray(d)
    fin = d[np.isfinite(d)]
    nfin, big, srt = fin.size, 1e300, np.sort(fin)
    # tau values half way between two neighbouring distances, so that no distance sits at a tau
    mid, low = (float(0.5 * (srt[k] + srt[k + 1])) for k in (nfin // 2, nfin // 10))
    lo, hi, it = ratio_with_fraction(nfin, 0.05, 0.5, 0.2), ratio_with_fraction(nfin, 0.5, 0.95, 0.2), integral_ratio(nfin)
    return [("defaults", 1.0, 0.2, 0.05),
            ("frac<0.5", big, lo, 0.05),
            ("frac>=0.5", big, hi, 0.05),
            ("integral", big, it, 0.05),
            ("tau-below-quantile", low, 0.2, 0.05),
            ("keep-off-high", mid, 1.5, 0.05),
            ("keep-off-low", mid, 0.0, 0.05),
            ("keep-off-one", mid, 1.0, 0.3),
            ("min-off-high", big, lo, 1.0),
            ("min-off-low", big, hi, -0.5),
            ("both-off", mid, 0.0, 1.0),
            ("relax-frac<0.5", big, 0.2, ratio_with_fraction(nfin, 0.05, 0.5, 0.5)),
            ("relax-frac>=0.5", big, 0.2, ratio_with_fraction(nfin, 0.5, 0.95, 0.5)),
            ("relax-integral", big, 0.2, integral_ratio(nfin, 0.5)),
            ("relax-tightens", low, 0.2, 0.15),
            ("no-relax", big, hi, 0.1)]
