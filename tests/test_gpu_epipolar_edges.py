"""GPU checks of csrc/pwc_epipolar.hip off the two aligned geometries of the g9 fixture: the ragged cases of
tests/epipolar_cases.py against the float64 NumPy oracle (tests/epipolar_oracle.py), through the comparators that
tests/test_epipolar_cases_cpu.py shows can fail.  Every bound is one the project already asserts for the same quantity (1e-8 on F,
1e-6 on loss and gradient, 1e-9 in sqrt form on d, a 1e-4 share of threshold pixels, bit-equality of thr, of the pairs and of every
count); each test prints the worst value it saw (`pytest -s`).

Worst values seen on an MI355X (2026-10-18, kernels as of f39da20; none within a factor of 10 of its bound):
  ||F - F_ref|| / ||F_ref||      9.1e-12 (tie-rule table; 7.3e-12 holes-multi-chunk, 8.3e-15 eight-inliers)   bound 1e-8
  sqrt-form distance error       5.5e-14 (holes-multi-chunk)                                                 bound 1e-9
  pixels off the oracle's mask   0 in all 5 cases x 16 settings and in the mixed batch                        bound 1e-4 of the pixels
  loss, relative                 5.4e-8 (5x7 huber)                                                          bound 1e-6
  gradient / its largest entry   5.6e-8 (5x7 huber)                                                          bound 1e-6
  pairs, N, ok, best, every count, thr: equal to the oracle (thr: to numpy on the kernel's own distances) bit for bit
The loss and gradient figures are float32 rounding of the outputs (2^-24 = 6.0e-8).
"""
import numpy as np
import pytest
import torch

import epipolar_cases as EC
import epipolar_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _report(what, value, bound=None):
    print("[epipolar-edges] %s = %.3e%s" % (what, value, "" if bound is None else " (bound %.0e)" % bound))


def _strided(arr, dev, extra=37):
    """Device view of arr [B,...] (float32) whose batch stride is larger than a sample; the gap is NaN, so a kernel that ignores
    the stride shows (as test_gpu_pyr1_wino._strided)."""
    arr = np.ascontiguousarray(arr, np.float32)
    n = arr[0].size
    buf = torch.full((arr.shape[0], n + extra), NAN, device=dev)
    v = buf[:, :n].view(arr.shape)
    v.copy_(torch.from_numpy(arr))
    assert arr.shape[0] == 1 or v.stride(0) == n + extra
    return buf, v


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------------------------------------------------------- pairs
@pytest.mark.parametrize("name", EC.RANSAC_CASES)
def test_pairs_match_oracle(gpu_device, name):
    from opticalflow_amd import ops
    c = EC.CASES[name]
    fl = EC.case_flow(name)
    pts, n = ops.epipolar_pairs(_dev(fl[None], gpu_device), c.stride)
    assert tuple(pts.shape) == (1, EC.cap_of(c), 4) and int(n[0]) == EC.POINTS[name][0]
    EC.check_pairs(pts[0].cpu().numpy(), n[0], EC.oracle_pairs(fl, c.stride))


def test_pairs_mixed_batch_dense_and_strided(gpu_device):
    from opticalflow_amd import ops
    flows, mask = EC.mixed_batch()
    mt = _dev(mask, gpu_device)
    _, fv = _strided(flows, gpu_device)
    pd, nd = ops.epipolar_pairs(_dev(flows, gpu_device), EC.MIXED.stride, mt)
    ps, ns = ops.epipolar_pairs(fv, EC.MIXED.stride, mt)
    assert nd.tolist() == ns.tolist() == [512, 420, 5, 0]
    for b in range(4):
        rows = EC.oracle_pairs(flows[b], EC.MIXED.stride, mask[b])
        EC.check_pairs(pd[b].cpu().numpy(), nd[b], rows)
        EC.check_pairs(ps[b].cpu().numpy(), ns[b], rows)


def test_pairs_mask_dtypes_and_shapes(gpu_device):
    from opticalflow_amd import ops
    name = "holes-one-chunk"
    c = EC.CASES[name]
    fl = EC.case_flow(name)
    ft = _dev(fl[None], gpu_device)
    var, keep = EC.mask_variants(c.H, c.W)
    rows = EC.oracle_pairs(fl, c.stride, keep)
    first = None
    for kind, m in var.items():
        for shape in ((1, c.H, c.W), (1, 1, c.H, c.W)):
            mt = _dev(m, gpu_device).view(shape)
            assert str(mt.dtype) == "torch." + kind
            pts, n = ops.epipolar_pairs(ft, c.stride, mt)
            got = pts[0, :int(n[0])].cpu().numpy()
            EC.check_pairs(got, n[0], rows)
            first = got if first is None else first
            assert got.tobytes() == first.tobytes(), (kind, shape)


# ---------------------------------------------------------------------------------------------------------------- RANSAC
def _run_ex(flow_t, c, iters=None, mask=None):
    from opticalflow_amd import epipolar
    return epipolar.ransac_fundamental_ex(flow_t, c.stride, c.thresh, c.iters if iters is None else iters, EC.SAMPLER_SEED, mask)


@pytest.mark.parametrize("name", EC.RANSAC_CASES)
def test_ransac_matches_oracle(gpu_device, name):
    c = EC.CASES[name]
    fit = EC.oracle_fit(name)
    F, ok, best, counts, N = _run_ex(_dev(EC.case_flow(name)[None], gpu_device), c)
    assert N == [EC.POINTS[name][0]] and tuple(counts.shape) == (1, c.iters) and counts.dtype == torch.int32
    rel = EC.check_ransac(F[0].cpu().numpy(), ok[0], best[0], counts[0].cpu().numpy(), fit)
    _report("%s ||F - F_ref|| / ||F_ref||" % name, rel, EC.F_TOL)
    if name == "eight-inliers":
        assert int(counts[0].max()) == 8


@pytest.mark.parametrize("iters", [1, 63, 64, 65])
def test_ransac_shorter_runs_are_prefixes(gpu_device, iters):
    """one block of 64 hypotheses less one, exactly, plus one; and a single hypothesis"""
    name = "one-chunk-ragged"
    c = EC.CASES[name]
    ft = _dev(EC.case_flow(name)[None], gpu_device)
    full = _run_ex(ft, c)[3][0].cpu().numpy()
    F, ok, best, counts, _ = _run_ex(ft, c, iters)
    assert np.array_equal(counts[0].cpu().numpy(), full[:iters])
    rel = EC.check_ransac(F[0].cpu().numpy(), ok[0], best[0], counts[0].cpu().numpy(), EC.oracle_fit(name, iters))
    _report("%s/%d iterations ||F - F_ref|| / ||F_ref||" % (name, iters), rel, EC.F_TOL)


def test_ransac_mixed_batch(gpu_device):
    """N = [512, 420, 5, 0] in one call: per-sample index tables ([B,iters,8]) next to samples that cannot be fitted, on a
    batch-strided flow; the good samples equal their single-sample runs (shared table) bit for bit"""
    flows, mask = EC.mixed_batch()
    c = EC.MIXED
    mt = _dev(mask, gpu_device)
    _, fv = _strided(flows, gpu_device)
    F, ok, best, counts, N = _run_ex(fv, c, mask=mt)
    assert N == [512, 420, 5, 0] and ok.tolist() == [True, True, False, False]
    for b in range(4):
        rel = EC.check_ransac(F[b].cpu().numpy(), ok[b], best[b], counts[b].cpu().numpy(), EC.oracle_fit_mixed(b))
        _report("mixed-batch[%d] ||F - F_ref|| / ||F_ref||" % b, rel, EC.F_TOL)
    for b in (2, 3):
        assert int(best[b]) == -1 and not F[b].any() and not counts[b].any()
    for b in (0, 1):
        F1, ok1, best1, c1, N1 = _run_ex(_dev(flows[b:b + 1], gpu_device), c, mask=mt[b:b + 1])
        assert N1 == [N[b]] and bool(ok1[0])
        assert _bits(F1[0]) == _bits(F[b]) and _bits(c1[0]) == _bits(counts[b]) and int(best1[0]) == int(best[b])


def _pairs_and_table(name, iters, dev):
    from opticalflow_amd import ops
    c = EC.CASES[name]
    fl = EC.case_flow(name)
    pts, n = ops.epipolar_pairs(_dev(fl[None], dev), c.stride)
    return c, fl, pts, n, O.index_table(int(n[0]), EC.SAMPLER_SEED, iters)


def test_argmax_keeps_the_first_of_equal_counts(gpu_device):
    """the winner's row copied to three later positions (EC.tie_rule_fit): another lane of its wave, the same lane one stride of
    256 later, and the last, partial block of 64 hypotheses -- across lanes (shuffle), a lane's own loop and waves (LDS)"""
    from opticalflow_amd import ops
    fit, b0, later = EC.tie_rule_fit()
    c, fl, pts, n, _ = _pairs_and_table(EC.TIE_CASE, 1, gpu_device)
    F, ok, best, counts = ops.epipolar_ransac(pts, n, _dev(fit["idx"], gpu_device), c.thresh)
    rel = EC.check_ransac(F[0].cpu().numpy(), ok[0], best[0], counts[0].cpu().numpy(), fit)
    assert int(best[0]) == b0 and all(int(counts[0, p]) == int(counts[0, b0]) for p in later)
    _report("tie rule ||F - F_ref|| / ||F_ref||", rel, EC.F_TOL)


def test_out_of_range_index_gives_a_dead_hypothesis(gpu_device):
    """a table row with an index >= N (or < 0) is a documented input: that hypothesis is NaN and counts 0, the others are untouched"""
    from opticalflow_amd import ops
    name = "sub-wave"
    c, fl, pts, n, table = _pairs_and_table(name, EC.CASES[name].iters, gpu_device)
    N = int(n[0])
    clean = EC.oracle_fit(name)
    dead = [r for r in (3, 40, 63) if r != clean["best"]]
    table = table.copy()
    for r, v in zip(dead, (N, -1, 2 ** 31 - 1)):
        table[r, 5] = v
    fit = EC.oracle_ransac(fl, c.stride, c.thresh, None, idx=table)
    F, ok, best, counts = ops.epipolar_ransac(pts, n, _dev(table, gpu_device), c.thresh)
    got = counts[0].cpu().numpy()
    assert all(got[r] == 0 for r in dead)
    keep = np.ones(c.iters, bool)
    keep[dead] = False
    assert np.array_equal(got[keep], clean["counts"][keep])
    EC.check_ransac(F[0].cpu().numpy(), ok[0], best[0], got, fit)
    assert int(best[0]) == clean["best"]


# ---------------------------------------------------------------------------------------------------------------- distance
def _poisoned(fl):
    """non-finite flow of each kind, in the first and the last pixel too"""
    fl = fl.copy()
    H, W = fl.shape[1:]
    fl[0, 0, 0] = -np.inf
    fl[1, H - 1, W - 1] = np.nan
    fl[1, H // 2, 1:W - 1:3] = np.inf
    fl[0, 1:H:4, W // 2] = np.nan
    return fl


@pytest.mark.parametrize("name", EC.RANSAC_CASES)
def test_sampson_distance_ragged(gpu_device, name):
    from opticalflow_amd import epipolar, ops
    F0 = EC.oracle_fit(name)["F"]
    F1 = EC.oracle_fit("sub-wave" if name != "sub-wave" else "one-chunk-ragged")["F"]
    flows = np.stack([EC.case_flow(name), _poisoned(EC.case_flow(name))])
    B, _, H, W = flows.shape
    _, fv = _strided(flows, gpu_device)
    shared = epipolar.sampson_distance(fv, F0).cpu().numpy()
    per = epipolar.sampson_distance(fv, _dev(np.stack([F0, F1]), gpu_device)).cpu().numpy()
    worst = 0.0
    for b in range(B):
        worst = max(worst, EC.check_distance(shared[b], EC.oracle_distance(flows[b], F0)),
                    EC.check_distance(per[b], EC.oracle_distance(flows[b], (F0, F1)[b])))
    assert np.isfinite(shared[1]).sum() < np.isfinite(shared[0]).sum()
    _report("%s sqrt-form distance error" % name, worst, EC.DIST_TOL)
    # a caller's output buffer: nothing behind the last plane is written
    big = torch.full((B * H * W + 300,), 777.0, dtype=torch.float64, device=gpu_device)
    out = ops.epipolar_distance(fv, F0, out=big[:B * H * W].view(B, H, W))
    assert _bits(out) == _bits(torch.from_numpy(shared)) and bool((big[B * H * W:] == 777.0).all())


# ---------------------------------------------------------------------------------------------------------------- threshold, mask
def _mask_run(flow_t, F, ok, tau, kr, mk):
    from opticalflow_amd import ops
    B, _, H, W = flow_t.shape
    d = torch.full((B, H, W), -1.0, dtype=torch.float64, device=flow_t.device)
    Ft = _dev(np.asarray(F, np.float64).reshape(-1, 9), flow_t.device)
    mask, thr = ops.epipolar_mask(flow_t, Ft, torch.as_tensor(ok, dtype=torch.int32, device=flow_t.device), tau, kr, mk, dist_out=d)
    assert tuple(mask.shape) == (B, 1, H, W) and mask.dtype == torch.bool
    return mask[:, 0].cpu().numpy(), thr.cpu().numpy(), d.cpu().numpy()


@pytest.mark.parametrize("name", EC.RANSAC_CASES)
def test_mask_every_select_branch(gpu_device, name):
    """every setting of EC.select_settings: thr is numpy's quantile logic on the kernel's own distances bit for bit, the mask is
    finite & (d <= thr), and against the oracle's mask only threshold pixels differ (at most 1e-4 of them)"""
    fl = EC.case_flow(name)
    F = EC.oracle_fit(name)["F"]
    dref = EC.oracle_distance(fl, F)
    ft = _dev(fl[None], gpu_device)
    differing = 0
    for tag, tau, kr, mk in EC.select_settings(dref):
        mask, thr, d = _mask_run(ft, F, [1], tau, kr, mk)
        EC.check_distance(d[0], dref)
        try:
            EC.check_threshold(thr[0], mask[0], d[0], tau, kr, mk)
            differing += EC.check_mask_against_oracle(mask[0], thr[0], fl, F, tau, kr, mk)
        except AssertionError as e:
            raise AssertionError("%s / %s (tau %r keep_ratio %r min_keep %r): %s" % (name, tag, tau, kr, mk, e)) from None
    _report("%s pixels that differ from the oracle's mask, all settings" % name, differing)


def test_mask_under_ties(gpu_device):
    """F = [[0,0,0],[0,0,-1],[0,1,0]]: d depends on flow[1] only, drawn from nine values: every order statistic is tied many
    times over, inside one radix bucket on every pass, and many d are exactly 0"""
    H, W = 37, 53
    g = np.random.default_rng(21)
    fl = np.stack([g.standard_normal((H, W)), g.integers(0, 9, (H, W)) * 0.25]).astype(np.float32)
    F = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    ft = _dev(fl[None], gpu_device)
    dref = EC.oracle_distance(fl, F)
    assert (dref == 0).sum() > 100
    n = 0
    for tag, tau, kr, mk in EC.select_settings(dref) + [("zero-quantile", 1e300, 0.03, 0.0), ("tau-zero", 0.0, 0.5, 0.05)]:
        mask, thr, d = _mask_run(ft, F, [1], tau, kr, mk)
        assert (d[0] == 0).sum() > 100 and len(np.unique(np.round(np.sqrt(d[0]) / 0.25 * np.sqrt(2.0)))) == 9
        try:
            EC.check_threshold(thr[0], mask[0], d[0], tau, kr, mk)
        except AssertionError as e:
            raise AssertionError("ties / %s: %s" % (tag, e)) from None
        n += 1
    _report("tied settings checked", n)


def test_mask_degenerate_maps(gpu_device):
    """one huge constant distance at every pixel (F = diag(0, 0, 1)); maps with exactly one, two and five finite distances (on
    which numpy's two interpolation expressions differ in their bits); no finite distance at all; a failed fit"""
    name = "one-chunk-ragged"
    fl = EC.case_flow(name)
    ft = _dev(fl[None], gpu_device)
    diag = np.diag([0.0, 0.0, 1.0])
    for tau, kr, mk in ((1e300, 0.2, 0.05), (1e300, 0.5, 0.9), (1.0, 0.2, 0.05), (1e300, 1.0, 1.0)):
        mask, thr, d = _mask_run(ft, diag, [1], tau, kr, mk)
        assert np.isfinite(d).all() and d.min() == d.max() and d.max() > 1e11
        EC.check_threshold(thr[0], mask[0], d[0], tau, kr, mk)
        assert mask.all() == (tau > 1.0)
    F = EC.oracle_fit(name)["F"]
    told = 0
    for nf in (1, 2, 5):
        sp = EC.sparse_flow(name, nf)
        st = _dev(sp[None], gpu_device)
        dref = EC.oracle_distance(sp, F)
        assert np.isfinite(dref).sum() == nf
        for q in EC.SPARSE_RATIOS:
            for tau, kr, mk in ((1e300, q, 0.0), (1e300, 1e-9, q), (1.0, q, q)):
                mask, thr, d = _mask_run(st, F, [1], tau, kr, mk)
                EC.check_distance(d[0], dref)
                EC.check_threshold(thr[0], mask[0], d[0], tau, kr, mk)
                assert mask.sum() >= 1
                told += EC.numpy_threshold(d[0], tau, kr, mk, quantile=EC.quantile_low_branch)[0] != float(thr[0])
    assert told >= 4          # the sparse maps did tell _lerp's two expressions apart, and the kernel took numpy's
    # no finite distance (ok = 1) and a failed fit (ok = 0) next to a good sample
    flows = np.stack([fl, np.full_like(fl, np.nan), fl])
    _, fv = _strided(flows, gpu_device)
    mask, thr, d = _mask_run(fv, np.stack([F, F, F]), [1, 1, 0], 1.0, 0.2, 0.05)
    EC.check_threshold(thr[0], mask[0], d[0], 1.0, 0.2, 0.05)
    EC.check_threshold(thr[1], mask[1], d[1], 1.0, 0.2, 0.05)
    assert np.isnan(thr[1]) and mask[1].all() and not np.isfinite(d[1]).any()
    assert np.isnan(thr[2]) and mask[2].all() and not mask[0].all()


def test_mask_mixed_batch_matches_oracle(gpu_device):
    """build_epipolar_mask_from_flow's tail on the mixed batch with 130-iteration fits: good samples against the oracle's mask,
    failed ones all true"""
    from opticalflow_amd import ops
    flows, mask = EC.mixed_batch()
    c = EC.MIXED
    _, fv = _strided(flows, gpu_device)
    F, ok, _, _, _ = _run_ex(fv, c, mask=_dev(mask, gpu_device))
    d = torch.empty((4, c.H, c.W), dtype=torch.float64, device=gpu_device)
    m, thr = ops.epipolar_mask(fv, F.view(4, 9), ok, 1.0, 0.2, 0.05, dist_out=d)
    m, thr, d = m[:, 0].cpu().numpy(), thr.cpu().numpy(), d.cpu().numpy()
    for b in (0, 1):
        EC.check_threshold(thr[b], m[b], d[b], 1.0, 0.2, 0.05)
        EC.check_mask_against_oracle(m[b], thr[b], flows[b], EC.oracle_fit_mixed(b)["F"], 1.0, 0.2, 0.05)
    assert m[2].all() and m[3].all() and np.isnan(thr[2:]).all()


# ---------------------------------------------------------------------------------------------------------------- soft loss
LOSS_PLANES = ((5, 7), (37, 53), (61, 127))
MASK_KINDS = ("none", "float32", "uint8", "float16", "int32")


def _loss_mask(kind, shape, seed):
    """(mask array or None, selected [B,H,W] bool by the rule `value > 0.5`): float32 holds exactly 0.5 (out), the next float
    above it (in) and NaN (out); uint8 holds 0, 1 and 255; float16 and int32 go through the wrapper's threshold rule"""
    if kind == "none":
        return None, np.ones(shape, bool)
    g = np.random.default_rng(seed)
    vals = {"float32": np.array([0.0, 0.5, np.nextafter(np.float32(0.5), np.float32(1.0)), np.nan, 1.0, 0.25], np.float32),
            "uint8": np.array([0, 1, 255], np.uint8),
            "float16": np.array([0.0, 0.5, 0.5 + 2.0 ** -11, 0.75, 1.0], np.float16),
            "int32": np.array([0, 1, -3, 7], np.int32)}[kind]
    m = vals[g.integers(0, len(vals), shape)]
    with np.errstate(invalid="ignore"):
        return m, m.astype(np.float64) > 0.5


def _loss_grad(fv_buf, fv, F, mask, robust, delta, ok, scale=3.0):
    from opticalflow_amd import epipolar
    fv_buf.grad = None
    loss = epipolar.epipolar_sampson_loss(fv, F, valid_mask=mask, robust=robust, delta=delta, weight=0.1, ok=ok)
    (scale * loss).backward()
    n = fv[0].numel()
    gap = fv_buf.grad[:, n:]
    assert not gap.any()                     # the NaN gap between the samples took no part
    return loss.detach(), fv_buf.grad[:, :n].reshape(fv.shape).clone()


@pytest.mark.parametrize("robust", ["huber", "l1", "mean"])
@pytest.mark.parametrize("plane", LOSS_PLANES, ids=lambda p: "%dx%d" % p)
def test_soft_loss_ragged(gpu_device, plane, robust):
    """B = 3 with ok = [True, False, True] and a per-sample F on a batch-strided flow, every mask kind: loss and gradient
    against the oracle, exact zeros at every unselected pixel (the whole failed sample between two ragged planes included),
    3.0 * loss scales the gradient, and a second call gives the same bits"""
    H, W = plane
    B = 3
    flows = np.stack([O.rigid_flow(H, W, 300 + b) for b in range(B)])
    Fs = np.stack([EC.oracle_fit(n)["F"] for n in ("one-chunk-ragged", "sub-wave", "holes-one-chunk")])
    okn = np.array([True, False, True])
    F32 = Fs.astype(np.float32)
    delta = 1.0
    if robust == "huber":
        # a delta between the residuals: both branches occur
        r = np.sqrt(np.stack([EC.oracle_distance(flows[b], F32[b]) for b in (0, 2)]))
        delta = float(np.median(r))
        assert (r <= 0.9 * delta).any() and (r > 1.1 * delta).any()
    buf, fv = _strided(flows, gpu_device)
    buf.requires_grad_(True)
    fv = buf[:, :2 * H * W].view(B, 2, H, W)
    Ft, okt = _dev(Fs, gpu_device), torch.tensor(okn, device=gpu_device)
    worst_l = worst_g = 0.0
    for kind in MASK_KINDS:
        for shape in ((B, H, W), (B, 1, H, W)):
            m, sel = _loss_mask(kind, (B, H, W), 17)
            mt = None if m is None else _dev(m, gpu_device).view(shape)
            loss, g = _loss_grad(buf, fv, Ft, mt, robust, delta, okt)
            lr, gr = O.soft_loss(flows, F32, None if m is None else sel.astype(np.float64), robust, delta, 0.1, okn)
            sel = sel & okn[:, None, None]
            assert 0 < sel.sum() < B * H * W and (gr != 0).any(axis=1).sum() == sel.sum()
            try:
                el, eg = EC.check_loss(loss, g.cpu().numpy(), lr, 3.0 * gr, sel)
            except AssertionError as e:
                raise AssertionError("%dx%d %s mask %s %s: %s" % (H, W, robust, kind, shape, e)) from None
            # the selected count the kernel used, implied by its gradient's support
            assert int((g != 0).any(dim=1).sum()) == int(sel.sum())
            worst_l, worst_g = max(worst_l, el), max(worst_g, eg)
            if shape == (B, H, W):
                loss2, g2 = _loss_grad(buf, fv, Ft, mt, robust, delta, okt)
                assert _bits(loss) == _bits(loss2) and _bits(g) == _bits(g2)
                l1, g1 = _loss_grad(buf, fv, Ft, mt, robust, delta, okt, scale=1.0)
                assert _bits(l1) == _bits(loss)
                assert np.abs(g.cpu().numpy() - 3.0 * g1.cpu().numpy()).max() <= 2.0 ** -22 * np.abs(g.cpu().numpy()).max()
    _report("%dx%d %s loss error" % (H, W, robust), worst_l, EC.LOSS_TOL)
    _report("%dx%d %s gradient error" % (H, W, robust), worst_g, EC.LOSS_TOL)


@pytest.mark.parametrize("plane", LOSS_PLANES, ids=lambda p: "%dx%d" % p)
def test_soft_loss_backward_writes_nothing_past_the_plane(gpu_device, plane):
    """the C entry on a gradient buffer with a sentinel behind it: the last, partly filled workgroup stops at the plane"""
    from opticalflow_amd import _lib, ops
    from opticalflow_amd._lib import check
    H, W = plane
    B, n = 2, 2 * H * W
    flows = np.stack([O.rigid_flow(H, W, 310 + b) for b in range(B)])
    F = EC.oracle_fit("one-chunk-ragged")["F"]
    ft, Ft = _dev(flows, gpu_device), _dev(F.reshape(9), gpu_device)
    up = torch.tensor([3.0], device=gpu_device)
    big = torch.full((B * n + 1000,), 777.0, device=gpu_device)
    with torch.cuda.device(gpu_device):
        ws, nb = ops._loss_workspace(B, H, W, gpu_device)
        rc = _lib.load().pwc_epipolar_loss_bwd(ft.data_ptr(), Ft.data_ptr(), 0, None, 0, None, 0, up.data_ptr(), big.data_ptr(), B, H, W,
                                               1, 1.0, 0.1, n, 0, ws.data_ptr(), nb, torch.cuda.current_stream(gpu_device).cuda_stream)
    check(rc, "pwc_epipolar_loss_bwd")
    torch.cuda.synchronize(gpu_device)
    lr, gr = O.soft_loss(flows, F.astype(np.float32), None, "l1", 1.0, 0.1)
    got = big.cpu().numpy()
    EC.check_loss(lr, got[:B * n].reshape(B, 2, H, W), lr, 3.0 * gr, guard=got[B * n:], sentinel=777.0)


# ---------------------------------------------------------------------------------------------------------------- reproducibility
def _every_entry(flows, mask, c, dev):
    """every entry point once, on a batch-strided flow -> {name: bytes}"""
    from opticalflow_amd import epipolar, ops
    out = {}
    B = flows.shape[0]
    buf, fv = _strided(flows, dev)
    mt = None if mask is None else _dev(mask, dev)
    pts, n = ops.epipolar_pairs(fv, c.stride, mt)
    N = n.tolist()
    out["pairs"] = b"".join(_bits(pts[b, :N[b]]) for b in range(B)) + _bits(n)
    F, ok, best, counts, _ = _run_ex(fv, c, mask=mt)
    out["ransac"] = _bits(F) + _bits(ok) + _bits(best) + _bits(counts)
    out["distance"] = _bits(epipolar.sampson_distance(fv, F))
    d = torch.empty((B, c.H, c.W), dtype=torch.float64, device=dev)
    m, thr = ops.epipolar_mask(fv, F.view(B, 9), ok, 1.0, 0.2, 0.05, dist_out=d)
    out["mask"] = _bits(m) + _bits(thr) + _bits(d)
    m2, thr2 = epipolar.build_epipolar_mask_from_flow(fv, 1.0, c.stride, mt, return_thr=True)
    out["build_mask"] = _bits(m2) + _bits(thr2)
    buf.requires_grad_(True)
    fg = buf[:, :fv[0].numel()].view(fv.shape)
    loss, g = _loss_grad(buf, fg, F, m, "huber", 0.05, ok)
    out["loss"] = _bits(loss) + _bits(g)
    return out


@pytest.mark.parametrize("name", ["holes-multi-chunk", "mixed-batch"])
def test_every_entry_point_is_bit_reproducible(gpu_device, name):
    """twice on the multi-chunk case (counts summed by integer atomics over four score chunks) and on the mixed batch"""
    if name == "mixed-batch":
        flows, mask = EC.mixed_batch()
        c = EC.MIXED
    else:
        flows, mask, c = EC.case_flow(name)[None], None, EC.CASES[name]
    a, b = _every_entry(flows, mask, c, gpu_device), _every_entry(flows, mask, c, gpu_device)
    for k in a:
        assert a[k] == b[k], k
