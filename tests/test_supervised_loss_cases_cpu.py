"""CPU checks of tests/supervised_loss_cases.py, with the fp64 oracle alone: the conditions on the inputs under which a passing
tests/test_gpu_supervised_loss_edges.py means something -- every geometry is one the kernels accept and has the chunk arithmetic
its name promises; no photometric sample sits on an integer, no residual or neighbour difference on a kink, no mask value on the
threshold; taps fall inside and outside the level; a dropped last row or column moves loss and gradient by at least ten bounds --
a tie of the oracle to the torch route in float64 and of its index arithmetic to torch's interpolate at the new ratios, and a
negative control per comparator."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import supervised_loss_cases as SC
import supervised_loss_oracle as O

FLOW_IDS = ["%s-%s-%s" % (n, r, m) for n in SC.FLOW_CASES for r, _, m in SC.FLOW_SETTINGS]
FLOW_PARAMS = [(n, r, e, m) for n in SC.FLOW_CASES for r, e, m in SC.FLOW_SETTINGS]
MS_PARAMS = [(n, t) for n in SC.MS_CASES for t in SC.TERMS]
MS_IDS = ["%s-%s" % p for p in MS_PARAMS]


def test_tables_are_the_planned_ones():
    assert {n: tuple(c) for n, c in SC.FLOW_CASES.items()} == {
        "tail-1": (2, 17, 65, 5, 17), "chunk-exact": (1, 32, 32, 8, 8), "chunk-plus-1": (1, 25, 41, 5, 9), "same": (1, 15, 63, 15, 63),
        "min-2x2": (2, 2, 2, 2, 2), "min-3-from-2": (1, 3, 3, 2, 2), "coarse-2x2": (1, 40, 130, 2, 2), "near-1": (1, 33, 70, 32, 69),
        "row-same": (2, 24, 96, 24, 24), "col-same": (2, 24, 96, 6, 96)}
    geo = {n: (c.B, c.H, c.W, c.levels) for n, c in SC.MS_CASES.items()}
    l8 = ((40, 56), (20, 28), (13, 19), (10, 14), (7, 9), (5, 7), (3, 4), (2, 2))
    assert geo == {"ms-ragged": (2, 37, 83, ((10, 21), (5, 11), (3, 6), (2, 3))),
                   "ms-chunks": (1, 64, 96, ((32, 32), (25, 41), (64, 96), (2, 2))),
                   "ms-chunks-b2": (2, 64, 96, ((32, 32), (25, 41), (64, 96), (2, 2))),
                   "ms-8": (1, 40, 56, l8), "ms-8w": (1, 40, 56, l8), "ms-1": (2, 17, 65, ((5, 17),)),
                   "ms-64": (1, 128, 192, ((2, 3),)), "ms-twins": (1, 12, 20, ((6, 10), (6, 10)))}
    assert SC.TERMS == {"charb": ("binary", 0.0, 0.0), "photo": ("0.4", 0.4, 0.0), "smooth": ("zero", 0.0, 0.2), "all": ("frac", 0.4, 0.2)}
    assert (SC.LOSS_RTOL, SC.LOSS_ATOL, SC.GRAD_TOL, SC.SENSITIVITY) == (1e-5, 1e-9, 1e-4, 10.0)
    assert (SC.COORD_MARGIN, SC.RESID_MARGIN, SC.DIFF_MARGIN, SC.MASK_MARGIN) == (1e-3, 1e-4, 1e-4, 1e-3)
    assert SC.MS_CASES["ms-1"].one_tensor and SC.MS_CASES["ms-8"].w is None and len(set(SC.MS_CASES["ms-8w"].w)) == 8


# ---------------------------------------------------------------- geometry and chunk arithmetic
@pytest.mark.parametrize("name", list(SC.FLOW_CASES))
def test_flow_geometry_is_accepted_and_is_what_the_name_promises(name):
    from opticalflow_amd import ops
    c = SC.FLOW_CASES[name]
    assert ops._sup_geometry_ok(c.H, c.W, c.h, c.w) and SC.geometry_ok(c.H, c.W, c.h, c.w) and 2 * c.H * c.W < 2 ** 31
    pred, gt = SC.flow_inputs(name)
    assert tuple(pred.shape) == (c.B, 2, c.h, c.w) and tuple(gt.shape) == (c.B, 2, c.H, c.W) and pred.dtype == gt.dtype == torch.float32
    assert not ops.sup_flow_loss_supported(pred, gt)                      # CPU tensors
    n = c.B * c.H * c.W
    chunks, tail = SC.blocks_of(n), (n - 1) % SC.CHUNK + 1
    want = {"tail-1": (2210, 3, 162), "chunk-exact": (1024, 1, 1024), "chunk-plus-1": (1025, 2, 1), "same": (945, 1, 945),
            "min-2x2": (8, 1, 8), "min-3-from-2": (9, 1, 9), "coarse-2x2": (5200, 6, 80), "near-1": (2310, 3, 262),
            "row-same": (4608, 5, 512), "col-same": (4608, 5, 512)}[name]
    assert (n, chunks, tail) == want
    rh, rw = np.float32(c.h) / np.float32(c.H), np.float32(c.w) / np.float32(c.W)
    if name == "tail-1":
        assert (c.H / c.h, round(c.W / c.w, 2)) == (3.4, 3.82) and c.H * c.W % SC.CHUNK != 0 and c.H * c.W > SC.CHUNK
    if name == "near-1":
        assert 0.96 < rh < 1 and 0.98 < rw < 1
    if name == "row-same":
        assert rh == 1.0 and rw == 0.25
    if name == "col-same":
        assert rw == 1.0 and rh == 0.25
    if name == "coarse-2x2":
        assert c.W / c.w == 65 and c.h * c.w == 4
    if name in ("same", "min-2x2"):
        assert (c.h, c.w) == (c.H, c.W)
    # the gather of every low-resolution index is not empty, and the last full-resolution index uses the last source index
    for n_in, n_out in ((c.h, c.H), (c.w, c.W)):
        A = O.interp_matrix(n_in, n_out)
        assert (A.sum(0) > 0).all() and A[-1, n_in - 1] > 0 and np.allclose(A.sum(1), 1.0)
    assert SC.flow_min_epe(name) >= 2.5                                   # the GT is a few pixels from the scaled prediction


@pytest.mark.parametrize("name", list(SC.MS_CASES))
def test_multiscale_geometry_is_accepted_and_is_what_the_name_promises(name):
    from opticalflow_amd import ops
    c = SC.MS_CASES[name]
    L = len(c.levels)
    assert 1 <= L <= SC.MAX_LEVELS == ops.SUP_MAX_LEVELS and 6 * c.H * c.W < 2 ** 31
    assert all(ops._sup_geometry_ok(c.H, c.W, h, w) for h, w in c.levels)
    preds, img, gt, mask, lp, ls = SC.ms_inputs(name, "all")
    assert [tuple(p.shape) for p in preds] == [(c.B, 2, h, w) for h, w in c.levels]
    assert tuple(img.shape) == (c.B, 6, c.H, c.W) and tuple(gt.shape) == (c.B, 2, c.H, c.W) and tuple(mask.shape) == (c.B, c.H, c.W)
    assert not ops.sup_multiscale_loss_supported(preds, gt, mask, img)    # CPU tensors
    px = [c.B * h * w for h, w in c.levels]
    first, grid = SC.blk0(name)
    wts = SC.level_weights(name)
    assert len(wts) == L
    if name == "ms-ragged":
        assert px == [420, 110, 36, 12] and first == [0, 1, 2, 3] and grid == 4
        assert all(c.H % h and c.W % w for h, w in c.levels)              # no integer ratio
    if name == "ms-chunks":
        assert px == [1024, 1025, 6144, 4] and first == [0, 1, 3, 9] and grid == 10
        assert c.levels[2] == (c.H, c.W) and px != sorted(px, reverse=True)
    if name == "ms-chunks-b2":
        assert px == [2048, 2050, 12288, 8] and first == [0, 2, 5, 17] and grid == 18
    if name in ("ms-8", "ms-8w"):
        assert L == 8 and first == [0, 3, 4, 5, 6, 7, 8, 9] and grid == 10 and c.levels[0] == (c.H, c.W)
    if name == "ms-8":
        assert wts == (0.32, 0.08, 0.02, 0.01, 0.005, 0.005, 0.005, 0.005)
    if name == "ms-8w":
        assert wts == c.w and wts[4:] == (0.005, 0.004, 0.003, 0.002)
    if name == "ms-1":
        assert L == 1 and wts == (0.32,)
    if name == "ms-64":
        assert (c.H // c.levels[0][0], c.W // c.levels[0][1]) == (64, 64)
    if name == "ms-twins":
        assert c.levels[0] == c.levels[1] and wts[0] != wts[1] and not torch.equal(preds[0], preds[1])


# ---------------------------------------------------------------- conditions (a)-(f)
@pytest.mark.parametrize("name", list(SC.MS_CASES))
def test_multiscale_inputs_meet_the_conditions(name):
    s = SC.conditions(name)
    print("[sup-cases] %s: sample to integer %.1e, residual %.1e max|img|, neighbour difference %.1e, mask to 0.5 %.1e, taps "
          "inside / outside %d / %d, past (left, right, top, bottom) %s, least epe %.2e"
          % (name, s["coord"], s["resid"], s["diff"], s["mask"], s["taps"][0], s["taps"][1], s["sides"], s["epe"]))
    assert s["coord"] >= SC.COORD_MARGIN                                  # (a)
    assert s["resid"] >= SC.RESID_MARGIN                                  # (b), at every pixel and channel
    assert s["diff"] >= SC.DIFF_MARGIN                                    # (c)
    assert s["mask"] >= SC.MASK_MARGIN                                    # (d)
    assert s["taps"][0] > 0 and s["taps"][1] > 0 and s["taps"][0] > s["taps"][1]      # (e): both, and most inside
    assert s["epe"] >= 0.5                                                # far from eps = 1e-3: the slope d / epe is well conditioned


def test_photometric_samples_leave_the_level_on_every_side():
    sides = np.array([SC.conditions(n)["sides"] for n in SC.MS_CASES])
    assert (sides[[list(SC.MS_CASES).index(n) for n in SC.MS_CASES if n != "ms-64"]] > 0).all()     # a 2 x 3 level has 6 samples
    assert sides.sum(1).min() > 0


def test_mask_values_and_forms():
    for name in SC.MS_CASES:
        c = SC.MS_CASES[name]
        m = {t: SC.ms_inputs(name, t)[3].numpy() for t in SC.TERMS}
        assert set(np.unique(m["charb"])) <= {0.0, 1.0} and 0.3 < m["charb"].mean() < 0.9
        assert (m["photo"] == np.float32(0.4)).all() and not m["smooth"].any()
        f = m["all"]
        assert (f == 0).mean() > 0.1 and ((f > 0) & (f < 0.5)).any() and (f > 0.5).any() and np.abs(f - 0.5).min() >= SC.MASK_MARGIN
        # no pixel of the photo setting is valid, and every level of the all setting has valid and invalid pixels with weight
        for h, w in c.levels[:1]:
            ms = f[:, O.nearest_index(c.H, h)][:, :, O.nearest_index(c.W, w)]
            assert (ms > 0.5).any() and (h * w <= 6 or ((ms > 0) & (ms <= 0.5)).any())
    for name in SC.FLOW_CASES:
        c = SC.FLOW_CASES[name]
        edge, off, frac = (SC.flow_mask(name, k).numpy() for k in ("edge", "off", "frac"))
        assert edge.sum() == c.B * (c.H + c.W - 1) and edge[:, -1].all() and edge[:, :, -1].all() and not off.any()
        assert np.abs(frac - 0.5).min() >= SC.MASK_MARGIN and (frac.size < 100 or (frac == 0).any()) and SC.flow_mask(name, None) is None
    forms = SC.mask_forms(SC.flow_mask("tail-1", "binary").numpy())
    assert [t for t, _ in forms] == ["float32-3d", "float32-4d", "bool-3d", "bool-4d", "uint8-3d", "uint8-4d"]
    on = forms[0][1].numpy() > 0.5
    for tag, m in forms:
        assert str(m.dtype) == "torch." + tag[:-3] and m.dim() == int(tag[-2])
        assert np.array_equal((m.float() > 0.5).numpy().reshape(on.shape), on)
    assert (forms[4][1] == 255).any() and (forms[4][1] == 1).any()


@pytest.mark.parametrize("name", list(SC.FLOW_CASES))
def test_flow_last_row_and_column_move_loss_and_gradient(name):
    """(f) masking out the last image row, and the last column, moves the oracle's loss and gradient by at least 10 bounds"""
    (rl, rg), (cl, cg) = SC.flow_sensitivity(name)
    print("[sup-cases] %s: last row moves loss / gradient by %.0f / %.0f bounds, last column by %.0f / %.0f" % (name, rl, rg, cl, cg))
    assert min(rl, rg, cl, cg) >= SC.SENSITIVITY


@pytest.mark.parametrize("name,term", MS_PARAMS, ids=MS_IDS)
def test_multiscale_last_row_and_column_move_loss_and_gradient(name, term):
    """(f) per level: taking away what the level's last row (column) reads moves its loss and gradient by at least 10 bounds"""
    s = SC.ms_sensitivity(name, term)
    worst = min(v for lv in s for pair in lv for v in pair)
    print("[sup-cases] %s-%s: least change over levels, rows / columns, loss / gradient: %.0f bounds" % (name, term, worst))
    assert worst >= SC.SENSITIVITY, s


@pytest.mark.parametrize("name,term,kind", SC.ZERO_KINDS, ids=["%s-%s-%s" % z for z in SC.ZERO_KINDS])
def test_exact_zero_kinds(name, term, kind):
    ref, rough = SC.ms_oracle(name, term, kind), SC.ms_oracle(name, term)
    assert all(not g.any() for g in ref["grads"]) and all(g.any() for g in rough["grads"])
    if kind == "const":
        assert ref["total"] == 0.0            # mask 0: no Charbonnier term; |0| everywhere
    else:
        # zero padding: every tap is 0, so the level's loss is lambda_photo times the masked mean of |im1_s| and has no slope
        c = SC.MS_CASES[name]
        preds, img, gt, mask, lp, ls = SC.ms_inputs(name, term, kind)
        for li, (h, w) in enumerate(c.levels):
            im1 = O.resize(img.numpy()[:, :3], h, w)
            m = float(np.float32(0.4))
            want = lp * np.abs(im1).sum() * m / (m * c.B * h * w + 1e-8)
            assert abs(ref["levels"][li] - want) <= 1e-12 * want and want > 0.1


# ---------------------------------------------------------------- the oracle is tied to an independent implementation
@pytest.mark.parametrize("name,rule,eps,mk", FLOW_PARAMS, ids=FLOW_IDS)
def test_torch_route_fp64_reproduces_the_flow_oracle(name, rule, eps, mk):
    """MaskedCharbonnier / compute_epe(route="torch") in float64: 1e-6 on the loss, 1e-5 max|g| on the gradient (the g10 CPU
    test's bounds: the oracle rounds its source indices in float32, torch's float64 resize does not)."""
    from opticalflow_amd import losses
    pred, gt = (t.double() for t in SC.flow_inputs(name))
    m = SC.flow_mask(name, mk)
    p = pred.clone().requires_grad_(True)
    got = losses.MaskedCharbonnier(eps=eps, route="torch")(p, gt, m) if rule == "threshold" else losses.compute_epe(p, gt, m, route="torch")
    (g,) = torch.autograd.grad(got, p)
    ref = SC.flow_oracle(name, rule, eps, mk)
    np.testing.assert_allclose(got.item(), ref["loss"], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(g.numpy(), ref["grad"], rtol=0, atol=1e-5 * max(np.abs(ref["grad"]).max(), 1e-30))
    if mk == "off":
        assert ref["loss"] == 0.0 and ref["den"] == 1.0 and not ref["grad"].any()


@pytest.mark.parametrize("name,term", MS_PARAMS, ids=MS_IDS)
def test_torch_route_fp64_reproduces_the_multiscale_oracle(name, term):
    from opticalflow_amd import losses
    c = SC.MS_CASES[name]
    preds, img, gt, mask, lp, ls = SC.ms_inputs(name, term)
    ps = [p.double().requires_grad_(True) for p in preds]
    w = None if c.w is None else list(c.w)
    got = losses.supervised_multiscale_loss(ps[0] if c.one_tensor else ps, img.double(), gt.double(), mask.double(), w=w,
                                            lambda_photo=lp, lambda_smooth=ls, route="torch")
    grads = torch.autograd.grad(got, ps)
    ref = SC.ms_oracle(name, term)
    np.testing.assert_allclose(got.item(), ref["total"], rtol=1e-6)
    np.testing.assert_allclose(sum(w_ * l for w_, l in zip(SC.level_weights(name), ref["levels"])), ref["total"], rtol=1e-12)
    for g, gr in zip(grads, ref["grads"]):
        np.testing.assert_allclose(g.numpy(), gr, rtol=0, atol=1e-5 * np.abs(gr).max())
    if term in ("photo", "smooth"):
        assert (ref["den_c"] == 1.0).all()                                # no pixel is valid: the clamp
    if term == "photo":
        np.testing.assert_allclose(ref["den_p"], [np.float32(0.4).astype(np.float64) * c.B * h * w + 1e-8 for h, w in c.levels], rtol=1e-12)


NEW_RATIOS = sorted({(a, b) for c in SC.FLOW_CASES.values() for a, b in ((c.h, c.H), (c.w, c.W))}
                    | {(a, b) for c in SC.MS_CASES.values() for h, w in c.levels for a, b in ((c.H, h), (c.W, w))})


@pytest.mark.parametrize("n_in,n_out", NEW_RATIOS)
def test_index_arithmetic_matches_torch_interpolate_at_the_new_ratios(n_in, n_out):
    """O.linear_taps against torch's align_corners=False resize of one-hot rows (the bound of test_supervised_loss_cpu's
    test_bilinear_taps_match_torch_interpolate), O.nearest_index against torch's nearest resize where a mask is downsampled."""
    eye = torch.eye(n_in, dtype=torch.float32).reshape(n_in, 1, 1, n_in)
    got = F.interpolate(eye, size=(1, n_out), mode="bilinear", align_corners=False)[:, 0, 0, :].T.numpy()
    A = O.interp_matrix(n_in, n_out)
    assert np.array_equal(got > 1e-4, A > 1e-4)
    np.testing.assert_allclose(got, A, rtol=0, atol=2 * 2.0 ** -23 * n_in)
    i0, i1, l0, l1 = O.linear_taps(n_in, n_out)
    assert i0.min() >= 0 and i1.max() <= n_in - 1 and np.all(i1 - i0 <= 1)
    if n_in >= n_out:
        x = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, 1, n_in)
        near = F.interpolate(x, size=(1, n_out), mode="nearest")[0, 0, 0].numpy().astype(np.int64)
        np.testing.assert_array_equal(near, O.nearest_index(n_in, n_out))


# ---------------------------------------------------------------- every comparator passes on the oracle and can fail
def _copy_flow(ref):
    return {"loss": ref["loss"], "den": ref["den"], "grad": ref["grad"].copy()}


def _copy_ms(ref):
    return {"total": ref["total"], "levels": ref["levels"].copy(), "den_c": ref["den_c"].copy(), "den_p": ref["den_p"].copy(),
            "grads": [g.copy() for g in ref["grads"]]}


@pytest.mark.parametrize("name,rule,eps,mk", [p for p in FLOW_PARAMS if p[3] != "off"], ids=[i for i in FLOW_IDS if not i.endswith("off")])
def test_flow_comparator_can_fail(name, rule, eps, mk):
    ref = SC.flow_oracle(name, rule, eps, mk)
    assert set(SC.check_flow(_copy_flow(ref), ref).values()) == {0.0}
    bad = _copy_flow(ref)
    bad["grad"][:, :, -1, :] = 0.0                                        # the last row zeroed
    with pytest.raises(AssertionError):
        SC.check_flow(bad, ref)
    bad = _copy_flow(ref)
    bad["grad"][:, :, :, -1] = 0.0
    with pytest.raises(AssertionError):
        SC.check_flow(bad, ref)
    bad = _copy_flow(ref)
    bad["grad"] *= 1.0 + 2e-4                                             # an upstream gradient off by two bounds
    with pytest.raises(AssertionError):
        SC.check_flow(bad, ref)
    ok = _copy_flow(ref)
    ok["grad"] *= 1.0 + 0.5e-4
    assert 0.49 < SC.check_flow(ok, ref)["grad"] < 0.51
    assert SC.check_flow({"loss": ref["loss"], "den": ref["den"], "grad": 3.5 * ref["grad"]}, ref, scale=3.5)["grad"] < 1e-9
    with pytest.raises(AssertionError):
        SC.check_flow(_copy_flow(ref), ref, scale=3.5)                    # gout ignored
    for key in ("loss", "den"):
        bad = _copy_flow(ref)
        bad[key] = ref[key] * (1.0 + 2e-5) + 2e-9
        with pytest.raises(AssertionError):
            SC.check_flow(bad, ref)
        bad[key] = SC.NAN
        with pytest.raises(AssertionError):
            SC.check_flow(bad, ref)
    bad = _copy_flow(ref)
    bad["grad"][0, 0, 0, 0] = SC.NAN
    with pytest.raises(AssertionError):
        SC.check_flow(bad, ref)


def test_exact_zero_comparator_can_fail():
    ref = SC.flow_oracle("tail-1", "threshold", 1e-3, "off")
    assert SC.check_flow(_copy_flow(ref), ref)["grad"] == 0.0
    for v in (1e-30, SC.NAN):
        bad = _copy_flow(ref)
        bad["grad"][1, 1, 4, 16] = v
        with pytest.raises(AssertionError):
            SC.check_flow(bad, ref)


@pytest.mark.parametrize("name,term", MS_PARAMS, ids=MS_IDS)
def test_multiscale_comparator_can_fail(name, term):
    ref = SC.ms_oracle(name, term)
    L = len(ref["grads"])
    assert set(SC.check_ms(_copy_ms(ref), ref).values()) == {0.0}
    for l in range(L):
        for sl in ((Ellipsis, -1, slice(None)), (Ellipsis, -1)):
            bad = _copy_ms(ref)
            bad["grads"][l][sl] = 0.0                                     # the last row / column of one level zeroed
            with pytest.raises(AssertionError):
                SC.check_ms(bad, ref)
        bad = _copy_ms(ref)
        bad["grads"][l] *= 1.0 + 2e-4
        with pytest.raises(AssertionError):
            SC.check_ms(bad, ref)
        keys = ("levels", "den_c") + (("den_p",) if ref["photo_on"] else ())
        for key in keys:
            bad = _copy_ms(ref)
            bad[key][l] = ref[key][l] * (1.0 + 2e-5) + 2e-9
            with pytest.raises(AssertionError):
                SC.check_ms(bad, ref)
    bad = _copy_ms(ref)
    bad["total"] = ref["total"] * (1.0 - 2e-5) - 2e-9
    with pytest.raises(AssertionError):
        SC.check_ms(bad, ref)
    with pytest.raises(AssertionError):
        SC.check_ms(_copy_ms(ref), ref, scale=3.5)
    with pytest.raises(AssertionError):
        SC.check_ms(dict(_copy_ms(ref), grads=[g.copy() for g in ref["grads"][:-1]]), ref)     # a level missing


@pytest.mark.parametrize("term", list(SC.TERMS))
def test_swapped_levels_of_one_size_fail(term):
    """ms-twins: two 6 x 10 levels.  A result whose levels are exchanged has the right shapes and must not pass."""
    ref = SC.ms_oracle("ms-twins", term)
    bad = _copy_ms(ref)
    bad["grads"] = bad["grads"][::-1]
    with pytest.raises(AssertionError):
        SC.check_ms(bad, ref)
    bad = _copy_ms(ref)
    bad["levels"] = bad["levels"][::-1].copy()
    with pytest.raises(AssertionError):
        SC.check_ms(bad, ref)


def test_ignored_strides_fail():
    """What a kernel that took the dense batch stride would compute from the strided operands of the GPU test: it reads the NaN
    gap (inside the allocation), and the comparators do not let NaN pass."""
    pred, gt = (t.numpy() for t in SC.flow_inputs("tail-1"))
    ref = SC.flow_oracle("tail-1")
    buf, view = SC.strided_np(pred)
    assert np.array_equal(view, pred) and np.isnan(buf[:, pred[0].size:]).all() and view.base is not None
    wrong = SC.read_ignoring_stride(buf, pred.shape)
    assert np.array_equal(wrong[0], pred[0]) and np.isnan(wrong[1]).any()
    loss, grad = O.flow_loss(wrong, gt)
    with pytest.raises(AssertionError):
        SC.check_flow({"loss": loss, "den": ref["den"], "grad": ref["grad"]}, ref)
    with pytest.raises(AssertionError):
        SC.check_flow({"loss": ref["loss"], "den": ref["den"], "grad": grad}, ref)
    preds, img, gt, mask, lp, ls = (SC.ms_inputs("ms-ragged", "all"))
    mref = SC.ms_oracle("ms-ragged", "all")
    for l in range(len(preds)):
        ps = [p.numpy() for p in preds]
        b, _ = SC.strided_np(ps[l])
        ps[l] = SC.read_ignoring_stride(b, ps[l].shape)
        with np.errstate(invalid="ignore"):
            total, grads = O.multiscale_loss(ps, img.numpy(), gt.numpy(), mask.numpy(), list(SC.level_weights("ms-ragged")), lp, ls)
        res = _copy_ms(mref)
        res["total"] = total
        with pytest.raises(AssertionError):
            SC.check_ms(res, mref)
        res = _copy_ms(mref)
        res["grads"] = grads
        with pytest.raises(AssertionError):
            SC.check_ms(res, mref)


def test_oracle_results_are_shared_and_read_only():
    a, b = SC.flow_oracle("tail-1"), SC.flow_oracle("tail-1", "threshold", 1e-3, None)
    assert a is b and not a["grad"].flags.writeable
    m = SC.ms_oracle("ms-1", "all")
    assert m is SC.ms_oracle("ms-1", "all", "rough") and not m["grads"][0].flags.writeable
    p, _ = SC.flow_inputs("tail-1")
    p.zero_()
    assert SC.flow_inputs("tail-1")[0].abs().max() > 0
