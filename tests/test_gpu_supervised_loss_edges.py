"""GPU checks of csrc/pwc_sup_loss.hip off the aligned training sizes of tests/test_gpu_supervised_loss.py: the ragged cases of
tests/supervised_loss_cases.py against the fp64 oracle (tests/supervised_loss_oracle.py), through the comparators that
tests/test_supervised_loss_cases_cpu.py shows can fail.  What that file cannot see and this one does: an upstream gradient other
than 1 (3.5 against the oracle, 65536 and 2^-10 bit for bit against 1, autograd, a GradScaler round trip); batch-strided
operands as the training scripts pass them; each term of the multiscale gradient alone; the flattened multi-level grid at 1024
and 1025 pixels, with a full-resolution level amid smaller ones, 8 levels, one level, two levels of one size; first_user and the
separable gather at ratios just under 1, 65, h = H with w < W and its transpose, and the 2 x 2 extremes.  Every bound is one the
project already asserts for the same quantity (rtol 1e-5 / atol 1e-9 on losses and denominators, 1e-4 max|g| per level on
gradients); no element is left out of any comparison; each test prints the worst error / bound it saw (`pytest -s`).

Two things differ from a literal reading of the plan.  A flow that puts every photometric sample outside the level does not give a
zero photometric loss: the padding is zeros, so the loss is lambda_photo times the masked mean of |im1_s|; what is exactly zero is
the gradient, and both are asserted (the loss against the oracle).  And the flow-loss backward is also run under rule "raw" with
a fractional mask, which no module reaches but ops.sup_flow_loss_backward offers.  Three cases were added to the planned table
(ms-chunks-b2, ms-8w, ms-twins: see supervised_loss_cases.py).  No test here exposed a bug in the kernels.

Worst error / bound seen on an MI355X (2026-10-20, kernels as of 3bf6da8; none above a quarter of its bound, the largest 0.021):
  flow loss, "threshold" / "raw"            6.8e-3 (chunk-plus-1, binary mask) / 5.7e-3 (near-1, fractional mask)
  flow denominator                          0 under "threshold" (a count), 4.9e-3 under "raw" (coarse-2x2)
  flow gradient, "threshold" / "raw"        1.2e-2 / 1.2e-2 (coarse-2x2 both)                 bound 1e-4 max|g|
  multiscale total and level losses         charb 6.5e-3 (ms-ragged), photo 8.5e-3 (ms-ragged), smooth 8.2e-3 (ms-twins),
                                            all 5.4e-3 (ms-8)                                 bound rtol 1e-5 + atol 1e-9
  multiscale denominators                   Charbonnier: equal (a count); photometric 4.9e-3 (ms-8w, all)
  multiscale gradient per term setting      charb 5.6e-3 (ms-chunks-b2), photo 2.1e-2 (ms-chunks), smooth 1.7e-3 (ms-chunks-b2),
                                            all 7.4e-3 (ms-chunks-b2)                         bound 1e-4 max|g| per level
  upstream gradient 3.5 vs 3.5 x oracle     2.1e-2 (ms-chunks, photo): the figures of gout = 1; 65536 and 2^-10 against 1: equal
                                            bits in every case; (3.5 * loss).backward() equals ops.*_backward(gout = 3.5) bit for
                                            bit; the GradScaler(65536) round trip stayed within one float32 rounding
  strided vs dense                          equal bits in all three cases; against the oracle 5.7e-3 (loss), 5.6e-3 (gradient)
  torch fallback (9 levels, h = 1, a level larger than gt, a flow one row high)  loss 1.0e-2, gradient 3.3e-3
  exact zeros ("off" masks, constant predictions, out-of-level flows), equal bits across mask dtypes / shapes, two calls, and
  autograd against ops.*_backward: all held.  The 158 tests take under 4 s.

That the file bites was shown on scratch builds of the kernel source with one change each to arithmetic or in-bounds indexing
(never committed); tests failing here (of 158) / in test_gpu_supervised_loss.py (of 22):
  (i)   gout[0] replaced by 1 in flow_cols_kernel and ms_bwd_kernel         53 (the three upstream-gradient tests) / none
  (ii)  every batch stride replaced by the dense one                         3 (the three batch-strided tests) / none
  (iii) level_of gives the previous level at an exact blk0 boundary          57 (every multiscale case with two or more levels) / 8
  (iv)  first_user's estimate two late, no backward walk                     75 (every flow backward but "off" masks) / 8
  (v)   gsx divided by w instead of w - 1                                    36 (every "smooth" and "all" setting) / 3
  (vi)  the photometric gradient's `* m` dropped                             36 (every "photo" and "all" setting) / 2
  (vii) weight w[L-1] for every level past the fourth                        8 (ms-8w, the case with eight distinct weights) / none
No mutant survives this file; (i), (ii) and (vii) survive the other one.  With the default five weights (vii) changes nothing,
since levels 5 to 7 share w[-1] there: ms-8 alone would not have seen it, which is why ms-8w exists.
"""
import warnings

import numpy as np
import pytest
import torch

import supervised_loss_cases as SC
import supervised_loss_oracle as O

pytestmark = pytest.mark.gpu

NAN = SC.NAN
FLOW_PARAMS = [(n, r, e, m) for n in SC.FLOW_CASES for r, e, m in SC.FLOW_SETTINGS]
FLOW_IDS = ["%s-%s-%s" % (n, r, m) for n, r, _, m in FLOW_PARAMS]
MS_PARAMS = [(n, t) for n in SC.MS_CASES for t in SC.TERMS]
MS_IDS = ["%s-%s" % p for p in MS_PARAMS]
POW2 = (65536.0, 2.0 ** -10)


def _report(what, worst):
    print("[sup-edges] %s: worst error / bound %s" % (what, ", ".join("%s %.3e" % kv for kv in worst.items())))


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _route(loss):
    """'hip' when the 0-dim loss is an element of one of the fused autograd Functions' outputs, else 'torch' (as
    test_gpu_supervised_loss._route)."""
    fn = loss.grad_fn
    nxt = fn.next_functions[0][0] if fn is not None and fn.next_functions else None
    return "hip" if nxt is not None and type(nxt).__name__ in ("FlowLossFunctionBackward", "MultiscaleLossFunctionBackward") else "torch"


def _strided(t, dev, extra=37):
    """Device view of t [B,...] (float32) whose batch stride is larger than a sample; the gap is NaN, so a kernel that ignores
    the stride shows (as test_gpu_proxy_loss_edges._strided).  A dense batch stride still reads inside the buffer."""
    n = t[0].numel()
    buf = torch.full((t.shape[0], n + extra), NAN, device=dev)
    v = buf[:, :n].view(t.shape)
    v.copy_(t)
    assert v.stride(0) == n + extra
    return buf, v


def _gout(g, n, dev):
    """upstream gradient of an [n] output: g for the loss, 0 for the entries that carry no gradient (as autograd hands it over)"""
    t = torch.zeros(n, dtype=torch.float32, device=dev)
    t[0] = g
    return t


def _run_flow(pred, gt, mask, rule, eps, gout=1.0):
    """({"loss", "den", "grad"} as NumPy, the bits of all of it) of one forward and one backward"""
    from opticalflow_amd import ops
    out = ops.sup_flow_loss(pred, gt, mask, eps, rule)
    g = ops.sup_flow_loss_backward(pred, gt, mask, out, _gout(gout, 2, gt.device), eps, rule)
    assert out.dtype == torch.float32 and tuple(out.shape) == (2,)
    assert g.dtype == torch.float32 and tuple(g.shape) == tuple(pred.shape) and g.is_contiguous()
    o = out.double().cpu().numpy()
    return {"loss": o[0], "den": o[1], "grad": g.cpu().numpy()}, _bits(out) + _bits(g)


def _run_ms(preds, gt, mask, img, weights, lp, ls, gout=1.0):
    """({"total", "levels", "den_c", "den_p", "grads"} as NumPy, the bits of all of it) of one forward and one backward"""
    from opticalflow_amd import ops
    L = len(preds)
    out = ops.sup_multiscale_loss(preds, gt, mask, img, weights, lp, ls)
    gs = ops.sup_multiscale_loss_backward(preds, gt, mask, img, weights, out, _gout(gout, 1 + 3 * L, gt.device), lp, ls)
    assert out.dtype == torch.float32 and tuple(out.shape) == (1 + 3 * L,) and len(gs) == L
    assert all(g.dtype == torch.float32 and tuple(g.shape) == tuple(p.shape) and g.is_contiguous() for g, p in zip(gs, preds))
    o = out.double().cpu().numpy()
    res = {"total": o[0], "levels": o[1:1 + L], "den_c": o[1 + L:1 + 2 * L], "den_p": o[1 + 2 * L:], "grads": [g.cpu().numpy() for g in gs]}
    return res, _bits(out) + b"".join(_bits(g) for g in gs)


def _flow_dev(name, mk, dev):
    pred, gt = SC.flow_inputs(name)
    m = SC.flow_mask(name, mk)
    return pred.to(dev), gt.to(dev), None if m is None else m.to(dev)


def _ms_dev(name, term, dev, kind="rough"):
    preds, img, gt, mask, lp, ls = SC.ms_inputs(name, term, kind)
    return [p.to(dev) for p in preds], img.to(dev), gt.to(dev), mask.to(dev), lp, ls


def _zero_bits(a):
    return a.tobytes() == bytes(a.nbytes)


# ---------------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("name,rule,eps,mk", FLOW_PARAMS, ids=FLOW_IDS)
def test_flow_loss_matches_oracle(gpu_device, name, rule, eps, mk):
    """loss, denominator and gradient of every flow case and setting; two calls give the same bits"""
    pred, gt, mask = _flow_dev(name, mk, gpu_device)
    res, bits = _run_flow(pred, gt, mask, rule, eps)
    _report("%s %s mask %s" % (name, rule, mk), SC.check_flow(res, SC.flow_oracle(name, rule, eps, mk), name))
    if mk == "off":
        assert res["loss"] == 0.0 and res["den"] == 1.0 and _zero_bits(res["grad"])      # the clamp; zeros, not small numbers
    assert _run_flow(pred, gt, mask, rule, eps)[1] == bits


@pytest.mark.parametrize("name,term", MS_PARAMS, ids=MS_IDS)
def test_multiscale_matches_oracle(gpu_device, name, term):
    """total, level losses, both denominators of every level and every level's gradient, for each term alone and for all of
    them; two calls give the same bits"""
    preds, img, gt, mask, lp, ls = _ms_dev(name, term, gpu_device)
    w = SC.level_weights(name)
    res, bits = _run_ms(preds, gt, mask, img, w, lp, ls)
    _report("%s %s" % (name, term), SC.check_ms(res, SC.ms_oracle(name, term), name))
    if term in ("photo", "smooth"):
        assert (res["den_c"] == 1.0).all()                                  # no pixel is valid: the clamp
    assert _run_ms(preds, gt, mask, img, w, lp, ls)[1] == bits


@pytest.mark.parametrize("name,term,kind", SC.ZERO_KINDS, ids=["%s-%s-%s" % z for z in SC.ZERO_KINDS])
def test_multiscale_exact_zeros(gpu_device, name, term, kind):
    """A constant prediction under the smoothness term alone: loss 0 and an all-zero gradient.  A flow larger than the level
    under the photometric term alone: every tap is padding, so the gradient is all zero and the loss is lambda_photo times the
    masked mean of |im1_s| (zero padding leaves the residual of a black im2, not 0; the oracle's value)."""
    preds, img, gt, mask, lp, ls = _ms_dev(name, term, gpu_device, kind)
    res, _ = _run_ms(preds, gt, mask, img, SC.level_weights(name), lp, ls)
    ref = SC.ms_oracle(name, term, kind)
    _report("%s %s %s" % (name, term, kind), SC.check_ms(res, ref, name))
    assert all(not g.any() for g in ref["grads"]) and all(_zero_bits(g) for g in res["grads"])
    if kind == "const":
        assert res["total"] == 0.0 and not res["levels"].any()


# ---------------------------------------------------------------------------------------------------------------- upstream gradient
def _scaled_bits(g, k):
    """float32 array times a power of two, as bits (exact: no entry is near the subnormal range or the overflow threshold)"""
    a = np.asarray(g, np.float32)
    assert a.size == 0 or not a.any() or (np.abs(a[a != 0]).min() > 1e-25 and np.abs(a).max() < 1e25)
    return (a * np.float32(k)).tobytes()


@pytest.mark.parametrize("name,rule,eps,mk", [p for p in FLOW_PARAMS if p[3] in ("binary", "frac")],
                         ids=[i for i in FLOW_IDS if i.endswith(("binary", "frac"))])
def test_flow_upstream_gradient(gpu_device, name, rule, eps, mk):
    """gout = 3.5 against 3.5 x the oracle; gout = 65536 and 2^-10 against gout = 1 times that power of two, bit for bit: the
    column pass forms gs = gout / den and gs * (sum * scale), and every one of these scales exactly"""
    pred, gt, mask = _flow_dev(name, mk, gpu_device)
    one, _ = _run_flow(pred, gt, mask, rule, eps)
    res, _ = _run_flow(pred, gt, mask, rule, eps, 3.5)
    _report("%s %s gout 3.5" % (name, rule), SC.check_flow(res, SC.flow_oracle(name, rule, eps, mk), name, scale=3.5))
    for k in POW2:
        got, _ = _run_flow(pred, gt, mask, rule, eps, k)
        assert got["grad"].tobytes() == _scaled_bits(one["grad"], k), (name, k)


@pytest.mark.parametrize("name,term", MS_PARAMS, ids=MS_IDS)
def test_multiscale_upstream_gradient(gpu_device, name, term):
    """as above for ms_bwd_kernel: g = gout * w_l, then g / den, g * lambda / den, g * lambda / count times values that do not
    depend on gout, and sums of such products: all exact under a power of two"""
    preds, img, gt, mask, lp, ls = _ms_dev(name, term, gpu_device)
    w = SC.level_weights(name)
    one, _ = _run_ms(preds, gt, mask, img, w, lp, ls)
    res, _ = _run_ms(preds, gt, mask, img, w, lp, ls, 3.5)
    _report("%s %s gout 3.5" % (name, term), SC.check_ms(res, SC.ms_oracle(name, term), name, scale=3.5))
    for k in POW2:
        got, _ = _run_ms(preds, gt, mask, img, w, lp, ls, k)
        for l, (a, b) in enumerate(zip(got["grads"], one["grads"])):
            assert a.tobytes() == _scaled_bits(b, k), (name, term, k, l)


def _within_one_rounding(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)).astype(np.float64)))


def test_upstream_gradient_through_autograd_and_grad_scaler(gpu_device):
    """(3.5 * loss).backward() through the modules against 3.5 x the oracle and against ops.*_backward with gout = 3.5 bit for
    bit; a torch.amp.GradScaler(init_scale=65536) round trip gives the unscaled run's gradient within one float32 rounding"""
    from opticalflow_amd import losses
    pred, gt, mask = _flow_dev("tail-1", "binary", gpu_device)
    preds, img, gt2, mask2, lp, ls = _ms_dev("ms-ragged", "all", gpu_device)

    def flow_loss(p):
        return losses.MaskedCharbonnier()(p, gt, mask)

    def ms_loss(*ps):
        return losses.supervised_multiscale_loss(list(ps), img, gt2, mask2, lambda_photo=lp, lambda_smooth=ls)

    for tag, fn, leaves, direct, ref in (
            ("tail-1", flow_loss, [pred], lambda g: [_run_flow(pred, gt, mask, "threshold", 1e-3, g)[0]["grad"]],
             [SC.flow_oracle("tail-1", "threshold", 1e-3, "binary")["grad"]]),
            ("ms-ragged all", ms_loss, preds, lambda g: _run_ms(preds, gt2, mask2, img, SC.level_weights("ms-ragged"), lp, ls, g)[0]["grads"],
             SC.ms_oracle("ms-ragged", "all")["grads"])):
        ps = [p.clone().requires_grad_(True) for p in leaves]
        loss = fn(*ps)
        assert _route(loss) == "hip"
        (3.5 * loss).backward()
        worst = max(SC.check_grad(p.grad.cpu().numpy(), gr, tag + " 3.5 x loss", 3.5) for p, gr in zip(ps, ref))
        _report("%s (3.5 * loss).backward()" % tag, {"grad": worst})
        for p, d in zip(ps, direct(3.5)):
            assert p.grad.cpu().numpy().tobytes() == d.tobytes()
        # GradScaler: scale(loss).backward(), unscale_(optimizer)
        plain = [p.clone().requires_grad_(True) for p in leaves]
        fn(*plain).backward()
        scaled = [p.clone().requires_grad_(True) for p in leaves]
        opt = torch.optim.SGD(scaled, lr=0.0)
        scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
        scaler.scale(fn(*scaled)).backward()
        for p, q in zip(scaled, plain):
            assert _within_one_rounding(p.grad.cpu().numpy(), 65536.0 * q.grad.cpu().numpy())
        scaler.unscale_(opt)
        assert scaler.get_scale() == 65536.0
        for p, q in zip(scaled, plain):
            assert _within_one_rounding(p.grad.cpu().numpy(), q.grad.cpu().numpy()) and bool(torch.isfinite(p.grad).all())


# ---------------------------------------------------------------------------------------------------------------- strides
def _batch9(img, gt, dev):
    """one [B,9,H,W] batch: images in channels 0-5, the GT in 6-7, NaN wherever an operand is not given and in channel 8"""
    B, _, H, W = gt.shape
    batch = torch.full((B, 9, H, W), NAN, device=dev)
    batch[:, 6:8] = gt.to(dev)
    if img is not None:
        batch[:, :6] = img.to(dev)
    return batch


def _mask2(mask, dev):
    mm = torch.full((mask.shape[0], 2) + tuple(mask.shape[-2:]), NAN, device=dev)
    mm[:, 0] = mask.to(dev)
    return mm


def test_batch_strided_flow_operands(gpu_device):
    """tail-1 as a training script passes it: gt = batch[:, 6:8] of a [B,9,H,W] tensor whose other channels are NaN, a
    prediction with NaN between its samples, the mask channel 0 of a [B,2,H,W] tensor whose channel 1 is NaN"""
    from opticalflow_amd import ops
    name = "tail-1"
    c = SC.FLOW_CASES[name]
    pred, gt = SC.flow_inputs(name)
    batch = _batch9(None, gt, gpu_device)
    gt_v = batch[:, 6:8]
    pbuf, pred_v = _strided(pred, gpu_device)
    for v, bs in ((gt_v, 9 * c.H * c.W), (pred_v, 2 * c.h * c.w + 37)):
        assert ops.densify(v) is v and v.stride(0) == bs and not v.is_contiguous()          # the kernel does receive the strides
    for rule, eps, mk in (("threshold", 1e-3, None), ("threshold", 1e-3, "binary"), ("raw", 0.0, "frac")):
        mm = None if mk is None else _mask2(SC.flow_mask(name, mk), gpu_device)
        m_v = None if mm is None else mm[:, 0]
        assert m_v is None or not m_v.is_contiguous()
        res_v, bits_v = _run_flow(pred_v, gt_v, m_v, rule, eps)
        res_d, bits_d = _run_flow(pred_v.contiguous(), gt_v.contiguous(), None if m_v is None else m_v.contiguous(), rule, eps)
        assert bits_v == bits_d, (rule, mk)
        _report("%s strided %s mask %s" % (name, rule, mk), SC.check_flow(res_v, SC.flow_oracle(name, rule, eps, mk), name))
        assert mm is None or bool(torch.isnan(mm[:, 1]).all())
    assert bool(torch.isnan(pbuf[:, pred[0].numel():]).all()) and bool(torch.isnan(batch[:, :6]).all()) and bool(torch.isnan(batch[:, 8]).all())


@pytest.mark.parametrize("name,term", (("ms-ragged", "all"), ("ms-chunks-b2", "charb")))
def test_batch_strided_multiscale_operands(gpu_device, name, term):
    """images = batch[:, :6] and gt = batch[:, 6:8] of one [B,9,H,W] tensor, every level a view with NaN between its samples,
    the mask one channel of a [B,2,H,W] tensor: the bits of the dense copies, and the oracle's result (B = 2: ms-chunks at the
    batch size at which a stride means something)"""
    from opticalflow_amd import ops
    c = SC.MS_CASES[name]
    assert c.B >= 2
    preds, img, gt, mask, lp, ls = SC.ms_inputs(name, term)
    batch = _batch9(img, gt, gpu_device)
    img_v, gt_v = batch[:, :6], batch[:, 6:8]
    bufs, views = zip(*[_strided(p, gpu_device) for p in preds])
    mm = _mask2(mask, gpu_device)
    m_v = mm[:, 0]
    for v, bs in [(img_v, 9 * c.H * c.W), (gt_v, 9 * c.H * c.W)] + [(v, 2 * h * w + 37) for v, (h, w) in zip(views, c.levels)]:
        assert ops.densify(v) is v and v.stride(0) == bs and not v.is_contiguous()
    assert not m_v.is_contiguous()
    w = SC.level_weights(name)
    res_v, bits_v = _run_ms(list(views), gt_v, m_v, img_v, w, lp, ls)
    res_d, bits_d = _run_ms([v.contiguous() for v in views], gt_v.contiguous(), m_v.contiguous(), img_v.contiguous(), w, lp, ls)
    assert bits_v == bits_d
    _report("%s %s strided" % (name, term), SC.check_ms(res_v, SC.ms_oracle(name, term), name))
    assert all(bool(torch.isnan(b[:, p[0].numel():]).all()) for b, p in zip(bufs, preds))
    assert bool(torch.isnan(batch[:, 8]).all()) and bool(torch.isnan(mm[:, 1]).all())


# ---------------------------------------------------------------------------------------------------------------- mask forms
def test_mask_forms_on_ragged_sizes(gpu_device):
    """bool / uint8 / float32 and [B,H,W] / [B,1,H,W]: one result, bit for bit, and it is the oracle's"""
    pred, gt, _ = _flow_dev("tail-1", None, gpu_device)
    first = None
    for tag, m in SC.mask_forms(SC.flow_mask("tail-1", "binary").numpy()):
        res, bits = _run_flow(pred, gt, m.to(gpu_device), "threshold", 1e-3)
        if first is None:
            first = bits
            _report("tail-1 mask forms", SC.check_flow(res, SC.flow_oracle("tail-1", "threshold", 1e-3, "binary"), "tail-1"))
        assert bits == first, tag
    preds, img, gt, mask, lp, ls = _ms_dev("ms-ragged", "charb", gpu_device)
    w = SC.level_weights("ms-ragged")
    first = None
    for tag, m in SC.mask_forms(mask.cpu().numpy()):
        res, bits = _run_ms(preds, gt, m.to(gpu_device), None, w, lp, ls)
        if first is None:
            first = bits
            _report("ms-ragged mask forms", SC.check_ms(res, SC.ms_oracle("ms-ragged", "charb"), "ms-ragged"))
        assert bits == first, tag


# ---------------------------------------------------------------------------------------------------------------- module routes
@pytest.mark.parametrize("name", ("min-2x2", "coarse-2x2"))
def test_flow_modules_take_the_hip_route(gpu_device, name):
    """MaskedCharbonnier and compute_epe take the kernels at the smallest and the coarsest geometry; autograd through the module
    is ops.sup_flow_loss_backward bit for bit"""
    from opticalflow_amd import losses
    pred, gt, mask = _flow_dev(name, "binary", gpu_device)
    p = pred.clone().requires_grad_(True)
    loss = losses.MaskedCharbonnier()(p, gt, mask)
    assert _route(loss) == "hip"
    loss.backward()
    res, _ = _run_flow(pred, gt, mask, "threshold", 1e-3)
    assert np.float32(res["loss"]).tobytes() == _bits(loss) and p.grad.cpu().numpy().tobytes() == res["grad"].tobytes()
    _report("%s module" % name, SC.check_flow({"loss": loss.item(), "den": res["den"], "grad": p.grad.cpu().numpy()},
                                              SC.flow_oracle(name, "threshold", 1e-3, "binary"), name))
    frac = SC.flow_mask(name, "frac").to(gpu_device)
    for m, mk in ((None, None), (frac, "frac")):
        with torch.no_grad():
            e = losses.compute_epe(pred, gt, m)
        assert _bits(e) == np.float32(_run_flow(pred, gt, m, "raw", 0.0)[0]["loss"]).tobytes()
        SC.check_loss(e.item(), SC.flow_oracle(name, "raw", 0.0, mk)["loss"], name + " compute_epe")


@pytest.mark.parametrize("name", ("ms-8", "ms-1"))
def test_multiscale_module_takes_the_hip_route(gpu_device, name):
    """supervised_multiscale_loss takes the kernels with 8 levels and the default five weights (w[-1] past their end) and with
    one tensor that is not a list; autograd through it is ops.sup_multiscale_loss_backward bit for bit"""
    from opticalflow_amd import losses
    c = SC.MS_CASES[name]
    preds, img, gt, mask, lp, ls = _ms_dev(name, "all", gpu_device)
    ps = [p.clone().requires_grad_(True) for p in preds]
    loss = losses.supervised_multiscale_loss(ps[0] if c.one_tensor else ps, img, gt, mask, lambda_photo=lp, lambda_smooth=ls)
    assert _route(loss) == "hip"
    loss.backward()
    res, _ = _run_ms(preds, gt, mask, img, SC.level_weights(name), lp, ls)
    assert np.float32(res["total"]).tobytes() == _bits(loss)
    assert all(p.grad.cpu().numpy().tobytes() == g.tobytes() for p, g in zip(ps, res["grads"]))
    _report("%s module" % name, SC.check_ms(dict(res, total=loss.item(), grads=[p.grad.cpu().numpy() for p in ps]),
                                            SC.ms_oracle(name, "all"), name))


def test_declined_geometries_fall_back_to_torch_silently(gpu_device):
    """A 9-level list, a level with h = 1 and a level larger than the ground truth are not the kernels' to take: the modules
    answer with the torch chain's value, without a warning, and it is the oracle's"""
    from opticalflow_amd import losses
    preds, img, gt, mask, _, _ = _ms_dev("ms-8", "charb", gpu_device)
    B, _, H, W = gt.shape
    gen = torch.Generator().manual_seed(77)
    extra = {"9 levels": preds + [preds[-1] * 0.5],
             "h = 1": [preds[1], torch.randn(B, 2, 1, 7, generator=gen).to(gpu_device)],
             "larger than gt": [preds[1], torch.randn(B, 2, H + 3, W + 5, generator=gen).to(gpu_device)]}
    for tag, lv in extra.items():
        ps = [p.clone().requires_grad_(True) for p in lv]
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            loss = losses.supervised_multiscale_loss(ps, None, gt, mask)
            want = losses.supervised_multiscale_loss_torch(lv, None, gt, mask)
        assert _route(loss) == "torch" and torch.equal(loss.detach(), want)
        loss.backward()
        lo, go = O.multiscale_loss([p.cpu().numpy() for p in lv], None, gt.cpu().numpy(), mask.cpu().numpy())
        worst = {"loss": SC.check_loss(loss.item(), lo, tag),
                 "grad": max(SC.check_grad(p.grad.cpu().numpy(), g, tag) for p, g in zip(ps, go))}
        _report("torch fallback, %s" % tag, worst)
    # the flow loss: a prediction one row high
    pred, gtf, m = _flow_dev("tail-1", "binary", gpu_device)
    p = pred[:, :, :1].clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loss = losses.MaskedCharbonnier()(p, gtf, m)
        e = losses.compute_epe(p.detach(), gtf, m)
    assert _route(loss) == "torch"
    assert torch.equal(loss.detach(), losses.masked_charbonnier_torch(p.detach(), gtf, m)) and torch.equal(e, losses.compute_epe_torch(p.detach(), gtf, m))
    lo, go = O.flow_loss(p.detach().cpu().numpy(), gtf.cpu().numpy(), m.cpu().numpy())
    loss.backward()
    _report("torch fallback, flow h = 1", {"loss": SC.check_loss(loss.item(), lo), "grad": SC.check_grad(p.grad.cpu().numpy(), go)})
