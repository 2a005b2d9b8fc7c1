"""GPU checks of the epipolar mask and soft Sampson penalty (csrc/pwc_epipolar.hip) against the reference's own results (g9
fixture) and the float64 NumPy oracle of tests/epipolar_oracle.py."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import epipolar_oracle as O
from test_epipolar_cpu import CASES, case_flow, case_mask

pytestmark = pytest.mark.gpu


def _dev_case(z, name, dev):
    fl = case_flow(z, name)
    m = case_mask(z, name)
    ft = torch.from_numpy(fl).unsqueeze(0).to(dev)
    mt = None if m is None else torch.from_numpy(m).unsqueeze(0).to(dev)
    return fl, ft, mt


@pytest.mark.parametrize("name", CASES)
def test_ransac_matches_reference_g9(gpu_device, name):
    from opticalflow_amd import epipolar
    z = load_golden("g9_epipolar.npz")
    stride = int(z[name + "/cfg"][2])
    _, ft, mt = _dev_case(z, name, gpu_device)
    for tag, iters, thresh in (("fit", 2000, 0.5), ("soft", 1000, 1.0)):
        F, ok, best, counts, N = epipolar.ransac_fundamental_ex(ft, stride, thresh, iters, 0, mt)
        assert N[0] == int(z[name + "/cfg"][7])
        assert bool(ok[0]) == bool(z[name + "/%s_ok" % tag]), (name, tag)
        if N[0] < 8:
            assert int(best[0]) == -1 and not counts.any()
            continue
        c, cr = counts[0].cpu().numpy(), z[name + "/%s_counts" % tag].astype(np.int64)
        assert np.mean(c == cr) >= 0.999, (name, tag, np.flatnonzero(c != cr)[:10])
        assert int(best[0]) == int(z[name + "/%s_best" % tag])
        if bool(ok[0]):
            Fr = z[name + "/%s_F" % tag]
            rel = np.linalg.norm(F[0].cpu().numpy() - Fr) / np.linalg.norm(Fr)
            assert rel <= 1e-8, (name, tag, rel)


@pytest.mark.parametrize("name", CASES)
def test_mask_matches_reference_g9(gpu_device, name):
    from opticalflow_amd import epipolar, ops
    z = load_golden("g9_epipolar.npz")
    H, W, stride = (int(v) for v in z[name + "/cfg"][:3])
    tau, kr, mk = (float(v) for v in z[name + "/cfg"][4:7])
    _, ft, mt = _dev_case(z, name, gpu_device)
    F, ok = epipolar.ransac_fundamental(ft, stride, 0.5, 2000, 0, mt)
    d = torch.empty((1, H, W), dtype=torch.float64, device=gpu_device)
    mask, thr = ops.epipolar_mask(ft, F.view(1, 9), ok, tau, kr, mk, dist_out=d)
    mask2 = epipolar.build_epipolar_mask_from_flow(ft, tau, stride, mt, kr, mk)
    assert torch.equal(mask, mask2)
    m = mask[0, 0].cpu().numpy()
    ref = np.unpackbits(z[name + "/mask"])[:H * W].astype(bool).reshape(H, W)
    t = float(thr[0])
    if not bool(ok[0]) or np.isnan(float(z[name + "/thr"])):
        assert m.all() and np.isnan(t)
        return
    # the threshold is numpy's quantile of the kernel's own distances, bit for bit
    dn = d[0].cpu().numpy()
    fin = np.isfinite(dn)
    want = float(tau)
    if 0 < kr < 1:
        want = min(want, float(np.quantile(dn[fin], kr)))
    if 0 < mk < 1 and (fin & (dn <= want)).mean() < mk:
        want = min(float(tau), float(np.quantile(dn[fin], mk)))
    assert t == want, (name, t, want)
    assert np.array_equal(m, fin & (dn <= t))
    # against the reference: few mismatches, each at the threshold
    bad = m != ref
    assert bad.sum() <= 1e-4 * H * W, (name, int(bad.sum()))
    dref = O.distance_map(np.ascontiguousarray(case_flow(z, name).transpose(1, 2, 0)), z[name + "/fit_F"])
    assert np.all(np.abs(dref[bad] - float(z[name + "/thr"])) <= 1e-6 * float(z[name + "/thr"])), name
    np.testing.assert_allclose(t, float(z[name + "/thr"]), rtol=1e-6)


def test_sampson_distance_matches_oracle(gpu_device):
    from opticalflow_amd import epipolar
    z = load_golden("g9_epipolar.npz")
    fl, ft, _ = _dev_case(z, "nan", gpu_device)
    Fr = z["nan/fit_F"]
    d = epipolar.sampson_distance(ft, Fr)[0].cpu().numpy()
    dr = O.distance_map(np.ascontiguousarray(fl.transpose(1, 2, 0)), Fr)
    assert np.array_equal(np.isfinite(d), np.isfinite(dr))
    f = np.isfinite(dr)
    # x2^T F x1 cancels (d is tiny next to its terms): the bound follows sqrt(d), the quantity that rounds in fp64
    assert np.all(np.abs(np.sqrt(d[f]) - np.sqrt(dr[f])) <= 1e-9 * np.sqrt(dr[f]).max())


def test_batched_equals_per_sample_and_reproducible(gpu_device):
    from opticalflow_amd import epipolar
    z = load_golden("g9_epipolar.npz")
    flows = [case_flow(z, n) for n in ("small", "nan", "minkeep")]
    fb = torch.from_numpy(np.stack(flows)).to(gpu_device)
    nanfill = torch.from_numpy(np.stack(flows)).to(gpu_device)
    F, ok, best, counts, N = epipolar.ransac_fundamental_ex(fb, 4)
    mb, tb = epipolar.build_epipolar_mask_from_flow(fb, 1.0, 4, return_thr=True)
    mb2, tb2 = epipolar.build_epipolar_mask_from_flow(nanfill.clone(), 1.0, 4, return_thr=True)
    assert torch.equal(mb, mb2) and torch.equal(tb.isnan(), tb2.isnan()) and torch.equal(tb.nan_to_num(), tb2.nan_to_num())
    for b in range(3):
        F1, ok1, best1, c1, N1 = epipolar.ransac_fundamental_ex(fb[b:b + 1], 4)
        assert N1[0] == N[b] and torch.equal(F1[0], F[b]) and torch.equal(c1[0], counts[b]) and int(best1[0]) == int(best[b])
        m1, t1 = epipolar.build_epipolar_mask_from_flow(fb[b:b + 1], 1.0, 4, return_thr=True)
        assert torch.equal(m1[0], mb[b]) and float(t1[0]) == float(tb[b])
    # soft loss and its gradient: two calls bit-identical
    l1, g1 = _loss_and_grad(fb, F[0], mb, "huber", 1.0, 0.1, ok[0])
    l2, g2 = _loss_and_grad(fb, F[0], mb, "huber", 1.0, 0.1, ok[0])
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_failure_paths(gpu_device):
    from opticalflow_amd import epipolar
    H, W = 32, 48
    f = torch.zeros(2, 2, H, W, device=gpu_device)
    f[1] = float("nan")                      # no finite endpoint: N = 0
    img_mask = torch.zeros(2, H, W, dtype=torch.bool, device=gpu_device)
    img_mask[:, 0, :12] = True               # 3 grid points at stride 4
    F, ok = epipolar.ransac_fundamental(f, 4, mask=img_mask)
    assert not ok.any() and not F.any()
    m, thr = epipolar.build_epipolar_mask_from_flow(f, 1.0, 4, img_mask, return_thr=True)
    assert m.all() and thr.isnan().all()
    l, g = _loss_and_grad(f[:1], torch.eye(3, dtype=torch.float64), None, "huber", 1.0, 0.1, ok[0])
    assert float(l) == 0.0 and not g.any()
    l, g = _loss_and_grad(f[:1], torch.eye(3, dtype=torch.float64), torch.zeros(1, 1, H, W, device=gpu_device), "l1", 1.0, 0.1, None)
    assert float(l) == 0.0 and not g.any()


def _loss_and_grad(flow, F, mask, robust, delta, weight, ok):
    from opticalflow_amd import epipolar
    f = flow.detach().clone().requires_grad_(True)
    loss = epipolar.epipolar_sampson_loss(f, F, valid_mask=mask, robust=robust, delta=delta, weight=weight, ok=ok)
    (3.0 * loss).backward()
    return loss.detach(), f.grad


@pytest.mark.parametrize("robust", ["huber", "l1", "mean"])
@pytest.mark.parametrize("mask_kind", ["none", "bool", "float", "uint8", "perF"])
def test_soft_loss_matches_oracle(gpu_device, robust, mask_kind):
    z = load_golden("g9_epipolar.npz")
    flows = np.stack([case_flow(z, n) for n in ("small", "minkeep")])
    B, _, H, W = flows.shape
    rng = np.random.default_rng(5)
    mval = rng.uniform(0, 1, (B, 1, H, W)).astype(np.float32)
    mask, mref = None, None
    if mask_kind in ("bool", "perF"):
        mask = torch.from_numpy(mval > 0.5).to(gpu_device)
    elif mask_kind == "float":
        mask = torch.from_numpy(mval).to(gpu_device)
    elif mask_kind == "uint8":
        mask = torch.from_numpy((mval > 0.3).astype(np.uint8)).to(gpu_device)
    if mask is not None:
        mref = mask.cpu().numpy().astype(np.float64) if mask_kind == "float" else (mask.cpu().numpy() != 0).astype(np.float64)
    if mask_kind == "perF":
        F = np.stack([z["small/soft_F"], z["minkeep/soft_F"]])
        Ft, ok, okn = torch.from_numpy(F).to(gpu_device), torch.tensor([True, False], device=gpu_device), np.array([True, False])
    else:
        F = z["small/soft_F"]
        Ft, ok, okn = F, None, None
    delta = 1e-3 if robust == "huber" else 1.0       # both Huber branches are taken
    ft = torch.from_numpy(flows).to(gpu_device)
    loss, g = _loss_and_grad(ft, Ft, mask, robust, delta, 0.1, ok)
    lr, gr = O.soft_loss(flows, F.astype(np.float32), mref, robust, delta, 0.1, okn)
    gr = 3.0 * gr
    assert abs(float(loss) - lr) <= 1e-6 * abs(lr), (float(loss), lr)
    assert np.abs(g.cpu().double().numpy() - gr).max() <= 1e-6 * np.abs(gr).max()
