"""CPU checks of the no-ground-truth validation path (opticalflow_amd/validation.py, csrc/pwc_fb_metrics.hip): the float64 oracle
reproduces the reference's own float64 results (g11 fixture); the C ABI is declared, bound, exported and refuses bad arguments
before any launch; the torch route restates the scripts' chain; route selection, the flow_pair cache key and validate's averaging."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
import validation_oracle as VO

NAMES = ("pwc_fb_metrics_workspace_bytes", "pwc_fb_metrics")
CASES = ("smooth", "rough", "odd", "same", "zero", "const_neg", "clamp", "oob_only")


def _case(z, name):
    H, W = (int(v) for v in z[name + "/size"])
    f21 = z[name + "/flow21"] if name + "/flow21" in z.files else None
    return z[name + "/flow12"], f21, H, W


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_reference_fp64(name):
    z = load_golden("g11_validation.npz")
    f12, f21, H, W = _case(z, name)
    m = VO.metrics(f12, f21, H, W)
    print("%s: cycle oracle %.12g reference %s; oob count oracle %d reference %s, knife-edge %d"
          % (name, m["cycle"], z[name + "/cycle"], m["oob_count"], z[name + "/oob_count"], m["knife_edge"]))
    assert z[name + "/oob_count"][0] == z[name + "/oob_count"][1]           # the two scripts' functions agree
    # both sides are float64: rtol 1e-9.  Only const_neg, whose cycle is zero in exact arithmetic, gets an absolute floor instead:
    # the reference's normalise / unnormalise chain leaves residues of a few float64 ulps of the 7 px vectors there (1e-16)
    for ref in z[name + "/cycle"]:
        if name == "const_neg":
            assert abs(ref) <= 1e-12 and abs(m["cycle"]) <= 1e-12
        else:
            np.testing.assert_allclose(m["cycle"], ref, rtol=1e-9, atol=0)
    for ref in z[name + "/oob_count"]:
        assert abs(m["oob_count"] - int(ref)) <= m["knife_edge"]
    if name == "zero":
        assert m["cycle"] == 0.0 and m["oob_count"] == 0
    if name == "oob_only":
        assert f21 is None and m["cycle"] == 0.0


def test_symbols_declared_bound_exported():
    from opticalflow_amd import _lib
    text = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n + "(" in text and n in _lib.SIGNATURES and hasattr(lib, n)
    assert "pwc_fb_metrics.hip" in open(os.path.join(REPO, "opticalflow_amd", "csrc", "Makefile")).read()
    import opticalflow_amd
    from opticalflow_amd import ops, validation
    assert opticalflow_amd.validation is validation
    for n in ("fb_metrics", "fb_metrics_supported", "fb_metrics_workspace_bytes"):
        assert hasattr(ops, n)
    for n in ("forward_backward_cycle", "_forward_backward_consistency", "oob_ratio", "_oob_ratio", "cycle_and_oob", "validate"):
        assert hasattr(validation, n)
    from models.PWCNet import PWCDCNet, PWCDCNet_old
    assert callable(PWCDCNet.flow_pair) and callable(PWCDCNet_old.flow_pair)


def test_workspace_formula_and_rejects_without_device():
    """Only arguments that are refused before any launch."""
    from opticalflow_amd import _lib
    lib = _lib.load()
    for B, H, W in ((4, 384, 512), (16, 448, 1024), (1, 37, 53), (2, 2, 2)):
        assert lib.pwc_fb_metrics_workspace_bytes(B, H, W) == 16 + 16 * B * ((H + 15) // 16) * ((W + 63) // 64)
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert lib.pwc_fb_metrics_workspace_bytes(*bad) == -1
    if torch.cuda.is_available():
        keep = [torch.zeros(1 << 18, dtype=torch.float32, device="cuda:0") for _ in range(4)]
        p = [ctypes.c_void_p(t.data_ptr()) for t in keep]
    else:
        p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(4)]

    def call(f12=p[0], f21=p[1], B=1, h=8, w=16, H=32, W=64, bs=None, ws=p[2], nb=None, out=p[3]):
        need = lib.pwc_fb_metrics_workspace_bytes(max(B, 1), max(H, 1), max(W, 1))
        bs = bs or (2 * h * w, 2 * h * w)
        return lib.pwc_fb_metrics(f12, f21, B, h, w, H, W, bs[0], bs[1], ws, need if nb is None else nb, out, None)

    for kw in (dict(f12=None), dict(ws=None), dict(out=None)):
        assert call(**kw) == -1 and b"null pointer" in lib.pwc_last_error()
    assert call(B=0) == -1 and b"bad shape" in lib.pwc_last_error()
    for H, W, h, w in ((1, 64, 1, 16), (32, 1, 8, 1), (32, 64, 1, 16), (32, 64, 8, 1), (32, 64, 33, 16), (32, 64, 8, 65)):
        assert call(H=H, W=W, h=h, w=w) == -1 and b"declined geometry" in lib.pwc_last_error(), (H, W, h, w)
    assert call(bs=(8, 256)) == -1 and b"batch stride" in lib.pwc_last_error()
    assert call(bs=(256, 8)) == -1 and b"batch stride" in lib.pwc_last_error()
    assert call(nb=16) == -1 and b"workspace" in lib.pwc_last_error()
    assert call(ws=ctypes.c_void_p(p[2].value + 4)) == -1 and b"workspace" in lib.pwc_last_error()
    assert call(f12=ctypes.c_void_p(p[0].value + 2)) == -1 and b"aligned" in lib.pwc_last_error()
    assert call(B=2, H=32768, W=16384, h=8, w=16) == -1 and b"2^31" in lib.pwc_last_error()      # B*2*H*W = 2^31


@pytest.mark.parametrize("name", CASES)
def test_torch_route_matches_reference_fp64(name):
    """float64 CPU tensors take the torch route whatever route is asked for; it restates the scripts' chain"""
    from opticalflow_amd import validation as V
    z = load_golden("g11_validation.npz")
    f12, f21, H, W = _case(z, name)
    t12 = torch.from_numpy(f12).double()
    oob = V.oob_ratio(t12, H, W, device=t12.device, dtype=torch.float64)
    assert oob.dim() == 0 and int(round(oob.item() * t12.shape[0] * H * W)) == int(z[name + "/oob_count"][0])
    assert torch.equal(oob, V._oob_ratio(t12, H, W, t12.device, torch.float64, route="torch"))
    if f21 is not None:
        t21 = torch.from_numpy(f21).double()
        for route in ("hip", "torch"):
            cyc, oob2 = V.cycle_and_oob(t12, t21, H, W, route=route)
            np.testing.assert_allclose(cyc.item(), z[name + "/cycle"][0], rtol=1e-12, atol=1e-15)
            assert torch.equal(oob2, oob)


def test_route_selection_on_cpu():
    from opticalflow_amd import ops, validation as V
    f = torch.zeros(1, 2, 8, 12)
    assert not ops.fb_metrics_supported(f, f, 32, 48)                      # not on a ROCm device
    assert not V._hip_applies("hip", f, f, 32, 48) and not V._hip_applies("torch", f, f, 32, 48)
    with pytest.raises(ValueError):
        V.cycle_and_oob(f, f, 32, 48, route="cuda")
    with pytest.raises(ValueError):
        V.validate(None, [], None, "cpu", route="fast")
    # flows of different sizes: each is upsampled on its own by the torch route
    cyc, oob = V.cycle_and_oob(torch.ones(1, 2, 8, 12), -torch.ones(1, 2, 16, 24) * 2, 32, 48)
    assert cyc.dim() == 0 and oob.dim() == 0 and abs(cyc.item()) < 1e-5


def test_flow_pair_cache_key():
    from opticalflow_amd import PWCDCNet, correlation
    net = PWCDCNet(normalize_corr=True)
    img = torch.zeros(2, 3, 64, 128)
    x = torch.zeros(2, 6, 64, 128)
    kp, kf = net._pair_key(img), net._key(x)
    assert kp != kf and kp[1:] == kf and kp[0] == "bidir"                   # same fields, told apart from a PwcPlan of that size
    assert net._pair_key(torch.zeros(4, 3, 64, 128)) != kp
    old = correlation.USE_ONNX_CORRELATION
    try:
        correlation.USE_ONNX_CORRELATION = True                             # the effective normalisation is part of the key
        assert net._pair_key(img) != kp
    finally:
        correlation.USE_ONNX_CORRELATION = old
    assert not net._shares_pyramid(img, img)                                # CPU tensors: two ordinary forwards
    assert not PWCDCNet(precision="fp16")._shares_pyramid(img, img)
    with pytest.raises(ValueError):
        net.flow_pair(img, torch.zeros(2, 3, 64, 64))


class _StubModel(torch.nn.Module):
    """A differentiable-free stand-in: 'flow' = a fixed linear map of the quarter-resolution image difference"""

    def __init__(self):
        super().__init__()
        self.calls = 0

    def forward(self, x):
        self.calls += 1
        a, b = x[:, :3], x[:, 3:]
        d = torch.nn.functional.avg_pool2d(b - a, 4)
        return torch.stack((3.0 * d[:, 0] + d[:, 1], d[:, 2] - 2.0 * d[:, 1]), dim=1)


def test_validate_torch_route_is_the_scripts_arithmetic():
    from opticalflow_amd import validation as V
    from opticalflow_amd.losses import ProxyLabelLoss, _warp_torch, upsample_flow_to
    gen = torch.Generator().manual_seed(5)
    loader = [(torch.rand(2, 3, 32, 48, generator=gen), torch.rand(2, 3, 32, 48, generator=gen)) for _ in range(3)]
    model, crit = _StubModel(), ProxyLabelLoss(variant="fundamental", route="torch")
    got = V.validate(model, loader, crit, torch.device("cpu"), route="torch")
    assert model.calls == 9                                                # the scripts' three forwards per batch
    # the scripts' loop, written out: float(.item()) sums, divided by the number of batches
    sums = [0.0, 0.0, 0.0, 0.0]
    for img1, img2 in loader:
        flow = model(torch.cat([img1, img2], 1))
        _, photo, smooth = crit(flow, img1, img2, valid_mask=None)
        f12 = upsample_flow_to(model(torch.cat([img1, img2], 1)), 32, 48)
        f21 = upsample_flow_to(model(torch.cat([img2, img1], 1)), 32, 48)
        fb = (f12 + _warp_torch(f21, f12)).abs().mean()
        yy, xx = torch.meshgrid(torch.linspace(-1.0, 1.0, 32), torch.linspace(-1.0, 1.0, 48), indexing="ij")
        up = upsample_flow_to(flow, 32, 48)
        x, y = xx + 2.0 * up[:, 0] / 47, yy + 2.0 * up[:, 1] / 31
        oob = ((x < -1) | (x > 1) | (y < -1) | (y > 1)).float().mean()
        for i, t in enumerate((photo, smooth, fb, oob)):
            sums[i] += float(t.item())
    want = dict(zip(("val_photo", "val_smooth", "val_fb", "val_oob"), (s / 3 for s in sums)))
    assert got == want
    # the hip route on CPU tensors: same values through the torch metric chain, with two forwards per batch (flow12 is reused)
    model.calls = 0
    got_hip = V.validate(model, loader, ProxyLabelLoss(variant="pseudo", route="hip"), "cpu", route="hip")
    assert model.calls == 6
    want_pseudo = V.validate(model, loader, ProxyLabelLoss(variant="pseudo", route="torch"), "cpu", route="torch")
    assert got_hip == want_pseudo
    assert V.validate(model, [], crit, "cpu") == {"val_photo": 0.0, "val_smooth": 0.0, "val_fb": 0.0, "val_oob": 0.0}
    c = V.forward_backward_cycle(model, *loader[0])
    assert c.dim() == 0 and torch.equal(c, V._forward_backward_consistency(model, *loader[0], crit.warp))
