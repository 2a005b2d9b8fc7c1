"""CPU checks of the supervised losses (train.py / train2.py): the C ABI is declared, bound and exported and validates its
arguments before any launch; the torch route and the fp64 oracle reproduce the reference's own float64 results (g10 fixture);
the oracle's float32 index arithmetic is torch's own interpolate at the ratios training meets."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO, load_golden
import supervised_loss_oracle as O

NAMES = ("pwc_sup_flow_loss_workspace_bytes", "pwc_sup_flow_loss_fwd", "pwc_sup_flow_loss_bwd",
         "pwc_sup_multiscale_loss_workspace_bytes", "pwc_sup_multiscale_loss_fwd", "pwc_sup_multiscale_loss_bwd")
FLOW_CASES = ("train", "kitti_odd", "same", "allzero", "epe_raw", "epe_none")
MS_CASES = ("ms", "ms_reg", "ms_odd")


def test_symbols_declared_bound_exported():
    from opticalflow_amd import _lib
    text = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n + "(" in text and n in _lib.SIGNATURES and hasattr(lib, n)
    assert "#define PWC_ABI_VERSION 13" in text and _lib.load().pwc_abi_version() == 13
    from opticalflow_amd import losses, ops
    for n in ("sup_flow_loss", "sup_flow_loss_backward", "FlowLossFunction", "sup_multiscale_loss",
              "sup_multiscale_loss_backward", "MultiscaleLossFunction", "sup_flow_loss_supported", "sup_multiscale_loss_supported"):
        assert hasattr(ops, n)
    for n in ("MaskedCharbonnier", "supervised_multiscale_loss", "compute_epe", "upsample_flow_to"):
        assert hasattr(losses, n)


def _hw(*sizes):
    return (ctypes.c_int * (2 * len(sizes)))(*[s for hw in sizes for s in hw])


def test_workspace_formula():
    from opticalflow_amd import _lib
    lib = _lib.load()
    r256 = lambda n: (n + 255) // 256 * 256                                        # noqa: E731
    for B, H, W, h, w in ((4, 320, 896, 80, 224), (1, 375, 1242, 94, 311), (2, 8, 8, 8, 8)):
        fwd = r256(-(-B * H * W // 1024) * 16)
        assert lib.pwc_sup_flow_loss_workspace_bytes(B, H, W, h, w, 0) == fwd
        assert lib.pwc_sup_flow_loss_workspace_bytes(B, H, W, h, w, 1) == max(fwd, r256(B * 2 * H * w * 8))
    assert lib.pwc_sup_flow_loss_workspace_bytes(0, 8, 8, 2, 2, 0) == -1
    sizes = ((96, 192), (48, 96), (24, 48), (12, 24), (6, 12))
    blocks = sum(-(-4 * h * w // 1024) for h, w in sizes)
    part = r256(blocks * 48)
    assert lib.pwc_sup_multiscale_loss_workspace_bytes(4, 384, 768, 5, _hw(*sizes), 0) == part
    assert lib.pwc_sup_multiscale_loss_workspace_bytes(4, 384, 768, 5, _hw(*sizes), 1) == part + r256(sum(4 * 6 * h * w * 4 for h, w in sizes))
    assert lib.pwc_sup_multiscale_loss_workspace_bytes(4, 384, 768, 9, _hw(*(sizes + sizes[:4])), 0) == -1     # > 8 levels
    assert lib.pwc_sup_multiscale_loss_workspace_bytes(4, 384, 768, 1, None, 0) == -1


def _buffers(n=8):
    """Operand buffers.  Where a GPU exists they are real 1 MiB device allocations, larger than any geometry passed below, so no
    argument check -- wherever it sits -- could let a kernel touch memory that is not there; without a GPU, addresses that are
    never dereferenced."""
    if torch.cuda.is_available():
        keep = [torch.zeros((1 << 20) // 4, dtype=torch.float32, device="cuda:0") for _ in range(n)]
        return [ctypes.c_void_p(t.data_ptr()) for t in keep], keep
    return [ctypes.c_void_p(4096 * (i + 1)) for i in range(n)], None


def test_flow_loss_argument_errors_without_launch():
    from opticalflow_amd import _lib
    lib = _lib.load()
    (pred, gt, mask, out, ws, fo, go, gp), _keep = _buffers()
    B, H, W, h, w = 1, 16, 24, 4, 6
    nb = lib.pwc_sup_flow_loss_workspace_bytes(B, H, W, h, w, 1)
    args = lambda **k: dict(dict(h=h, w=w, rule=0, ws=ws, nb=nb, bsp=2 * h * w, bsg=2 * H * W, eps=1e-3), **k)   # noqa: E731

    def fwd(p=pred, g=gt, **k):
        a = args(**k)
        return lib.pwc_sup_flow_loss_fwd(p, g, mask, 0, a["rule"], out, B, H, W, a["h"], a["w"], a["eps"], a["bsp"], a["bsg"],
                                         H * W, a["ws"], a["nb"], None)

    assert fwd(p=None) == -1 and b"null pointer" in lib.pwc_last_error()
    assert fwd(g=None) == -1
    assert fwd(ws=None) == -1
    assert fwd(rule=2) == -1 and b"mask rule" in lib.pwc_last_error()
    assert fwd(eps=-1.0) == -1
    assert fwd(bsp=2 * h * w - 1) == -1 and b"batch stride" in lib.pwc_last_error()
    assert fwd(nb=8) == -1 and b"workspace" in lib.pwc_last_error()
    assert fwd(h=1, bsp=2 * w) == -2 and b"declined geometry" in lib.pwc_last_error()
    assert fwd(h=H + 1, bsp=2 * (H + 1) * w, nb=1 << 20) == -2
    assert fwd(w=W + 1, bsp=2 * h * (W + 1), nb=1 << 20) == -2
    assert lib.pwc_sup_flow_loss_bwd(pred, gt, mask, 0, 0, None, go, gp, B, H, W, h, w, 1e-3, 2 * h * w, 2 * H * W, H * W,
                                     ws, nb, None) == -1
    assert lib.pwc_sup_flow_loss_bwd(pred, gt, mask, 0, 0, fo, go, gp, B, H, W, h, w, 1e-3, 2 * h * w, 2 * H * W, H * W,
                                     ws, 16, None) == -1


def test_multiscale_argument_errors_without_launch():
    from opticalflow_amd import _lib
    lib = _lib.load()
    (p0, p1, gt, mask, img, out, ws, go), _keep = _buffers()
    B, H, W = 1, 32, 48
    sizes = ((8, 12), (4, 6))
    ptrs = (ctypes.c_void_p * 2)(p0.value, p1.value)
    wts = (ctypes.c_float * 2)(0.32, 0.08)
    nb = lib.pwc_sup_multiscale_loss_workspace_bytes(B, H, W, 2, _hw(*sizes), 1)

    def fwd(preds=ptrs, hw=sizes, L=2, g=gt, images=img, lp=0.5, ls=0.0, n=nb, bsi=6 * H * W):
        return lib.pwc_sup_multiscale_loss_fwd(ctypes.cast(preds, ctypes.c_void_p) if preds is not None else None, None,
                                               _hw(*hw), ctypes.cast(wts, ctypes.c_void_p), L, g, mask, 0, images, out, B, H, W,
                                               1e-3, lp, ls, 2 * H * W, H * W, bsi, ws, n, None)

    assert fwd(preds=None) == -1 and b"null pointer" in lib.pwc_last_error()
    assert fwd(g=None) == -1
    assert fwd(images=None) == -1 and b"images" in lib.pwc_last_error()
    assert fwd(L=0) == -1
    assert fwd(lp=-1.0) == -1
    assert fwd(n=64) == -1 and b"workspace" in lib.pwc_last_error()
    assert fwd(bsi=6 * H * W - 1) == -1 and b"batch stride" in lib.pwc_last_error()
    nulls = (ctypes.c_void_p * 2)(p0.value, None)
    assert fwd(preds=nulls) == -1 and b"level 1" in lib.pwc_last_error()
    assert fwd(hw=((8, 12), (1, 6))) == -2 and b"declined geometry of level 1" in lib.pwc_last_error()
    assert fwd(hw=((33, 12), (4, 6)), n=1 << 20) == -2
    L9 = (ctypes.c_void_p * 9)(*([p0.value] * 9))
    assert fwd(preds=L9, hw=sizes * 4 + sizes[:1], L=9) == -2 and b"at most 8" in lib.pwc_last_error()
    gptrs = (ctypes.c_void_p * 2)(out.value, None)
    assert lib.pwc_sup_multiscale_loss_bwd(ctypes.cast(ptrs, ctypes.c_void_p), None, _hw(*sizes), ctypes.cast(wts, ctypes.c_void_p),
                                           2, gt, mask, 0, img, out, go, ctypes.cast(gptrs, ctypes.c_void_p), B, H, W, 1e-3, 0.5,
                                           0.0, 2 * H * W, H * W, 6 * H * W, ws, nb, None) == -1
    assert b"gradient of level 1" in lib.pwc_last_error()


def test_supported_mirror_declines():
    from opticalflow_amd import ops
    cpu = torch.zeros(1, 2, 8, 8)
    assert not ops.sup_flow_loss_supported(cpu[:, :, :4, :4], cpu)             # off the device
    assert not ops.sup_multiscale_loss_supported([cpu[:, :, :4, :4]], cpu)


# ------------------------------------------------------------------ g10: the reference's own float64 results
def _flow_case(z, name):
    t = lambda k: torch.from_numpy(z[name + "/" + k].astype(np.float64))        # noqa: E731
    mask = t("mask") if name + "/mask" in z.files else None
    return t("pred"), t("gt"), mask, float(z[name + "/loss"][0]), z[name + "/grad"]


def _ms_case(z, name):
    n = int(z[name + "/nlev"][0])
    preds = [torch.from_numpy(z["%s/pred%d" % (name, k)].astype(np.float64)) for k in range(n)]
    images = torch.from_numpy(z[name + "/images"].astype(np.float64)) if name + "/images" in z.files else None
    lp, ls = (float(v) for v in z[name + "/cfg"])
    w = [float(v) for v in z[name + "/w"]] or None
    return (preds, images, torch.from_numpy(z[name + "/gt"].astype(np.float64)), torch.from_numpy(z[name + "/mask"].astype(np.float64)),
            w, lp, ls, float(z[name + "/loss"][0]), [z["%s/grad%d" % (name, k)] for k in range(n)])


@pytest.mark.parametrize("name", FLOW_CASES)
def test_torch_route_and_oracle_reproduce_g10_flow_losses(name):
    from opticalflow_amd import losses
    z = load_golden("g10_supervised_loss.npz")
    pred, gt, mask, want, gwant = _flow_case(z, name)
    p = pred.clone().requires_grad_(True)
    if name.startswith("epe"):
        got = losses.compute_epe(p, gt, mask, route="torch")
        lo, go = O.flow_loss(pred.numpy(), gt.numpy(), mask, eps=0.0, rule="raw")
    else:
        got = losses.MaskedCharbonnier(route="torch")(p, gt, mask)
        lo, go = O.flow_loss(pred.numpy(), gt.numpy(), mask)
    (g,) = torch.autograd.grad(got, p)
    np.testing.assert_allclose(got.item(), want, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(g.numpy(), gwant, rtol=0, atol=1e-12 * max(np.abs(gwant).max(), 1e-30))
    # the oracle's fp32 index rounding vs the reference's float64 resize: ~1e-7 relative
    np.testing.assert_allclose(lo, want, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(go, gwant, rtol=0, atol=1e-5 * max(np.abs(gwant).max(), 1e-30))


@pytest.mark.parametrize("name", MS_CASES)
def test_torch_route_and_oracle_reproduce_g10_multiscale(name):
    from opticalflow_amd import losses
    z = load_golden("g10_supervised_loss.npz")
    preds, images, gt, mask, w, lp, ls, want, gwant = _ms_case(z, name)
    ps = [p.clone().requires_grad_(True) for p in preds]
    got = losses.supervised_multiscale_loss(ps, images, gt, mask, w=w, lambda_photo=lp, lambda_smooth=ls, route="torch")
    grads = torch.autograd.grad(got, ps)
    np.testing.assert_allclose(got.item(), want, rtol=1e-12)
    for g, gw in zip(grads, gwant):
        np.testing.assert_allclose(g.numpy(), gw, rtol=0, atol=1e-12 * np.abs(gw).max())
    lo, go = O.multiscale_loss([p.numpy() for p in preds], images.numpy() if images is not None else None, gt.numpy(),
                               mask.numpy(), w, lp, ls)
    np.testing.assert_allclose(lo, want, rtol=1e-6)
    for g, gw in zip(go, gwant):
        np.testing.assert_allclose(g, gw, rtol=0, atol=1e-5 * np.abs(gw).max())


# ------------------------------------------------------------------ torch's index arithmetic, at training ratios
RATIOS = ((375, 94), (1242, 311), (368, 23), (320, 5), (94, 375), (311, 1242), (80, 320), (224, 896))


@pytest.mark.parametrize("n_in,n_out", RATIOS)
def test_bilinear_taps_match_torch_interpolate(n_in, n_out):
    """Each source index of the oracle (= the kernels' fp32 rule) against torch's own align_corners=False resize of one-hot rows."""
    eye = torch.eye(n_in, dtype=torch.float32).reshape(n_in, 1, 1, n_in)
    got = F.interpolate(eye, size=(1, n_out), mode="bilinear", align_corners=False)[:, 0, 0, :].T.numpy()   # [n_out, n_in]
    A = O.interp_matrix(n_in, n_out)
    # the same taps; weights within two fp32 ulps of the source coordinate (torch's CPU resize rounds its lambda in its own
    # order; the GPU kernel the scripts run, like the HIP kernels, takes s - (int)s)
    assert np.array_equal(got > 1e-4, A > 1e-4)
    np.testing.assert_allclose(got, A, rtol=0, atol=2 * 2.0 ** -23 * n_in)
    i0, i1, l0, l1 = O.linear_taps(n_in, n_out)
    assert i0.min() >= 0 and i1.max() <= n_in - 1 and np.all(i1 - i0 <= 1)


@pytest.mark.parametrize("n_in,n_out", [r for r in RATIOS if r[0] > r[1]])
def test_nearest_index_matches_torch_interpolate(n_in, n_out):
    x = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, 1, n_in)
    got = F.interpolate(x, size=(1, n_out), mode="nearest")[0, 0, 0].numpy().astype(np.int64)
    np.testing.assert_array_equal(got, O.nearest_index(n_in, n_out))


def test_hand_checked_indices():
    # 375 -> 94: scale = 375/94 = 3.98936...; dst 0: s = 1.4946..; dst 93: s = 372.505..
    i0, i1, l0, l1 = O.linear_taps(375, 94)
    assert (i0[0], i1[0], i0[93], i1[93]) == (1, 2, 372, 373)
    # 368 -> 23 (16x): dst 0 -> s = 7.5; nearest floor(dst * 16)
    i0, _, _, l1 = O.linear_taps(368, 23)
    assert i0[0] == 7 and l1[0] == 0.5 and i0[22] == 359
    assert list(O.nearest_index(368, 23)[:3]) == [0, 16, 32]
    # 320 -> 5 (64x): nearest 0, 64, ..., 256; bilinear s = 31.5, 95.5, ...
    assert list(O.nearest_index(320, 5)) == [0, 64, 128, 192, 256]
    assert list(O.linear_taps(320, 5)[0]) == [31, 95, 159, 223, 287]
    # upsampling 94 -> 375: the first output pixels clamp at 0; the last taps stop at in-1
    i0, i1, l0, l1 = O.linear_taps(94, 375)
    assert i0[0] == 0 and l1[0] == 0.0 and i0[-1] == 93 and i1[-1] == 93
