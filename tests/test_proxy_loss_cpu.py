"""CPU checks of the proxy-label loss (train_pseudo.py / train_fundamental.py): the C ABI is declared, bound and exported and
validates its arguments before any launch; the torch route reproduces the reference's own float64 results (g8 fixture); the
float32 restatement of the kernel's sample-point arithmetic gives hand-computed values."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import REPO, load_golden
import proxy_loss_oracle as O

NAMES = ("pwc_proxy_loss_workspace_bytes", "pwc_proxy_loss_fwd", "pwc_proxy_loss_bwd", "pwc_flow_warp_image_fwd")


def test_symbols_declared_bound_exported():
    from opticalflow_amd import _lib
    text = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n + "(" in text and n in _lib.SIGNATURES and hasattr(lib, n)
    assert "#define PWC_ABI_VERSION 13" in text and _lib.load().pwc_abi_version() == 13
    from opticalflow_amd import losses, ops
    for n in ("proxy_loss", "proxy_loss_backward", "flow_warp_image", "ProxyLossFunction"):
        assert hasattr(ops, n)
    for n in ("ProxyLabelLoss", "upsample_flow_to", "warp_image"):
        assert hasattr(losses, n)


def test_workspace_formula():
    from opticalflow_amd import _lib
    lib = _lib.load()

    def want(B, H, W):
        tiles = B * ((H + 15) // 16) * ((W + 63) // 64)
        gup = (B * 2 * H * W * 4 + 255) // 256 * 256
        return tiles * 32, max(tiles * 32, gup + 256)

    for dims in ((4, 3, 384, 512, 96, 128), (16, 3, 448, 1024, 112, 256), (1, 3, 37, 53, 10, 14), (2, 2, 2, 2, 2, 2)):
        fwd, both = want(dims[0], dims[2], dims[3])
        assert lib.pwc_proxy_loss_fwd_workspace_bytes(*dims) == fwd
        assert lib.pwc_proxy_loss_workspace_bytes(*dims) == both
    for bad in ((0, 3, 8, 8, 2, 2), (1, 0, 8, 8, 2, 2), (1, 3, -1, 8, 2, 2), (1, 3, 8, 8, 0, 2), (1, 3, 8, 8, 2, -3)):
        assert lib.pwc_proxy_loss_workspace_bytes(*bad) == -1
        assert lib.pwc_proxy_loss_fwd_workspace_bytes(*bad) == -1


_BUF_BYTES = 1 << 20


def _buffers():
    """Seven operand buffers (flow img1 img2 mask out workspace grad_out).  Where a GPU exists they are real 1 MiB device
    allocations, larger than any geometry passed below except the 2^31 case, so that no argument check -- wherever it sits --
    could let a kernel touch memory that is not there; without a GPU, addresses that are never dereferenced."""
    if torch.cuda.is_available():
        keep = [torch.zeros(_BUF_BYTES // 4, dtype=torch.float32, device="cuda:0") for _ in range(7)]
        return [ctypes.c_void_p(t.data_ptr()) for t in keep], keep
    return [ctypes.c_void_p(4096 * (i + 1)) for i in range(7)], None


def _fwd(lib, p, B=1, C=3, H=32, W=64, h=8, w=16, ws=None, bs=None, mask_u8=0):
    need = lib.pwc_proxy_loss_fwd_workspace_bytes(max(B, 1), max(C, 1), max(H, 1), max(W, 1), max(h, 1), max(w, 1))
    st = bs or (2 * h * w, C * H * W, C * H * W, H * W)
    return lib.pwc_proxy_loss_fwd(p[0], p[1], p[2], p[3], mask_u8, p[4], B, C, H, W, h, w, 1.0, 0.1, 0.0, *st, p[5],
                                  need if ws is None else ws, None)


def _bwd(lib, p, B=1, C=3, H=32, W=64, h=8, w=16, ws=None):
    need = lib.pwc_proxy_loss_workspace_bytes(max(B, 1), max(C, 1), max(H, 1), max(W, 1), max(h, 1), max(w, 1))
    return lib.pwc_proxy_loss_bwd(p[0], p[1], p[2], p[3], 0, p[6], p[4], B, C, H, W, h, w, 1.0, 0.1, 0.0,
                                  2 * h * w, C * H * W, C * H * W, H * W, p[5], need if ws is None else ws, None)


def test_entries_reject_without_device():
    """Only arguments that are refused before any launch; with real buffers where a GPU exists (see _buffers)."""
    from opticalflow_amd import _lib
    lib = _lib.load()
    buf, _keep = _buffers()
    for i in (0, 1, 2, 4, 5):
        p = list(buf)
        p[i] = None
        assert _fwd(lib, p) == -1 and b"null pointer" in lib.pwc_last_error()
        assert _bwd(lib, p) == -1 and b"null pointer" in lib.pwc_last_error()
    p = list(buf)
    p[6] = None
    assert _bwd(lib, p) == -1
    assert _fwd(lib, buf, C=0) == -1 and b"bad shape" in lib.pwc_last_error()
    assert _fwd(lib, buf, bs=(8, 3 * 32 * 64, 3 * 32 * 64, 32 * 64)) == -1 and b"batch stride" in lib.pwc_last_error()
    assert _fwd(lib, buf, ws=32) == -1 and b"workspace" in lib.pwc_last_error()
    assert _bwd(lib, buf, ws=lib.pwc_proxy_loss_fwd_workspace_bytes(1, 3, 32, 64, 8, 16)) == -1
    assert b"workspace" in lib.pwc_last_error()
    # declined geometries: PWC_EUNSUPPORTED, nothing launched
    for H, W, h, w in ((1, 64, 1, 16), (32, 1, 8, 1), (32, 64, 1, 16), (32, 64, 8, 1), (32, 64, 33, 16), (32, 64, 8, 65)):
        assert _fwd(lib, buf, H=H, W=W, h=h, w=w) == -2, (H, W, h, w)
        assert _bwd(lib, buf, H=H, W=W, h=h, w=w) == -2
        assert lib.pwc_flow_warp_image_fwd(buf[1], buf[0], buf[4], 1, 3, H, W, h, w, 3 * H * W, 2 * h * w, 3 * H * W, None) == -2
    odd = list(buf)
    odd[1] = ctypes.c_void_p(buf[1].value + 2)
    assert _fwd(lib, odd) == -2 and _bwd(lib, odd) == -2
    assert lib.pwc_flow_warp_image_fwd(None, buf[0], buf[4], 1, 2, 8, 8, 2, 2, 128, 8, 128, None) == -1
    if not torch.cuda.is_available():
        # C*H*W >= 2^31: no buffer of that size is allocated for a unit test, so this decline is checked where nothing can run
        big = (1, 3, 16384, 65536, 8, 16)
        assert _fwd(lib, buf, *big, bs=(2 * 8 * 16, 3 * 16384 * 65536, 3 * 16384 * 65536, 16384 * 65536)) == -2


def _case(z, name):
    pfx = "base" if name.startswith("base") or name == "masked" else name
    img1, img2 = (torch.from_numpy(z[pfx + k]).double() for k in ("/img1", "/img2"))
    flow = torch.from_numpy(z[name + "/flow"]).double()
    mask = torch.from_numpy(z[name + "/mask"]).double() if name + "/mask" in z.files else None
    ap, asm, fund = (float(v) for v in z[name + "/cfg"])
    return flow, img1, img2, mask, ap, asm, "fundamental" if fund else "pseudo"


@pytest.mark.parametrize("name", ["base_pseudo", "base_fund", "odd", "same", "clamp", "masked"])
def test_torch_route_matches_reference_fp64(name):
    from opticalflow_amd.losses import ProxyLabelLoss
    z = load_golden("g8_proxy_loss.npz")
    flow, img1, img2, mask, ap, asm, variant = _case(z, name)
    flow.requires_grad_(True)
    loss = ProxyLabelLoss(ap, asm, variant=variant, route="hip")      # CPU tensors: the hip route declines to the torch route
    total, photo, smooth = loss(flow, img1, img2, mask)
    (g,) = torch.autograd.grad(total, flow)
    ref = z[name + "/loss"]
    np.testing.assert_allclose([total.item(), photo.item(), smooth.item()], ref, rtol=1e-12, atol=0)
    gr = z[name + "/grad_flow"]
    assert np.abs(g.numpy() - gr).max() <= 1e-12 * np.abs(gr).max()


def test_torch_warp_matches_reference_fp64():
    from opticalflow_amd.losses import ProxyLabelLoss, warp_image
    z = load_golden("g8_proxy_loss.npz")
    img, flow = torch.from_numpy(z["warp2/img"]).double(), torch.from_numpy(z["warp2/flow"]).double()
    np.testing.assert_allclose(ProxyLabelLoss().warp(img, flow).numpy(), z["warp2/out"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(warp_image(img, flow).numpy(), z["warp2/out_fund"], rtol=0, atol=1e-12)


def test_coordinate_restatement_hand_vectors():
    # h=3 -> H=7: rh = fl(2/6) = 0.3333333432674408; rh * 3 = 1.0000000298 rounds to 1.0 in float32, rh * 6 to 2.0 (= h-1:
    # the second row index stays 2)
    y0, y1, l1, l0 = O._lin32(3, 7)
    assert y0.tolist() == [0, 0, 0, 1, 1, 1, 2] and y1.tolist() == [1, 1, 1, 2, 2, 2, 2]
    assert l1.dtype == np.float32 and l1[3] == 0.0 and l1[6] == 0.0
    assert l1[1] == np.float32(np.float32(2.0 / 6.0) * np.float32(1.0))     # 0.33333334
    assert l1[2] == np.float32(0.6666667)
    # w=2 -> W=5: rw = 0.25 exactly, sx = 2.5; a constant flow (1, -1) becomes (2.5, -2.5 * H/h)
    flow = torch.zeros(1, 2, 3, 2)
    flow[:, 0], flow[:, 1] = 1.0, -1.0
    px, py = O.sample_points32(flow, 7, 5)
    assert px[0, 0].tolist() == [2.5, 3.5, 4.5, 5.5, 6.5]
    assert py.dtype == torch.float32 and py[0, 0, 0].item() == np.float32(-np.float32(7 / 3))
    # bilinear between rows: flow rows (0, 3, 6) at h=3 -> H=5 (rh = 0.5): row 1 is 1.5 * H/h
    f2 = torch.zeros(1, 2, 3, 2)
    f2[:, 1] = torch.tensor([0.0, 3.0, 6.0]).view(3, 1)
    _, py2 = O.sample_points32(f2, 5, 2)
    sy = np.float32(5 / 3)
    assert py2[0, :, 0].tolist() == [0.0, 1 + np.float32(1.5) * sy, 2 + np.float32(3.0) * sy, 3 + np.float32(4.5) * sy,
                                      4 + np.float32(6.0) * sy]
    # full-resolution flow: px = X + u exactly
    f3 = torch.full((1, 2, 2, 3), 0.25)
    px3, _ = O.sample_points32(f3, 2, 3)
    assert px3[0, 0].tolist() == [0.25, 1.25, 2.25]
