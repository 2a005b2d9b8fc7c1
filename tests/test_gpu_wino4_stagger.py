"""Staggered schedule of the F(4x4) Winograd loop (pwc_conv_wino4.hip, wino4p_body with SH = 1; option "w4_stagger"): waves 4-7 of a
workgroup place their VALU bursts and LDS reads behind other MFMAs of a phase than waves 0-3.  Only the order of independent
instructions changes, so every launch must give the SAME BITS as the parent schedule (w4_stagger = 0) -- under the shipped value (1:
the forms where it measured faster) and under 2 (every form).  The cases reach every Geo4 instantiation at the smallest shapes where
the schedule can go wrong: 1, 2 and 3 chunks (prologue shorter than the ring), an odd and an even count (parity ping-pong of the row
and V buffers, the carried column 2) and a ragged last chunk."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHIPPED = 1

# (B, cin, cout, H, W, split2, workspace, kernel reported for the call's last launch: (CB, TG, GW, IH))
CASES = [
    # <4,2,64>: one 64-cout workgroup of 8 x 64 pixels
    (1, 4, 64, 8, 64, False, False, (4, 2, 64, 0)),
    (1, 8, 64, 8, 64, False, False, (4, 2, 64, 0)),
    (1, 12, 64, 8, 64, False, False, (4, 2, 64, 0)),
    (1, 37, 64, 8, 64, False, False, (4, 2, 64, 0)),
    (1, 130, 64, 8, 64, False, False, (4, 2, 64, 0)),
    # 32-cout launches: <2,4,64> at 16 x 64; 72 columns pick the 32-column groups (<2,4,32>), two column tiles, ragged rows
    (2, 5, 32, 16, 64, False, False, (2, 4, 64, 0)),
    (2, 40, 32, 16, 64, False, False, (2, 4, 64, 0)),
    (2, 5, 32, 17, 72, False, False, (2, 4, 32, 0)),
    (2, 40, 32, 17, 72, False, False, (2, 4, 32, 0)),
    # 96 couts at 16 x 32: a <4,2,32> launch, then the last 32 couts
    (1, 12, 96, 16, 32, False, False, None),
    (1, 64, 96, 16, 32, False, False, None),
    # stacked forms: 14 x 32 images two per workgroup (the second group short), 7 x 16 images four per workgroup
    (3, 8, 32, 14, 32, False, False, (2, 4, 32, 16)),
    (3, 96, 32, 14, 32, False, False, (2, 4, 32, 16)),
    (5, 4, 64, 7, 16, False, False, (4, 2, 16, 8)),
    (5, 96, 64, 7, 16, False, False, (4, 2, 16, 8)),
    # pixel-lattice stores (PWC_CONV_SPLIT2), and the whole-launch split along Cin (needs the workspace)
    (1, 12, 64, 8, 64, True, False, (4, 2, 64, 0)),
    (1, 96, 64, 8, 64, False, True, (4, 2, 64, 0)),
]
FP64_CASE = (1, 130, 64, 8, 64, False, False, (4, 2, 64, 0))


def _id(c):
    return "B%d_%d-%d_%dx%d%s%s" % (c[0], c[1], c[2], c[3], c[4], "_split2" if c[5] else "", "_ws" if c[6] else "")


def _inputs(case, device):
    B, cin, cout, H, W = case[:5]
    g = torch.Generator().manual_seed(1000 + sum(case[:5]))
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    return x, w, b, x.to(device), w.to(device), b.to(device)


def _run(case, xd, wd, bd, value):
    """(output, reported kernel) of the case under w4_stagger = value"""
    from opticalflow_amd import _lib, ops
    B, cin, cout, H, W, split2, use_ws, _ = case
    ws = None
    if use_ws:
        nbytes = ops.conv3x3_wino4_workspace_bytes(B, cin, H, W, cout)
        assert nbytes > 0, "the case is meant to run as input-channel slices"
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=xd.device)
    saved = _lib.get_option("w4_stagger")
    try:
        _lib.set_option("w4_stagger", value)
        out = ops.conv3x3_wino4(xd, ops.pack_conv3x3_wino4(wd), bd, cout, split2=split2, workspace=ws)
        torch.cuda.synchronize()
        return out, _lib.load().pwc_last_conv_kernel().decode()
    finally:
        _lib.set_option("w4_stagger", saved)


def _kernel_args(kern):
    return [int(v) for v in kern[kern.index("<") + 1:kern.index(">")].split(",")]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_stagger_bit_identical(gpu_device, case):
    _, _, _, xd, wd, bd = _inputs(case, gpu_device)
    base, kern = _run(case, xd, wd, bd, 0)
    assert kern.startswith("conv3x3_wino4p_kernel<")
    a = _kernel_args(kern)
    print("%s: %s" % (_id(case), kern))
    if case[7] is not None:
        assert (a[0], a[1], a[2], a[5]) == case[7], kern
    assert (a[3] > 1) == case[6], "input-channel slices: %s" % kern
    assert bool(torch.isfinite(base).all()) and base.abs().max().item() > 0
    for value in (SHIPPED, 2):
        got, kern_v = _run(case, xd, wd, bd, value)
        assert kern_v == kern
        assert torch.equal(got, base), "w4_stagger = %d changes the result of %s" % (value, kern)


def test_stagger_vs_fp64(gpu_device):
    """the staggered launch itself against an fp64 convolution: the F(4x4) budget of test_conv3x3_winograd4_vs_fp64"""
    case = FP64_CASE
    x, w, b, xd, wd, bd = _inputs(case, gpu_device)
    cin = case[1]
    ref = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), padding=1), 0.1)
    for value in (0, SHIPPED, 2):
        got, kern = _run(case, xd, wd, bd, value)
        err = (got.cpu().double() - ref).abs().max().item()
        print("w4_stagger = %d, %s: max err vs fp64 %.2e (budget %.2e)" % (value, kern, err, 1e-6 * (cin * 9) ** 0.5))
        assert err <= 1e-6 * (cin * 9) ** 0.5


def test_stagger_option_roundtrip(gpu_device):
    from opticalflow_amd import _lib
    saved = _lib.get_option("w4_stagger")
    try:
        _lib.set_option("w4_stagger", 0)
        assert _lib.get_option("w4_stagger") == 0
    finally:
        _lib.set_option("w4_stagger", saved)
    assert _lib.get_option("w4_stagger") == saved
