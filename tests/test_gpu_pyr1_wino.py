"""The 16-channel Winograd kernels of the fp32 first pyramid level (csrc/pwc_pyr1_wino.hip; conv1aa and conv1b layer by layer or as
one launch, option "pyr1_wino" = 1 / 2).

Bounds are the project's, not this kernel's: per element 3e-6 * sqrt(9 * Cin) of test_conv3x3_baseline_shapes_vs_fp64 on data and
weights drawn as there (unit-variance inputs, He-scaled filters, 0.1-scaled bias); between routes of the whole forward the 5e-5 EPE
of test_forward_winograd4_error_budget.  The kernel is F(2x2,3x3), so WINO4_REL_BAR (the F(4x4) bound) does not apply."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import REPO
from oracle import pwc_oracle as O

TOL = 3e-6 * (16 * 9) ** 0.5          # test_conv3x3_baseline_shapes_vs_fp64: 3e-6 * sqrt(Cin * 9)
ROUTE_EPE = 5e-5                      # test_forward_winograd4_error_budget: between two Winograd routes of one forward

# (N, H, W, extra batch stride in elements).  224x512 is the headline level-1 map (4 of its 32 images: the fp64 reference runs on the
# CPU); 19x100 is ragged in both directions (the tile is 8 x 64, a strip 2 rows); 5x12 is smaller than a tile; strides: views of
# a wider buffer, as the plan passes arena slices.
SHAPES = [(4, 224, 512, 0), (3, 19, 100, 0), (1, 5, 12, 0), (3, 24, 64, 16 * 24 * 64), (1, 9, 132, 0), (2, 16, 128, 4)]


def _layer(seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(16, 16, 3, 3, generator=g) * (2.0 / (16 * 9)) ** 0.5
    b = torch.randn(16, generator=g) * 0.1
    return w, b


def _strided(n, h, w, extra, dev, fill=None, gen=None):
    """[n,16,h,w] view with batch stride 16*h*w + extra; the gap is poisoned with NaN so that a kernel ignoring the stride shows"""
    buf = torch.full((n, 16 * h * w + extra), float("nan"), device=dev)
    v = buf[:, :16 * h * w].view(n, 16, h, w)
    if gen is not None:
        v.copy_(torch.randn(n, 16, h, w, generator=gen))
    elif fill is not None:
        v.fill_(fill)
    return buf, v


def _ref(x, w, b):
    return F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), padding=1), 0.1)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d+%d" % s for s in SHAPES])
def test_layer_vs_fp64(gpu_device, shape):
    from opticalflow_amd import ops, _lib
    n, h, w_, extra = shape
    w, b = _layer(16 * 7 + 16)
    gen = torch.Generator().manual_seed(1000 + h + w_)
    xbuf, x = _strided(n, h, w_, extra, gpu_device, gen=gen)
    obuf, out = _strided(n, h, w_, extra, gpu_device, fill=7.0)
    ops.pyr1_wino(x, ops.pack_pyr1_wino(w.to(gpu_device)), b.to(gpu_device), out=out)
    assert "pyr1_wino2" in _lib.load().pwc_last_conv_kernel().decode()
    torch.set_num_threads(max(8, torch.get_num_threads()))
    err = (out.cpu().double() - _ref(x.cpu(), w, b)).abs().max().item()
    print("pyr1_wino %s: max err %.2e (bound %.2e)" % (shape, err, TOL))
    assert err <= TOL
    if extra:                                                     # nothing was written between the images
        assert bool(torch.isnan(obuf[:, 16 * h * w_:]).all())
    again = torch.empty_like(out)
    ops.pyr1_wino(x, ops.pack_pyr1_wino(w.to(gpu_device)), b.to(gpu_device), out=again)
    assert torch.equal(again, out)


def _pair(seed):
    return _layer(seed), _layer(seed + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d+%d" % s for s in SHAPES])
def test_pair_vs_fp64(gpu_device, shape):
    """conv1aa + conv1b in one launch against fp64 of the composition, under the second layer's per-element bound.
    Against the two-launch route only closeness is asserted, not torch.equal: the fused kernel's output tile is 14 rows with a
    one-row ring, so its conv1aa Winograd tiles start on ODD rows (y0 - 1) while the layer kernel's start on even ones -- the same
    pixel is then the sum of a different 2x2 tile's terms, equal in exact arithmetic and different in the last bits.  (A 12-row tile
    would keep both passes on even rows at 1.42x instead of 1.22x the arithmetic.)"""
    from opticalflow_amd import ops, _lib
    n, h, w_, extra = shape
    (w1, b1), (w2, b2) = _pair(40)
    gen = torch.Generator().manual_seed(2000 + h + w_)
    xbuf, x = _strided(n, h, w_, extra, gpu_device, gen=gen)
    obuf, out = _strided(n, h, w_, extra, gpu_device, fill=7.0)
    u1, u2 = ops.pack_pyr1_wino(w1.to(gpu_device)), ops.pack_pyr1_wino(w2.to(gpu_device))
    bd1, bd2 = b1.to(gpu_device), b2.to(gpu_device)
    ops.pyr1_wino_pair(x, u1, bd1, u2, bd2, out=out)
    assert "pyr1_wino2_pair" in _lib.load().pwc_last_conv_kernel().decode()
    torch.set_num_threads(max(8, torch.get_num_threads()))
    ref = _ref(_ref(x.cpu(), w1, b1), w2, b2)
    err = (out.cpu().double() - ref).abs().max().item()
    two = ops.pyr1_wino(ops.pyr1_wino(x, u1, bd1), u2, bd2)
    d = (two - out).abs().max().item()
    print("pyr1_wino_pair %s: max err %.2e (bound %.2e); vs two launches %.2e" % (shape, err, TOL, d))
    assert err <= TOL and d <= TOL
    if extra:
        assert bool(torch.isnan(obuf[:, 16 * h * w_:]).all())
    again = torch.empty_like(out)
    ops.pyr1_wino_pair(x, u1, bd1, u2, bd2, out=again)
    assert torch.equal(again, out)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(30, 132), (14, 60), (5, 8)], ids=["30x132", "14x60", "5x8"])
def test_pair_border_is_zero_padding_of_the_first_layer(gpu_device, hw):
    """Input non-zero only in the two outermost rows and columns: conv1b must see ZERO outside conv1aa's map, not conv1aa evaluated
    there (which is non-zero next to such an input: bias and the border pixels)."""
    from opticalflow_amd import ops
    h, w_ = hw
    (w1, b1), (w2, b2) = _pair(60)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 16, h, w_, generator=g)
    x[:, :, 2:-2, 2:-2] = 0
    out = ops.pyr1_wino_pair(x.to(gpu_device), ops.pack_pyr1_wino(w1.to(gpu_device)), b1.to(gpu_device),
                             ops.pack_pyr1_wino(w2.to(gpu_device)), b2.to(gpu_device)).cpu()
    err = (out.double() - _ref(_ref(x, w1, b1), w2, b2)).abs().max().item()
    print("border-only input %s: max err %.2e (bound %.2e)" % (hw, err, TOL))
    assert err <= TOL


@pytest.mark.gpu
def test_pair_nan_stays_local(gpu_device):
    """A NaN input pixel reaches the 5x5 outputs of the two convolutions, and beyond them only what the 2x2 tile granularity adds: an
    F(2x2) tile is NaN when its 4x4 window holds one, which widens the set by at most one pixel per layer and side -> within +-4.
    Nothing in another image.  The pixel sits at the corner of four workgroup tiles (14 x 60)."""
    from opticalflow_amd import ops
    (w1, b1), (w2, b2) = _pair(80)
    g = torch.Generator().manual_seed(78)
    x = torch.randn(3, 16, 30, 132, generator=g)
    py, px = 14, 60
    x[1, 7, py, px] = float("nan")
    out = ops.pyr1_wino_pair(x.to(gpu_device), ops.pack_pyr1_wino(w1.to(gpu_device)), b1.to(gpu_device),
                             ops.pack_pyr1_wino(w2.to(gpu_device)), b2.to(gpu_device)).cpu()
    bad = torch.isnan(out).any(1)
    assert not bad[0].any() and not bad[2].any()
    ys, xs = torch.nonzero(bad[1], as_tuple=True)
    assert ys.min() >= py - 4 and ys.max() <= py + 4 and xs.min() >= px - 4 and xs.max() <= px + 4, (ys.min(), ys.max(), xs.min(), xs.max())
    assert bad[1, py - 2:py + 3, px - 2:px + 3].all()


@pytest.mark.gpu
def test_rule_keeps_other_widths_and_small_launches_on_the_old_route(gpu_device):
    from opticalflow_amd import ops, _lib
    assert ops.pyr1_wino_preferred(32, 224, 512) and ops.pyr1_wino_preferred(4, 224, 512)      # batch 16 and batch 2 at 448x1024
    assert not ops.pyr1_wino_preferred(2, 224, 512)               # batch 1: 448 tiles < two workgroups per CU, measured no faster
    assert not ops.pyr1_wino_preferred(32, 224, 510) and not ops.pyr1_wino_preferred(32, 224, 511)
    assert not ops.pyr1_wino_preferred(2, 32, 32)                 # 8 tiles: far fewer workgroups than CUs
    w, b = _layer(3)
    with pytest.raises(_lib.PwcHipError, match="multiple of 4"):
        ops.pyr1_wino(torch.zeros(1, 16, 8, 30, device=gpu_device), ops.pack_pyr1_wino(w.to(gpu_device)), b.to(gpu_device))
    saved = _lib.get_option("pyr1_wino")
    try:
        _lib.set_option("pyr1_wino", 0)
        assert not ops.pyr1_wino_preferred(32, 224, 512)
    finally:
        _lib.set_option("pyr1_wino", saved)


@pytest.mark.gpu
def test_nan_stays_inside_its_winograd_tiles(gpu_device):
    """One NaN input pixel reaches the 2x2 output tiles whose 4x4 input windows hold it and nothing else, in no other image
    (a 3x3 convolution would spread it over 3x3 outputs; F(2x2) over the tiles that its neighbourhood touches)."""
    from opticalflow_amd import ops
    w, b = _layer(5)
    g = torch.Generator().manual_seed(77)
    x = torch.randn(3, 16, 24, 132, generator=g)
    py, px = 9, 64                                                 # first column of the second workgroup tile, odd row
    x[1, 5, py, px] = float("nan")
    out = ops.pyr1_wino(x.to(gpu_device), ops.pack_pyr1_wino(w.to(gpu_device)), b.to(gpu_device)).cpu()
    bad = torch.isnan(out).any(1)                                  # [3, H, W]
    assert not bad[0].any() and not bad[2].any()
    ys, xs = torch.nonzero(bad[1], as_tuple=True)
    # tiles (rows 2i..2i+1, columns 2j..2j+1) read input rows 2i-1..2i+2, columns 2j-1..2j+2
    assert ys.min() >= 8 and ys.max() <= 11 and xs.min() >= 62 and xs.max() <= 65, (ys.min(), ys.max(), xs.min(), xs.max())
    assert bad[1, py - 1:py + 2, px - 1:px + 2].all()              # at least what the convolution itself spreads


def _forward(gpu_device, x, option):
    from opticalflow_amd import PWCDCNet, _lib, ops
    from opticalflow_amd.weights import synthetic_state_dict
    _lib.set_option("pyr1_wino", option)
    net = PWCDCNet()
    sd = synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02)
    net.load_state_dict(sd)
    net = net.to(gpu_device).eval()
    names = []
    real = ops.conv3x3, ops.pyr1_wino, ops.pyr1_wino_pair

    def spy(tag, fn):
        def f(xx, *a, **kw):
            r = fn(xx, *a, **kw)
            if xx.shape[1] in (3, 16):
                names.append((tag, _lib.load().pwc_last_conv_kernel().decode()))
            return r
        return f
    ops.conv3x3, ops.pyr1_wino, ops.pyr1_wino_pair = spy("conv3x3", real[0]), spy("pyr1_wino", real[1]), spy("pyr1_wino_pair", real[2])
    try:
        with torch.no_grad():
            plan = net._plan_for(x)
            f = plan.run(x).clone()
            macs = dict(plan.conv_macs)
    finally:
        ops.conv3x3, ops.pyr1_wino, ops.pyr1_wino_pair = real
    assert torch.equal(net(x), f)
    return f.cpu(), names, macs


@pytest.mark.gpu
@pytest.mark.parametrize("geom", [(2, 128, 192), (1, 448, 1024)], ids=["2x128x192", "1x448x1024"])
def test_forward_routes_agree(gpu_device, geom):
    from opticalflow_amd import _lib
    B, H, W = geom
    x = torch.rand(B, 6, H, W, generator=torch.Generator().manual_seed(1234)).to(gpu_device)
    saved = {n: _lib.get_option(n) for n in ("pyr1_wino", "pyr1_wino_min_tiles")}
    try:
        _lib.set_option("pyr1_wino_min_tiles", 1)                  # the small geometry takes the new kernel too
        res = {v: _forward(gpu_device, x, v) for v in (0, 1, 2)}
    finally:
        for n, v in saved.items():
            _lib.set_option(n, v)
    old = res[0][1]
    print("level-1 kernels, option 0: %s" % old)
    # option 0: five launches, all through pwc_conv2d_fwd; conv1aa / conv1b on its 16-cout kernel, which names itself (it used to leave
    # conv1a's name standing: the launch audit records the kernel of every launch, so a stale name would be a wrong record)
    assert [t for t, _ in old] == ["conv3x3"] * 5 and all("pyr1" not in k for _, k in old)
    assert "image_conv_s2_f32" in old[0][1] and "image_conv_s2_f32" in old[1][1]
    assert "conv3x3_mfma16_kernel" in old[2][1] and old[3][1] == old[2][1] and "conv3x3_mfma_kernel" in old[4][1]
    new = res[1][1]
    print("level-1 kernels, option 1: %s" % new)
    assert [t for t, _ in new] == ["conv3x3", "conv3x3", "pyr1_wino", "pyr1_wino", "conv3x3"]
    assert "pyr1_wino2" in new[2][1] and "pyr1_wino2" in new[3][1] and new[:2] == old[:2]
    assert res[1][2]["direct"] == res[0][2]["direct"] and res[1][2]["executed"] < res[0][2]["executed"]
    pair = res[2][1]
    print("level-1 kernels, option 2: %s" % pair)
    assert [t for t, _ in pair] == ["conv3x3", "conv3x3", "pyr1_wino_pair", "conv3x3"]
    assert "pyr1_wino2_pair" in pair[2][1] and pair[:2] == old[:2]
    assert res[2][2] == res[1][2]                                  # same layers, same count: the tiles' recomputed ring is not counted
    for a, b_ in ((1, 0), (2, 0), (2, 1)):
        d = O.epe(res[a][0], res[b_][0])
        print("forward %s, pyr1_wino %d vs %d: EPE %.3e" % (geom, a, b_, d))
        assert d <= ROUTE_EPE


def test_new_abi_symbols_are_declared_exported_and_bound():
    from opticalflow_amd import _lib
    text = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pwc_[a-z0-9_]+)\s*\(", text))
    new = {"pwc_pyr1_wino_packed_bytes", "pwc_pyr1_wino_preferred", "pwc_pyr1_wino_pack", "pwc_pyr1_wino_fwd", "pwc_pyr1_wino_pair_fwd"}
    assert new <= declared and new <= set(_lib.SIGNATURES)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in new:
        assert hasattr(lib, n), "library does not export %s" % n
    lib = _lib.load()
    assert lib.pwc_pyr1_wino_packed_bytes() == 16 * 16 * 16 * 4
    four = [ctypes.c_void_p(4096)] * 4
    assert lib.pwc_pyr1_wino_fwd(None, None, None, None, 1, 8, 8, 0.1, 1024, 1024, None) == -1 and b"null pointer" in lib.pwc_last_error()
    assert lib.pwc_pyr1_wino_fwd(*four, 1, 8, 30, 0.1, 3840, 3840, None) == -2 and b"multiple of 4" in lib.pwc_last_error()
    assert lib.pwc_pyr1_wino_fwd(*four, 1, 8, 32, 0.1, 8, 4096, None) == -1 and b"batch stride" in lib.pwc_last_error()
    assert lib.pwc_pyr1_wino_fwd(*four, 1, 8, 32, 0.1, 4098, 4096, None) == -3
    six = [ctypes.c_void_p(4096)] * 6
    assert lib.pwc_pyr1_wino_pair_fwd(*six, 1, 8, 30, 0.1, 3840, 3840, None) == -2
    assert lib.pwc_pyr1_wino_pair_fwd(*six, 1, 8, 32, 0.1, 4096, 4096, None) == -1 and b"in-place" in lib.pwc_last_error()
    # the rule: option on, W % 4 == 0, two 8 x 64 tiles per CU at least (batch 1 at 448x1024 is 448 tiles: old route); the value is the route
    pref = lib.pwc_pyr1_wino_preferred
    v = ctypes.c_int(-1)
    assert lib.pwc_get_option(b"pyr1_wino", ctypes.byref(v)) == 0 and v.value in (0, 1, 2)
    assert pref(32, 224, 512) == v.value and pref(4, 224, 512) == v.value and pref(2, 224, 512) == 0
    assert pref(32, 224, 510) == 0 and pref(4, 64, 96) == 0 and pref(0, 8, 8) == 0
