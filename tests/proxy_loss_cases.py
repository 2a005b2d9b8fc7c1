"""Ragged cases of the proxy-label loss (csrc/pwc_proxy_loss.hip) and the comparators its GPU tests use.  A helper, not a test
module: tests/test_proxy_loss_cases_cpu.py pins the conditions on the inputs under which a passing GPU test means something and
shows that every comparator can fail; tests/test_gpu_proxy_loss_edges.py runs the kernels on the cases against the fp64 oracle
(tests/proxy_loss_oracle.py).

tests/test_gpu_proxy_loss.py runs the oracle at 384 x 512, 448 x 1024, 96 x 160 and 64 x 96 with flows at exactly a quarter of the
image: whole 16 x 64 tiles or tails of 32 columns, one upsampling ratio, three channels, dense operands.  The geometries here
(B, C, H, W, h, w) are the smallest at which each of the kernel's paths can still go wrong:

  tail-1            2 x 3 x 17 x 65 from 5 x 17: the last tile row and column hold one pixel; their forward halo and both backward
                    halo columns lie past the image; ratios 3.4 and 3.82
  tail-2            2 x 3 x 18 x 66 from 6 x 22: the tail is as wide as the backward halo; ratio 3 in both axes
  under-tile-same   1 x 3 x 15 x 63, flow at image size: one workgroup, ragged on both sides
  same-3-tiles      1 x 3 x 20 x 130, flow at image size: tile borders inside the image, a 2-column and a 4-row tail
  min-2x2           2 x 3 x 2 x 2 from 2 x 2: the smallest accepted call (nx = B 2 h (w - 1) = 8)
  min-3-from-2      1 x 3 x 3 x 3 from 2 x 2: the smallest upsampling call
  coarse-2x2        1 x 3 x 40 x 130 from 2 x 2: four gather lanes walk the whole image
  near-1            1 x 3 x 33 x 70 from 32 x 69: a ratio just under 1 (first_user's estimate and its walk)
  row-same          2 x 3 x 24 x 96 from 24 x 24: h = H with w < W, the upsampling path with rh = 1.0
  c1, c4            tail-1 with one channel, tail-2 (B = 1) with four: the weights 0.85 / C and 0.15 / C

Flow kinds: "rough" (every case) is a contraction towards the image centre plus a smooth field plus noise, given in image pixels
and divided by the vector scale (W / w, H / h), so that most samples stay inside the border clip; "zero"; "oob", a constant flow
larger than the image, every sample clipped on both axes.  Mask kinds (MASK_KINDS) on MASK_CASES, each as bool, uint8 and float32
and as [B,H,W] and [B,1,H,W].
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import proxy_loss_oracle as O

# pull: inward displacement of the border pixels (image pixels); amp: amplitude of the smooth + noise part (image pixels)
Case = namedtuple("Case", "B C H W h w pull amp")
CASES = {
    "tail-1": Case(2, 3, 17, 65, 5, 17, 2.0, 3.0),
    "tail-2": Case(2, 3, 18, 66, 6, 22, 2.0, 3.0),
    "under-tile-same": Case(1, 3, 15, 63, 15, 63, 2.0, 3.0),
    "same-3-tiles": Case(1, 3, 20, 130, 20, 130, 2.0, 3.0),
    "min-2x2": Case(2, 3, 2, 2, 2, 2, 0.5, 0.25),
    "min-3-from-2": Case(1, 3, 3, 3, 2, 2, 0.5, 0.25),
    "coarse-2x2": Case(1, 3, 40, 130, 2, 2, 4.0, 2.5),
    "near-1": Case(1, 3, 33, 70, 32, 69, 2.0, 3.0),
    "row-same": Case(2, 3, 24, 96, 24, 24, 2.0, 3.0),
    "c1": Case(2, 1, 17, 65, 5, 17, 2.0, 3.0),
    "c4": Case(1, 4, 18, 66, 6, 22, 2.0, 3.0),
}
KINDS = {"rough": tuple(CASES), "zero": ("tail-1",), "oob": ("tail-1", "same-3-tiles")}
CASE_KINDS = tuple((n, k) for k, names in KINDS.items() for n in names)
MASK_CASES = ("tail-1", "same-3-tiles")
MASK_KINDS = ("edge", "corner", "off", "half")
STRIDED_CASES = ("tail-1", "tail-2")
MODULE_CASES = ("tail-1", "min-2x2", "coarse-2x2")
EPS = (0.0, 1e-12)                      # the SSIM eps of the two variants
GRAD_OUTS = {"photo": (0.0, 1.0, 0.0), "total": (1.0, 0.0, 0.0), "smooth": (0.0, 0.0, 1.0)}

LOSS_RTOL, LOSS_ATOL = 1e-5, 1e-7       # (total, photo, smooth): _check_oracle of test_gpu_proxy_loss.py
GRAD_TOL = 1e-4                         # photo-only and total gradient, per element, of max|g_ref|: _check_oracle
# smooth only: gs * (tx / nx + ty / ny) with small integers tx, ty over the counts nx, ny: two quotients, one sum and one product,
# four float32 roundings of values no larger than the result's largest entry
SMOOTH_TOL = 4.0 * 2.0 ** -24
GRAD_TOLS = {"photo": GRAD_TOL, "total": GRAD_TOL, "smooth": SMOOTH_TOL}
SENSITIVITY = 10.0 * GRAD_TOL           # what masking out the last image row / column must change (condition b)
WARP32_TOL, WARP64_TOL = 1e-6, 1e-4     # of max|img|: test_warp_image_against_oracle


def accepted(c):
    """The kernel's acceptance rule (check_loss_args): 2 <= h <= H and 2 <= w <= W."""
    return 2 <= c.h <= c.H and 2 <= c.w <= c.W


def _seed(name):
    return 100 + 10 * list(CASES).index(name)


@functools.lru_cache(maxsize=None)
def _images(name, C=None):
    """The image recipe of test_gpu_proxy_loss.py (a sine, a step, noise; img2 = img1 rolled by (2, -3) plus noise)."""
    c = CASES[name]
    C = c.C if C is None else C
    gen = torch.Generator().manual_seed(_seed(name))
    yy, xx = torch.meshgrid(torch.arange(c.H, dtype=torch.float32), torch.arange(c.W, dtype=torch.float32), indexing="ij")
    base = torch.sin(0.07 * xx + 0.05 * yy)[None, None] + 0.5 * (xx > c.W / 3).float()[None, None]
    img1 = (base + 0.3 * torch.rand(c.B, C, c.H, c.W, generator=gen)).clamp(-1, 2) * 1.5 - 0.6
    img2 = torch.roll(img1, shifts=(2, -3), dims=(2, 3)) + 0.05 * torch.randn(c.B, C, c.H, c.W, generator=gen)
    return img1, img2


def images(name, C=None):
    """(img1, img2) float32 [B,C,H,W] on the CPU (fresh copies)."""
    return tuple(t.clone() for t in _images(name, C))


@functools.lru_cache(maxsize=None)
def _flow(name, kind):
    c = CASES[name]
    if kind == "zero":
        return torch.zeros(c.B, 2, c.h, c.w)
    if kind == "oob":
        f = torch.empty(c.B, 2, c.h, c.w)
        f[:, 0] = (c.W + 3.0) * c.w / c.W           # past the right edge from every column
        f[:, 1] = -(c.H + 3.0) * c.h / c.H          # above the top edge from every row
        return f
    assert kind == "rough", kind
    gen = torch.Generator().manual_seed(_seed(name) + 1)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, c.h), torch.linspace(0, 1, c.w), indexing="ij")
    pull = torch.stack((2.0 * c.pull * (0.5 - xx), 2.0 * c.pull * (0.5 - yy)))
    smooth = torch.stack((0.75 * torch.sin(4 * xx + yy), 0.5 * torch.cos(3 * yy - xx)))
    f = pull[None] + c.amp * (smooth[None] + torch.randn(c.B, 2, c.h, c.w, generator=gen))
    f[:, 0] *= c.w / c.W
    f[:, 1] *= c.h / c.H
    return f


def flow(name, kind="rough"):
    """float32 [B,2,h,w] on the CPU (a fresh copy)."""
    return _flow(name, kind).clone()


def clip_pass(name, kind):
    """(share of the pixels whose sample point passes the border clip on both axes, share that passes on x, share on y)."""
    c = CASES[name]
    px, py = O.sample_points32(_flow(name, kind), c.H, c.W)
    inx, iny = (px > 0) & (px < c.W - 1), (py > 0) & (py < c.H - 1)
    return (inx & iny).float().mean().item(), inx.float().mean().item(), iny.float().mean().item()


# ---------------------------------------------------------------- masks
def tail_region(H, W):
    """bool [H,W]: the pixels of the last tile row and the last tile column (16 x 64 tiles)."""
    t = np.zeros((H, W), bool)
    t[(H - 1) // 16 * 16:, :] = True
    t[:, (W - 1) // 64 * 64:] = True
    return t


def mask_pattern(kind, name):
    """(on [B,H,W] bool, float32 values [B,H,W]) of a mask kind.  The float values are 1 / 0 except for "half": there the tail
    region holds exactly 0.5 where the pattern is off (the rule is `> 0.5`) and the next float above 0.5 where it is on."""
    c = CASES[name]
    on = np.zeros((c.B, c.H, c.W), bool)
    if kind == "edge":
        on[:, c.H - 1, :] = True
        on[:, :, c.W - 1] = True
    elif kind == "corner":
        assert c.H > 16 and c.W > 64
        on[:, 15, 63] = True
        on[:, 16, 64] = True
    elif kind == "half":
        on[:] = np.random.default_rng(_seed(name) + 2).random((c.B, c.H, c.W)) < 0.5
    else:
        assert kind == "off", kind
    val = on.astype(np.float32)
    if kind == "half":
        t = np.broadcast_to(tail_region(c.H, c.W), on.shape)
        val[t & on] = np.nextafter(np.float32(0.5), np.float32(1.0))
        val[t & ~on] = np.float32(0.5)
    return on, val


def mask_variants(kind, name):
    """[(tag, tensor)]: the mask as bool, uint8 (on = 1, every third on-pixel 255) and float32, each as [B,H,W] and [B,1,H,W].
    The first entry is the float32 [B,H,W] one."""
    c = CASES[name]
    on, val = mask_pattern(kind, name)
    u8 = on.astype(np.uint8)
    idx = np.flatnonzero(on.ravel())[::3]
    u8.ravel()[idx] = 255
    out = []
    for tag, arr in (("float32", val), ("bool", on), ("uint8", u8)):
        for shape in ((c.B, c.H, c.W), (c.B, 1, c.H, c.W)):
            out.append(("%s-%dd" % (tag, len(shape)), torch.from_numpy(arr.copy()).view(shape)))
    return out


# ---------------------------------------------------------------- oracle results (computed once per process, never modified)
@functools.lru_cache(maxsize=None)
def _oracle(name, kind, eps, which, mask_kind=None, alpha_photo=1.0, alpha_smooth=0.1):
    img1, img2 = _images(name)
    mask = None if mask_kind is None else torch.from_numpy(mask_pattern(mask_kind, name)[1])
    loss, g = O.proxy_loss64(_flow(name, kind), img1, img2, mask, alpha_photo, alpha_smooth, eps, GRAD_OUTS[which])
    loss, g = loss.numpy(), g.numpy()
    loss.setflags(write=False)
    g.setflags(write=False)
    return loss, g


def oracle(name, kind="rough", eps=0.0, which="total", mask_kind=None):
    """((total, photo, smooth) float64 [3], grad_flow float64 [B,2,h,w]) for the upstream gradient GRAD_OUTS[which], as read-only
    NumPy arrays."""
    return _oracle(name, kind, float(eps), which, mask_kind)


def oracle_with_mask(name, kind, mask_on, which="photo"):
    """The oracle with an explicit bool mask [B,H,W] (not cached): (loss, grad, number of pixels the mask keeps)."""
    img1, img2 = _images(name)
    m = torch.from_numpy(np.ascontiguousarray(mask_on))
    loss, g = O.proxy_loss64(_flow(name, kind), img1, img2, m, 1.0, 0.1, 0.0, GRAD_OUTS[which])
    return loss.numpy(), g.numpy(), max(int(mask_on.sum()), 1)


def tail_sensitivity(name, kind):
    """(column, row): how far the den-normalised photo-only oracle gradient moves, as a share of its largest entry, when the last
    image column / the last image row is masked out.  den-normalised: each gradient times its own pixel count, so that the
    change of the mean's denominator does not count."""
    c = CASES[name]
    full = np.ones((c.B, c.H, c.W), bool)
    _, g0, n0 = oracle_with_mask(name, kind, full)
    g0 = g0 * n0
    out = []
    for sl in ((slice(None), slice(None), c.W - 1), (slice(None), c.H - 1, slice(None))):
        m = full.copy()
        m[sl] = False
        _, g1, n1 = oracle_with_mask(name, kind, m)
        out.append(float(np.abs(g1 * n1 - g0).max() / np.abs(g0).max()))
    return tuple(out)


# ---------------------------------------------------------------- comparators (pure NumPy, on downloaded arrays)
def check_losses(out, ref):
    """(total, photo, smooth) within LOSS_RTOL |ref| + LOSS_ATOL each.  Returns the worst error / bound."""
    out, ref = np.asarray(out, np.float64).reshape(3), np.asarray(ref, np.float64).reshape(3)
    bound = LOSS_ATOL + LOSS_RTOL * np.abs(ref)
    ratio = np.abs(out - ref) / bound
    assert np.all(ratio <= 1.0), "loss %s, oracle %s: error / bound %s" % (out, ref, ratio)     # also fails on NaN
    return float(ratio.max())


def check_grad(g, gref, which):
    """grad_flow against the oracle's for the upstream gradient `which`: every element within GRAD_TOLS[which] of the oracle's
    largest entry; exactly 0 everywhere when the oracle's gradient is.  Returns the worst error / bound."""
    g, gref = np.asarray(g, np.float64), np.asarray(gref, np.float64)
    assert g.shape == gref.shape, (g.shape, gref.shape)
    gmax = np.abs(gref).max()
    if gmax == 0.0:
        assert not g.any(), "%s gradient: the oracle's is exactly 0, %d entries are not" % (which, int(np.count_nonzero(g)))
        return 0.0
    bound = GRAD_TOLS[which] * gmax
    err = np.abs(g - gref)
    worst = float(err.max() / bound)
    assert np.all(err <= bound), ("%s gradient: error %.3e at %s, bound %.3e (%.2f x)"         # also fails on NaN
                                  % (which, err.max(), np.unravel_index(np.nanargmax(err), err.shape), bound, worst))
    return worst


def check_axis_zero(g, axes=(0, 1)):
    """The photo-only gradient planes of these axes (0 = u, 1 = v) are exactly 0.0: the kernel stores 0 at full resolution
    wherever the clip removes the axis's gradient or the mask is off, and the gather sums zeros."""
    g = np.asarray(g)
    for ax in axes:
        assert not g[:, ax].any(), "plane %d: %d entries are not exactly 0" % (ax, int(np.count_nonzero(g[:, ax])))
