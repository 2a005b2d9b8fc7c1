"""CPU checks of tests/proxy_loss_cases.py, with the fp64 oracle alone: the conditions on the inputs under which a passing
tests/test_gpu_proxy_loss_edges.py means something -- every geometry is one the kernel accepts, a dropped or mis-weighted tail
column / row moves the gradient by at least ten times what the comparator allows, the rough flows leave most samples inside the
border clip and the out-of-bounds flows none -- a negative control per comparator, and a tie of the oracle to the torch route."""
import numpy as np
import pytest
import torch

import proxy_loss_cases as PC
import proxy_loss_oracle as O

IDS = ["%s-%s" % nk for nk in PC.CASE_KINDS]


def test_table_is_the_planned_one():
    geo = {n: tuple(c[:6]) for n, c in PC.CASES.items()}
    assert geo == {"tail-1": (2, 3, 17, 65, 5, 17), "tail-2": (2, 3, 18, 66, 6, 22), "under-tile-same": (1, 3, 15, 63, 15, 63),
                   "same-3-tiles": (1, 3, 20, 130, 20, 130), "min-2x2": (2, 3, 2, 2, 2, 2), "min-3-from-2": (1, 3, 3, 3, 2, 2),
                   "coarse-2x2": (1, 3, 40, 130, 2, 2), "near-1": (1, 3, 33, 70, 32, 69), "row-same": (2, 3, 24, 96, 24, 24),
                   "c1": (2, 1, 17, 65, 5, 17), "c4": (1, 4, 18, 66, 6, 22)}
    assert PC.KINDS == {"rough": tuple(PC.CASES), "zero": ("tail-1",), "oob": ("tail-1", "same-3-tiles")}
    assert (PC.LOSS_RTOL, PC.LOSS_ATOL, PC.GRAD_TOL, PC.SMOOTH_TOL) == (1e-5, 1e-7, 1e-4, 4 * 2.0 ** -24)
    assert PC.SENSITIVITY == 10 * PC.GRAD_TOL == 1e-3 and (PC.WARP32_TOL, PC.WARP64_TOL) == (1e-6, 1e-4)
    assert all(PC.CASES[n].B == 2 for n in PC.STRIDED_CASES)


# ---------------------------------------------------------------- (a) the kernel accepts every geometry
@pytest.mark.parametrize("name", list(PC.CASES))
def test_geometry_is_accepted(name):
    """check_loss_args restated (2 <= h <= H, 2 <= w <= W; ops.proxy_loss_supported answers False off the device), and the
    structural fact each case exists for."""
    from opticalflow_amd import ops
    c = PC.CASES[name]
    assert PC.accepted(c) and 2 <= c.h <= c.H and 2 <= c.w <= c.W and c.C * c.H * c.W < 2 ** 31 and 1 <= c.B <= 65535
    f, (i1, i2) = PC.flow(name), PC.images(name)
    assert tuple(f.shape) == (c.B, 2, c.h, c.w) and tuple(i1.shape) == tuple(i2.shape) == (c.B, c.C, c.H, c.W)
    assert f.dtype == i1.dtype == i2.dtype == torch.float32
    assert not ops.proxy_loss_supported(f, i1, i2)                      # CPU tensors
    tail_h, tail_w = (c.H - 1) % 16 + 1, (c.W - 1) % 64 + 1              # pixels in the last tile row / column
    same = (c.h, c.w) == (c.H, c.W)
    want = {"tail-1": (1, 1, False), "tail-2": (2, 2, False), "under-tile-same": (15, 63, True), "same-3-tiles": (4, 2, True),
            "min-2x2": (2, 2, True), "min-3-from-2": (3, 3, False), "coarse-2x2": (8, 2, False), "near-1": (1, 6, False),
            "row-same": (8, 32, False), "c1": (1, 1, False), "c4": (2, 2, False)}[name]
    assert (tail_h, tail_w, same) == want
    if name == "row-same":
        assert np.float32(c.h - 1) / np.float32(c.H - 1) == 1.0 and c.w < c.W
    if name in ("tail-1", "c1"):
        assert (c.H / c.h, round(c.W / c.w, 2)) == (3.4, 3.82)
    if name == "min-2x2":
        assert c.B * 2 * c.h * (c.w - 1) == 8


# ---------------------------------------------------------------- (b) a wrong tail cannot pass
@pytest.mark.parametrize("name,kind", [nk for nk in PC.CASE_KINDS if nk[1] != "oob"], ids=[i for i in IDS if not i.endswith("oob")])
def test_tail_column_and_row_move_the_gradient(name, kind):
    """Masking out the last image column, and the last row, changes the den-normalised photo-only oracle gradient by at least
    10 x the comparator's bound: a kernel that drops or mis-weights that column / row is at least 10 bounds off.  (The oob kind
    has no photometric gradient at all: what it checks is the exact zero.)"""
    col, row = PC.tail_sensitivity(name, kind)
    print("[proxy-cases] %s-%s: last column moves the gradient by %.2e of max|g|, last row by %.2e (needed %.0e)"
          % (name, kind, col, row, PC.SENSITIVITY))
    assert col >= PC.SENSITIVITY and row >= PC.SENSITIVITY, (name, kind, col, row)


# ---------------------------------------------------------------- (c) the border clip
@pytest.mark.parametrize("name,kind", PC.CASE_KINDS, ids=IDS)
def test_border_clip_shares(name, kind):
    both, sx, sy = PC.clip_pass(name, kind)
    print("[proxy-cases] %s-%s: %.0f %% of the samples pass the clip on both axes (x %.0f %%, y %.0f %%)"
          % (name, kind, 100 * both, 100 * sx, 100 * sy))
    if kind == "rough":
        assert both >= 0.5
    elif kind == "oob":
        assert sx == 0.0 and sy == 0.0
        for eps in PC.EPS:
            loss, g = PC.oracle(name, kind, eps, "photo")
            assert not g.any() and loss[1] > 0
            PC.check_axis_zero(g)
    _, gs = PC.oracle(name, kind, 0.0, "smooth")
    assert gs.any() == (kind == "rough")                  # constant flows: |0| has gradient 0


def test_rough_flows_reach_both_sides_of_the_clip():
    """somewhere in the table the rough kind also fails the clip on each axis, so both of the kernel's branches run"""
    shares = np.array([PC.clip_pass(n, "rough")[1:] for n in PC.CASES])
    assert (shares[:, 0] < 1).any() and (shares[:, 1] < 1).any()


# ---------------------------------------------------------------- masks
@pytest.mark.parametrize("name", PC.MASK_CASES)
def test_mask_kinds(name):
    c = PC.CASES[name]
    tail = PC.tail_region(c.H, c.W)
    assert tail[c.H - 1].all() and tail[:, c.W - 1].all() and not tail[0, 0] and tail[16, 0] and tail[0, (c.W - 1) // 64 * 64]
    for kind in PC.MASK_KINDS:
        on, val = PC.mask_pattern(kind, name)
        assert on.shape == val.shape == (c.B, c.H, c.W) and val.dtype == np.float32
        assert np.array_equal(val > 0.5, on)
        var = PC.mask_variants(kind, name)
        assert [t for t, _ in var] == ["float32-3d", "float32-4d", "bool-3d", "bool-4d", "uint8-3d", "uint8-4d"]
        for tag, m in var:
            assert str(m.dtype) == "torch." + tag[:-3] and m.dim() == int(tag[-2])
            assert np.array_equal((m.float() > 0.5).numpy().reshape(on.shape), on), (kind, tag)
        if kind == "edge":
            assert on.sum() == c.B * (c.H + c.W - 1) and on[:, -1].all() and on[:, :, -1].all()
        elif kind == "corner":
            assert on.sum() == 2 * c.B and on[:, 15, 63].all() and on[:, 16, 64].all()
        elif kind == "off":
            assert not on.any()
        else:
            half, nxt = np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(1.0))
            t = np.broadcast_to(tail, on.shape)
            assert set(np.unique(val[t])) == {half, nxt} and set(np.unique(val[~t])) == {np.float32(0.0), np.float32(1.0)}
            assert (val[t] == half).sum() > 10 and (val[t] == nxt).sum() > 10 and nxt > 0.5
        if kind != "off":
            assert (var[4][1] == 255).any() and (var[4][1] == 1).any()
        # the masked oracle: photo is a mean over the kept pixels; nothing kept gives exactly 0 and no photometric gradient
        loss, g = PC.oracle(name, "rough", 0.0, "photo", kind)
        assert (loss[1] == 0.0 and not g.any()) if kind == "off" else (loss[1] > 0 and g.any())


# ---------------------------------------------------------------- (d) every comparator passes on the oracle and can fail
@pytest.mark.parametrize("name,kind", PC.CASE_KINDS, ids=IDS)
def test_comparators_pass_on_the_oracle_and_fail_two_bounds_off(name, kind):
    c = PC.CASES[name]
    for which in PC.GRAD_OUTS:
        loss, g = PC.oracle(name, kind, 0.0, which)
        assert PC.check_losses(loss, loss) == 0.0 and PC.check_grad(g, g, which) == 0.0
        for k in range(3):
            bad = loss.copy()
            bad[k] += 2.0 * (PC.LOSS_ATOL + PC.LOSS_RTOL * abs(loss[k]))
            with pytest.raises(AssertionError):
                PC.check_losses(bad, loss)
            ok = loss.copy()
            ok[k] += 0.5 * (PC.LOSS_ATOL + PC.LOSS_RTOL * abs(loss[k]))
            assert 0.49 < PC.check_losses(ok, loss) < 0.51
        gmax = np.abs(g).max()
        # one element of the tail: the last low-resolution row and column of the last image, either plane
        for pl in (0, 1):
            bad = g.copy()
            bad[c.B - 1, pl, c.h - 1, c.w - 1] += 2.0 * PC.GRAD_TOLS[which] * gmax if gmax else 1e-30
            with pytest.raises(AssertionError):
                PC.check_grad(bad, g, which)
            if gmax:
                ok = g.copy()
                ok[c.B - 1, pl, c.h - 1, c.w - 1] -= 0.5 * PC.GRAD_TOLS[which] * gmax
                assert 0.49 < PC.check_grad(ok, g, which) < 0.51
            else:
                with pytest.raises(AssertionError):
                    PC.check_axis_zero(bad, (pl,))
                PC.check_axis_zero(bad, (1 - pl,))
        nan = g.copy()
        nan[0, 0, 0, 0] = np.nan
        with pytest.raises(AssertionError):
            PC.check_grad(nan, g, which)
    with pytest.raises(AssertionError):
        PC.check_losses(np.array([np.nan, loss[1], loss[2]]), loss)


def test_oracle_results_are_shared_and_read_only():
    a, b = PC.oracle("tail-1"), PC.oracle("tail-1", "rough", 0.0, "total")
    assert a[0] is b[0] and a[1] is b[1] and not a[1].flags.writeable
    f = PC.flow("tail-1")
    f.zero_()
    assert PC.flow("tail-1").abs().max() > 0


# ---------------------------------------------------------------- (e) the oracle is tied to the reference expression
@pytest.mark.parametrize("name,kind", PC.CASE_KINDS, ids=IDS)
def test_oracle_agrees_with_the_torch_route_fp64(name, kind):
    """ProxyLabelLoss(route="torch") in float64 against the oracle's loss values, 1e-6 relative, both variants; on the mask cases
    with every mask kind too.  A sanity tie: the oracle evaluates the kernel's float32 sample points and float32 constants.  No
    case is left out."""
    from opticalflow_amd.losses import ProxyLabelLoss
    f, (i1, i2) = PC.flow(name, kind).double(), tuple(t.double() for t in PC.images(name))
    worst = 0.0
    masks = (None,) + (PC.MASK_KINDS if name in PC.MASK_CASES and kind == "rough" else ())
    for variant, eps in zip(("pseudo", "fundamental"), PC.EPS):
        for mk in masks:
            m = None if mk is None else torch.from_numpy(PC.mask_pattern(mk, name)[1])
            got = [t.item() for t in ProxyLabelLoss(variant=variant, route="torch")(f, i1, i2, m)]
            ref = PC.oracle(name, kind, eps, "photo", mk)[0]
            for a, b in zip(got, ref):
                assert abs(a - b) <= 1e-6 * abs(b), (name, kind, variant, mk, got, ref)
                worst = max(worst, abs(a - b) / abs(b) if b else 0.0)
    print("[proxy-cases] %s-%s: torch route (float64) vs oracle, worst relative loss difference %.1e" % (name, kind, worst))


def test_warp_restatements_agree():
    """O.warp32 (the kernel's float32 warp) against O.warp_image64 on every case: the two references of the warp test are within
    the tighter of its two bounds of each other, so neither bound rests on the other reference's error."""
    for name in PC.CASES:
        img, _ = PC.images(name)
        f = PC.flow(name)
        d = (O.warp32(img, f).double() - O.warp_image64(img, f)).abs().max().item()
        assert d <= PC.WARP32_TOL * img.abs().max().item(), (name, d)
