"""GPU checks of train2.py's augmentation on the device (csrc/pwc_augment_full.hip, opticalflow_amd/augment_full.py): every output of every
case equals the NumPy oracle (tests/augment_full_oracle.py, the reference's stages in forward order on whole windows) bit for bit -- the
arithmetic is integer, or fp32 / fp64 in a fixed order without fused multiply-add, so there is no tolerance anywhere -- and the status
vector is zero unless a case says otherwise."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_full_oracle as FO  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_augment_full.npz")) as z:
        return {k: z[k] for k in z.files}


_expected = {}


def expected(name, with_valid=True):
    """Oracle outputs of a named case, computed once and shared (read-only) by the tests that need them."""
    key = (name, with_valid)
    if key not in _expected:
        samples, recs, crop, slot = FO.case_inputs(name)
        want = FO.case_expected(samples, recs, crop, with_valid=with_valid)
        for w in want:
            w.setflags(write=False)
        _expected[key] = (samples, recs, crop, slot, want)
    return _expected[key]


def to_params(recs):
    """Oracle record dicts -> the product's FULL_PARAMS_DTYPE array."""
    from opticalflow_amd import augment_full
    p = augment_full.make_full_params(len(recs))
    for i, r in enumerate(recs):
        for k in p.dtype.names:
            p[k][i] = r[k]
    return p


def upload(samples, slot, dev, gt_kind=1, with_valid=True):
    """Host samples (im1, im2, png) -> device slot tensors (frames, gt, valid) in the requested ground-truth form."""
    from opticalflow_amd import augment
    if gt_kind == 0:
        samples = [(a, b, np.stack(FO.decode_png(p)[:2], -1), (p[..., 2] != 0) if with_valid else None) for a, b, p in samples]
    frames, gt, valid, _ = augment.pack_slots(samples, slot, gt_kind)
    return (torch.from_numpy(frames).to(dev), torch.from_numpy(gt).to(dev), None if valid is None else torch.from_numpy(valid).to(dev))


def assert_equal(got, want, status=None):
    for name, g, w in zip(("x", "flow", "mask"), got, want):
        g = g.cpu().numpy()
        assert g.dtype == np.float32 and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
        bad = g != w
        print("%s: %d of %d elements differ" % (name, np.count_nonzero(bad), bad.size))
        assert np.array_equal(g, w), name
    if status is not None:
        assert status.dtype == torch.int32 and not status.cpu().numpy().any()


# ---- every named case, both ground-truth forms: each stage alone and all together with the flip off and on, the ragged window, the
# windows smaller than the halo and the shift, the single row, three tiles in both directions, the extremes, blurred beside plain -----
@pytest.mark.parametrize("gt_kind", [1, 0])
@pytest.mark.parametrize("case", sorted(FO.CASES))
def test_case_equals_the_oracle(dev, case, gt_kind):
    from opticalflow_amd import augment_full
    samples, recs, crop, slot, want = expected(case)
    frames, gt, valid = upload(samples, slot, dev, gt_kind)
    *got, status = augment_full.augment_full_batch(frames, gt, valid, to_params(recs), crop, return_status=True)
    assert got[0].shape == (len(recs), 6) + crop and got[1].shape == (len(recs), 2) + crop and got[2].shape == (len(recs), 1) + crop
    assert_equal(got, want, status)


# ---- no valid plane means every pixel valid; the weights of a rotation add up to exactly 1 ----------------------------------------------
@pytest.mark.parametrize("case", ["stages", "tiny"])
def test_null_valid_is_all_ones(dev, case):
    from opticalflow_amd import augment_full
    samples, recs, crop, slot, want = expected(case, with_valid=False)
    frames, gt, _ = upload(samples, slot, dev, 0, with_valid=False)
    got = augment_full.augment_full_batch(frames, gt, None, to_params(recs), crop)
    assert (got[2] == 1).all()
    assert_equal(got, want)


# ---- misaligned output views take the guarded 4-byte stores: the ragged window, and a window whose width is a multiple of 4 -----------
@pytest.mark.parametrize("case", ["ragged", "tiles"])
def test_misaligned_outputs_take_the_guarded_stores(dev, case):
    from opticalflow_amd import augment_full
    samples, recs, crop, slot, want = expected(case)
    frames, gt, _ = upload(samples, slot, dev, 1)
    n = len(recs)
    bufs = [torch.full((n * c * crop[0] * crop[1] + 2,), float("nan"), device=dev) for c in (6, 2, 1)]
    out = tuple(b[1:-1].view(n, c, *crop) for b, c in zip(bufs, (6, 2, 1)))
    assert all(o.data_ptr() % 16 == 4 for o in out)
    got = augment_full.augment_full_batch(frames, gt, None, to_params(recs), crop, out=out)
    assert_equal(got, want)
    for b in bufs:                                             # nothing written in front of or behind the views
        assert torch.isnan(b[0]) and torch.isnan(b[-1])


# ---- a record the kernel must refuse: zeros and a flag for that sample only ------------------------------------------------------------
def test_out_of_range_records_give_zeros_and_a_flag(dev):
    """The kernel's own bounds CHECK: the host validation is bypassed (ops.kitti_augment_full takes the raw records) and the refused
    samples are never read."""
    from opticalflow_amd import augment_full, ops
    samples, recs, crop, slot, want = expected("mixed")
    n = len(recs)
    p = to_params(recs)
    p["y0"][1] = p["h"][1] - crop[0] + 1                       # origin one row too low
    p["ksize"][2] = 4                                          # a blurred sample with a kernel size that does not exist
    with pytest.raises(ValueError):
        augment_full.augment_full_batch(*upload(samples, slot, dev, 1), p, crop)
    frames, gt, _ = upload(samples, slot, dev, 1)
    pd = torch.from_numpy(p.view(np.uint8).reshape(n, -1)).to(dev)
    out = tuple(torch.full((n, c) + crop, float("nan"), device=dev) for c in (6, 2, 1))
    x, flow, mask, status = ops.kitti_augment_full(frames, gt, pd, crop, out=out, status=torch.full((n,), 7, dtype=torch.int32, device=dev))
    assert status.cpu().tolist() == [0, 1, 1, 0, 0]
    for b in range(n):
        for g, w in zip((x, flow, mask), want):
            g = g[b].cpu().numpy()
            assert np.array_equal(g, np.zeros_like(g) if b in (1, 2) else w[b]), b
    # the other conditions, one record each
    q = to_params(recs)
    bad = np.repeat(q[:1], 12)                                 # sample 0 is blurred
    bad["h"][0], bad["w"][1], bad["h"][2], bad["w"][3], bad["h"][5] = slot[0] + 1, slot[1] + 1, crop[0] - 1, crop[1] - 1, 0
    bad["x0"][4] = bad["w"][4] - crop[1] + 1
    bad["x0"][6], bad["y0"][7] = -1, -1
    bad["ksize"][8] = 9
    bad["wk"][9, 0] += 1                                       # the weights add up to 257
    bad["trans"][10], bad["tx"][10] = 1, 32768
    bad["trans"][11], bad["ty"][11] = 1, -32768
    frames, gt, _ = upload([samples[0]] * 12, slot, dev, 1)
    pd = torch.from_numpy(bad.view(np.uint8).reshape(12, -1)).to(dev)
    x, flow, mask, status = ops.kitti_augment_full(frames, gt, pd, crop)
    assert status.cpu().tolist() == [1] * 12 and not x.any() and not flow.any() and not mask.any()


# ---- the fixture made from the reference's own pipeline class ------------------------------------------------------------------------------
def test_fixture_through_augment_full_batch(dev, gold):
    from opticalflow_amd import augment_full
    samples = [(gold["im1/%d" % i], gold["im2/%d" % i], gold["png/%d" % i]) for i in range(3)]
    sizes = [s[0].shape[:2] for s in samples]
    slot = (max(h for h, _ in sizes), max(w for _, w in sizes))
    crop = tuple(int(v) for v in gold["crop"])
    frames, gt, _ = upload(samples, slot, dev, 1)
    for s in [int(v) for v in gold["seeds"]] + [-1]:          # -1: augment=False under seed 1
        np.random.seed(abs(s))
        p = augment_full.sample_full_params(sizes, crop, augment=s >= 0)
        *got, status = augment_full.augment_full_batch(frames, gt, None, p, crop, return_status=True)
        want = [np.stack([gold["%s/%d/%d" % (k, s, i)] for i in range(3)]) for k in ("x", "flow", "mask")]
        assert_equal(got, want, status)


# ---- one train2.py-shaped call, and the same call twice -------------------------------------------------------------------------------
def test_train2_shaped_batch_on_sampled_rows_and_twice(dev):
    from opticalflow_amd import augment_full
    sizes = [(375, 1242), (370, 1224), (376, 1241), (375, 1242)]
    crop, slot = (320, 896), (376, 1242)
    samples = [FO.make_sample(s, 1600 + i) for i, s in enumerate(sizes)]
    recs = [FO.record(sizes[0], crop, y0=55, x0=346, flip=True, rot=17.0, trans=(-10, 10), bright=1.44, blur=1.5),
            FO.record(sizes[1], crop, y0=0, x0=0, flip=True),
            FO.record(sizes[2], crop, y0=56, x0=345, rot=-17.0, trans=(10, -10), bright=0.64, blur=0.75),
            FO.record(sizes[3], crop, y0=17, x0=101, blur=1.0)]
    frames, gt, _ = upload(samples, slot, dev, 1)
    p = to_params(recs)
    *got, status = augment_full.augment_full_batch(frames, gt, None, p, crop, return_status=True)
    rows = [0] + sorted((1 + np.random.default_rng(5).choice(318, 62, replace=False)).tolist()) + [319]
    assert len(rows) == 64
    want = FO.case_expected(samples, recs, crop, rows=rows)
    assert_equal([g[:, :, rows] for g in got], want, status)
    again = augment_full.augment_full_batch(frames, gt, None, p, crop)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


# ---- the staged path: equal to augment_full_batch, reproducible, and capturable ---------------------------------------------------------
def test_device_full_augmenter_repeats_and_replays_in_a_graph(dev):
    from opticalflow_amd import augment_full
    samples, recs, crop, slot, want = expected("mixed")
    n = len(recs)
    p = to_params(recs)
    aug = augment_full.DeviceFullAugmenter(dev, n + 1, slot, crop, gt_kind=1)
    first = [t.clone() for t in aug(samples, p)]
    assert_equal(first, want, aug.status[:n])
    frames, gt, _ = upload(samples, slot, dev, 1)
    for a, b in zip(first, augment_full.augment_full_batch(frames, gt, None, p, crop)):
        assert torch.equal(a, b)
    for a, b in zip(first, aug(samples, p)):
        assert torch.equal(a, b)
    # records drawn by the augmenter itself, in the reference's order
    np.random.seed(11)
    drawn = aug.stage(samples)
    np.random.seed(11)
    assert drawn.tobytes() == augment_full.sample_full_params([s[0].shape[:2] for s in samples], crop).tobytes()
    drawn_want = FO.case_expected(samples, [{k: r[k] for k in r.dtype.names} for r in drawn], crop)
    aug.upload()
    assert_equal(aug.run(), drawn_want, aug.status[:n])
    # the kernel inside a captured graph: replayed after each stage + upload
    aug.stage(samples, p)
    aug.upload()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        aug.run()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = aug.run()
    for t in (aug.x, aug.flow, aug.mask):
        t.fill_(float("nan"))
    graph.replay()
    assert_equal(outs, want, aug.status[:n])
    aug.stage(samples, drawn)
    aug.upload()
    graph.replay()
    assert_equal(outs, drawn_want, aug.status[:n])
    # float ground truth with a valid plane through the same class
    fl = [(a, b, np.stack(FO.decode_png(g)[:2], -1), g[..., 2] != 0) for a, b, g in samples]
    aug0 = augment_full.DeviceFullAugmenter(dev, n, slot, crop, gt_kind=0)
    assert_equal(aug0(fl, p), want, aug0.status)


# ---- the argument checks with real device pointers: nothing is launched, nothing is written ----------------------------------------
def test_einval_and_ealign_leave_the_outputs_untouched(dev):
    from opticalflow_amd import _lib, ops
    lib = _lib.load()
    samples, recs, crop, slot, _ = expected("mixed")
    frames, gt, _ = upload(samples, slot, dev, 1)
    n = len(recs)
    pd = torch.from_numpy(to_params(recs).view(np.uint8).reshape(n, -1)).to(dev)
    pad = torch.zeros(n * 128 + 8, dtype=torch.uint8, device=dev)
    x = torch.full((n, 6) + crop, -1.0, device=dev)
    flow = torch.full((n, 2) + crop, -1.0, device=dev)
    mask = torch.full((n, 1) + crop, -1.0, device=dev)
    status = torch.full((n,), 7, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(frames=frames.data_ptr(), gt=gt.data_ptr(), kind=1, valid_in=None, n=n, Hs=slot[0], Ws=slot[1], ch=crop[0], cw=crop[1],
             params=pd.data_ptr(), x=x.data_ptr(), flow=flow.data_ptr(), mout=mask.data_ptr(), status=status.data_ptr()):
        return lib.pwc_kitti_augment_full(frames, gt, kind, valid_in, n, Hs, Ws, ch, cw, params, x, flow, mout, status, stream)
    for kw in (dict(frames=None), dict(status=None), dict(n=0), dict(n=65536), dict(Hs=32768), dict(ch=slot[0] + 1), dict(cw=slot[1] + 1),
               dict(kind=2), dict(kind=1, valid_in=frames.data_ptr())):
        assert call(**kw) == -1, kw
    for kw in (dict(x=x.data_ptr() + 2), dict(flow=flow.data_ptr() + 1), dict(mout=mask.data_ptr() + 2), dict(status=status.data_ptr() + 2),
               dict(gt=gt.data_ptr() + 1), dict(kind=0, gt=gt.data_ptr() + 2), dict(params=pad.data_ptr() + 4)):
        assert call(**kw) == -3, kw
    torch.cuda.synchronize(dev)
    assert (x == -1).all() and (flow == -1).all() and (mask == -1).all() and (status == 7).all()
    with pytest.raises(ValueError):
        ops.kitti_augment_full(frames, gt, pd, crop, valid=torch.ones((n,) + slot, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        ops.kitti_augment_full(frames, gt, pd, (slot[0] + 1, crop[1]))
    with pytest.raises(ValueError):
        ops.kitti_augment_full(frames, gt, pd[:, :88].contiguous(), crop)
    with pytest.raises(ValueError):
        ops.kitti_augment_full(frames, gt.cpu(), pd, crop)
